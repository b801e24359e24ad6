"""What the threshold step of an ordered trait costs per iteration at the bench's 10k x 100k BayesPR shape: device time per iteration from
the HIP events of ngp_run (ngp_get_timing) of a three-class chain under Albert-Chib (mode 0: k_thresholds), under Cowles' step (mode 1:
k_threshold_terms + k_threshold_decide), and under Cowles' step with 2,000 records held out and their class probabilities accumulated
(k_holdout_prob, every iteration kept).  The sweep kernel is the same in all.  Every leg runs in fresh processes (one per repeat, legs
interleaved), as a comparison of two builds must; the table reports the median and the range per leg.

    python tools/threshold_time.py                         # the legs, 3 fresh processes each
    python tools/threshold_time.py --leg cowles            # one leg in this process (what the children run)
    python tools/threshold_time.py --parent-lib build_ab/libparent.so   # another leg: "albert-chib" on a library built from the parent commit
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ngp_pkg import load_pkg  # noqa: E402

LEGS = ("albert-chib", "cowles", "cowles-prob")
N, P = 10_000, 100_000


def one(leg, warm, iters, parent):
    ngp = load_pkg()
    s = ngp.Sampler(device=0, seed=1001, chain=0)
    s.generate_panel(N, P)
    rng = np.random.default_rng(1)
    bt = np.zeros(P)
    idx = rng.choice(P, P // 100, replace=False)
    bt[idx] = rng.normal(size=len(idx))
    g = s.xbeta(bt)
    y = 10.0 + g + np.random.default_rng(2).normal(size=N) * np.sqrt(g.var())
    z = (y - y.mean()) / y.std()
    v = 0.5 / (s.mpm().sum() / N)                     # the liability has residual variance 1
    if leg == "cowles-prob":
        s.set_holdout(np.arange(0, N, 5))
    s.set_classes((1 + np.digitize(z, np.quantile(z, [1 / 3, 2 / 3]))).astype(np.int32), 3)
    if leg != "albert-chib":
        s.set_threshold_step("cowles")
    elif not parent:
        s.set_threshold_step("albert-chib")
    if leg == "cowles-prob":
        s.enable_class_probabilities()
    s.add_marker_set(0, P, 0, 4.0, v * 0.5, [(0, P)], [v])
    s.set_y(y)
    s.set_schedule(warm + iters, warm, 1)
    s.run(warm)
    s.get_timing()                                    # (resets the accumulated device time)
    s.run(iters)
    t = s.get_timing()
    out = dict(leg=leg, ms=t["iter_ms"] / t["iters"], fallthrough=s.liability_fallthrough())
    if leg != "albert-chib":
        ts = s.threshold_step()
        out.update(acceptance=ts["accepted"] / max(ts["tries"], 1), sigma=ts["sigma"])
    s.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent", action="store_true", help="(children) the library is the parent's: call nothing it does not have")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args()
    if a.leg:
        print(json.dumps(one(a.leg, a.warmup, a.iters, a.parent)), flush=True)
        return
    legs = (["parent"] if a.parent_lib else []) + a.legs.split(",")
    ms = {leg: [] for leg in legs}
    for _ in range(a.repeats):                        # interleaved: drift of the machine hits every leg alike
        for leg in legs:
            env = dict(os.environ, NGP_HIP_LIB=os.path.abspath(a.parent_lib)) if leg == "parent" else None
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", "albert-chib" if leg == "parent" else leg, "--warmup", str(a.warmup),
                   "--iters", str(a.iters)] + (["--parent"] if leg == "parent" else [])
            out = subprocess.run(cmd, check=True, capture_output=True, text=True, timeout=600, env=env).stdout
            r = json.loads(out.strip().splitlines()[-1])
            assert r["fallthrough"] == 0, r
            ms[leg].append(r["ms"])
            print(f"{leg}: {r['ms']:.4f} ms/iter" + (f" (acceptance {r['acceptance']:.3f}, sigma {r['sigma']:.5f})" if "sigma" in r else ""), flush=True)
    base = float(np.median(ms[legs[0]]))
    for leg in legs:
        m = float(np.median(ms[leg]))
        print(f"{leg:11s} median {m:.4f} ms/iter (min {min(ms[leg]):.4f}, max {max(ms[leg]):.4f}; {a.repeats} fresh processes)"
              f"  {m / base:.4f} x {legs[0]}", flush=True)


if __name__ == "__main__":
    main()
