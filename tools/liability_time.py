"""What liability traits (ngp_set_liability_classes / ngp_set_liability_bounds) cost per iteration at the bench's 10k x 100k BayesPR shape:
device time per iteration from the HIP events of ngp_run (ngp_get_timing) with no liabilities, with classes on every record (C = 2 and
C = 4) and with 30 % of the records censored.  The sweep kernel is the same in all; a liability chain launches k_liability_augment (and
k_thresholds for C >= 3) in front of k_head.  Every leg runs in fresh processes (one per repeat, legs interleaved), as a comparison of two
builds must; the table reports the median and the range per leg.

    python tools/liability_time.py                         # the four legs, 3 fresh processes each
    python tools/liability_time.py --leg classes4          # one leg in this process (what the children run)
    python tools/liability_time.py --parent-lib build_ab/libparent.so   # a fifth leg: "none" on a library built from the parent commit
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

LEGS = ("none", "classes2", "classes4", "censored30")
N, P = 10_000, 100_000


def one(leg, warm, iters):
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
    v = 0.5 * y.var() / (s.mpm().sum() / N)
    if leg.startswith("classes"):
        C_ = int(leg[-1])
        cuts = np.quantile(z, np.arange(1, C_) / C_)
        s.set_classes((1 + np.digitize(z, cuts)).astype(np.int32), C_)
        v = v / y.var()                               # the liability has residual variance 1
    elif leg == "censored30":
        rows = np.flatnonzero(z > np.quantile(z, 0.7)).astype(np.int64)
        s.set_censored(rows, np.full(len(rows), np.quantile(y, 0.7)), np.full(len(rows), np.inf))
    s.add_marker_set(0, P, 0, 4.0, v * 0.5, [(0, P)], [v])
    s.set_y(y)
    s.set_residual_prior(4.0, 0.25 * y.var())
    s.run(warm)
    s.get_timing()                                    # (resets the accumulated device time)
    s.run(iters)
    t = s.get_timing()
    try:
        fell = s.liability_fallthrough()
    except AttributeError:                            # (a parent build's library has no such entry point)
        fell = 0
    s.close()
    return dict(leg=leg, ms=t["iter_ms"] / t["iters"], fallthrough=fell)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=LEGS)
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args()
    if a.leg:
        print(json.dumps(one(a.leg, a.warmup, a.iters)), flush=True)
        return
    legs = (["parent"] if a.parent_lib else []) + a.legs.split(",")
    ms = {leg: [] for leg in legs}
    for _ in range(a.repeats):                        # interleaved: drift of the machine hits every leg alike
        for leg in legs:
            env = dict(os.environ, NGP_HIP_LIB=os.path.abspath(a.parent_lib)) if leg == "parent" else None
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", "none" if leg == "parent" else leg, "--warmup", str(a.warmup),
                                  "--iters", str(a.iters)], check=True, capture_output=True, text=True, timeout=600, env=env).stdout
            r = json.loads(out.strip().splitlines()[-1])
            assert r["fallthrough"] == 0, r
            ms[leg].append(r["ms"])
            print(f"{leg}: {r['ms']:.4f} ms/iter", flush=True)
    base = float(np.median(ms[legs[0]]))
    for leg in legs:
        m = float(np.median(ms[leg]))
        print(f"{leg:11s} median {m:.4f} ms/iter (min {min(ms[leg]):.4f}, max {max(ms[leg]):.4f}; {a.repeats} fresh processes)"
              f"  {m / base:.4f} x {legs[0]}", flush=True)


if __name__ == "__main__":
    main()
