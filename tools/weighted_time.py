"""What weighted residuals (ngp_set_residual_weights) cost per iteration: the same model run unweighted and weighted, device time per
iteration from the HIP events of ngp_run (ngp_get_timing).  The sweep kernel is the same in both; only k_head reads one more N-vector.

    python tools/weighted_time.py                       # 10k x 100k BayesPR, 10k x 100k BayesR, 50k x 600k 3 x BayesPR
    python tools/weighted_time.py --cases pr10k --only w  # one leg (e.g. under rocprofv3 --kernel-trace --stats)
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ngp_pkg import load_pkg  # noqa: E402

CASES = {  # name: (N, P, sets)
    "pr10k": (10_000, 100_000, "pr1"),
    "r10k": (10_000, 100_000, "r"),
    "pr50k": (50_000, 600_000, "pr3"),
}


def one(ngp, N, P, sets, weighted, warm, iters):
    s = ngp.Sampler(device=0, seed=1001, chain=0)
    if weighted:
        s.set_residual_weights(np.random.default_rng(5).uniform(0.2, 5.0, N))
    s.generate_panel(N, P)
    rng = np.random.default_rng(1)
    bt = np.zeros(P)
    idx = rng.choice(P, P // 100, replace=False)
    bt[idx] = rng.normal(size=len(idx))
    g = s.xbeta(bt)
    y = 10.0 + g + np.random.default_rng(2).normal(size=N) * np.sqrt(g.var())
    v = 0.5 * y.var() / (s.mpm().sum() / N)
    if sets == "r":
        s.add_marker_set_r(0, P, 4.0, v * 0.5, v, [0.0, 0.01, 0.1, 1.0], [0.95, 0.03, 0.015, 0.005], estPi=True)
    else:
        k = 3 if sets == "pr3" else 1
        for j in range(k):
            c0, c1 = j * P // k, (j + 1) * P // k
            s.add_marker_set(c0, c1 - c0, 0, 4.0, v * 0.5, [(0, c1 - c0)], [v])
    s.set_y(y)
    s.set_residual_prior(4.0, 0.25 * y.var())
    s.run(warm)
    s.get_timing()                        # (resets the accumulated device time)
    s.run(iters)
    t = s.get_timing()
    st = s.get_state()
    s.close()
    return t["iter_ms"] / t["iters"], st["varE"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--only", choices=["u", "w", "both"], default="both")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=30)
    a = ap.parse_args()
    ngp = load_pkg()
    for name in a.cases.split(","):
        N, P, sets = CASES[name]
        res = {}
        for wt in ([False, True] if a.only == "both" else [a.only == "w"]):
            ms, varE = one(ngp, N, P, sets, wt, a.warmup, a.iters)
            res[wt] = ms
            print(f"{name} {N}x{P} {'weighted  ' if wt else 'unweighted'}: {ms:.3f} ms/iter ({1e3 / ms:.1f} it/s), varE {varE:.4g}", flush=True)
        if len(res) == 2:
            print(f"{name}: weighted / unweighted = {res[True] / res[False]:.4f}", flush=True)


if __name__ == "__main__":
    main()
