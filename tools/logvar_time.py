"""Device time per iteration of a BayesLV set (ngp_logvar.h behind the BayesPR sweep) at 10,000 x 100,000 and 50,000 x 600,000 with
ncov = 3 and 16, varZeta fixed (mode 0) and estimated (mode 1), beside a BayesPR set with one region per locus at the same shape: the
sweep of the two is the same, so the difference is the variance step (five or six small launches against k_regssq + k_regdraw over
one region per locus).  One panel per shape, shared by the runs (ngp_share_panel).

    python tools/logvar_time.py [--iters 20] [--shapes 10000x100000,50000x600000] [--ncov 3,16] [--only-pr]

--only-pr times the BayesPR comparator alone: run it with NGP_HIP_LIB pointing at another build of the library (the parent commit's)
to have that build's number from the same machine.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ngp_pkg import load_pkg  # noqa: E402


def timed(s, y, iters):
    s.set_y(y)
    s.set_residual_prior(4.0, 0.5)
    s.run(3)
    s.get_timing()                                   # (reading the timers clears them)
    s.run(iters)
    t = s.get_timing()
    return t["iter_ms"] / max(t["iters"], 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--shapes", default="10000x100000,50000x600000")
    ap.add_argument("--only-pr", action="store_true")
    ap.add_argument("--ncov", default="3,16")
    a = ap.parse_args()
    ngp = load_pkg()
    out = dict(iters=a.iters, lib=os.environ.get("NGP_HIP_LIB", "this tree"), shapes={})
    for shape in a.shapes.split(","):
        N, P = (int(v) for v in shape.split("x"))
        rng = np.random.default_rng(1)
        y = rng.normal(size=N) + 5.0
        owner = ngp.Sampler(device=0, seed=3, chain=0)
        owner.generate_panel(N, P)
        res = {}

        def sharer(chain):
            s = ngp.Sampler(device=0, seed=3, chain=chain)
            s.share_panel(owner)
            return s
        s = sharer(1)
        s.add_marker_set(0, P, 0, 4.0, 0.0005, [(j, j + 1) for j in range(P)], [0.001] * P)
        res["bayespr_one_region_per_locus_ms"] = timed(s, y, a.iters)
        s.close()
        if not a.only_pr:
            for ncov in (int(v) for v in a.ncov.split(",")):
                C = rng.normal(size=(P, ncov))
                C[:, 0] = 1.0
                for mode in (0, 1):
                    s = sharer(2)
                    s.add_marker_set_lv(0, P, 0.001, C, 0.5, est_mode=mode)
                    ms = timed(s, y, a.iters)
                    lv = s.lv_state(0)
                    res[f"bayeslv_ncov{ncov}_mode{mode}_ms"] = ms
                    res[f"bayeslv_ncov{ncov}_mode{mode}_over_bayespr"] = ms / res["bayespr_one_region_per_locus_ms"]
                    res[f"bayeslv_ncov{ncov}_mode{mode}_trapped"] = lv["trapped"]
                    s.close()
        owner.close()
        out["shapes"][shape] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
