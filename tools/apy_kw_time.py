"""Times W = K X of the SNP back-solve (ngp_backsolve_begin) over an APY set (apy_kw: k_apy_kw_tail, k_apy_kw_core) and, with --dense,
over a dense set of the same N (backsolve_kw).  Wall time of the whole call, which ends in a stream synchronise and includes the
allocation of W; the kernels' own times come from a kernel trace of this script in a run of its own.  The
call is repeated behind one warm-up (begin on the open set starts again).  Prints one JSON line.

    python tools/apy_kw_time.py [--n 40000] [--nc 4096] [--p 2048] [--draws 256] [--repeats 5] [--dense]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed_begin(s, repeats):
    ts = []
    for _ in range(repeats + 1):
        t0 = time.perf_counter()
        s._chk(s.L.ngp_backsolve_begin(s.h, C.c_int32(0)))
        ts.append(time.perf_counter() - t0)
    return ts[1:]   # (the first call loads the code objects)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=40000)
    ap.add_argument("--nc", type=int, default=4096)
    ap.add_argument("--p", type=int, default=2048)
    ap.add_argument("--draws", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--dense", action="store_true")
    a = ap.parse_args()
    from ngp_pkg import load_pkg
    ngp = load_pkg()
    N, nc, P, T = a.n, a.nc, a.p, a.draws
    nn = N - nc
    rng = np.random.default_rng(1)
    Z = np.asfortranarray(rng.integers(0, 3, size=(N, P), dtype=np.uint8))
    Z[0], Z[1] = 0, 1
    y = rng.normal(size=N)
    out = dict(N=N, nc=nc, P=P, draws=T)
    for kind in ["apy"] + (["dense"] if a.dense else []):
        s = ngp.Sampler(device=0, seed=1)
        s.set_records(N)
        s.set_residual_prior(4.0, 0.5)
        t0 = time.perf_counter()
        if kind == "apy":
            s.grm_begin_apy(N, nc, 1); s.grm_columns(Z); s.grm_end(); s.grm_apy()
            s.add_random_set_apy(None, N, nc, df=4.0, scale=0.5, varU0=1.0)
        else:
            s.grm_begin(N, 1); s.grm_columns(Z); s.grm_end(); s.grm_invert()
            s.add_random_set_dense(None, N, df=4.0, scale=0.5, varU0=1.0)
        out[kind + "_setup_s"] = round(time.perf_counter() - t0, 3)
        s.set_y(y); s.set_schedule(2 + T, 2, 1); s.enable_backsolve(0, T)
        t0 = time.perf_counter()
        s.run(2 + T)
        out[kind + "_chain_s"] = round(time.perf_counter() - t0, 3)
        ts = timed_begin(s, a.repeats)
        best = min(ts)
        # fp64 work from the shapes: two passes over P and one over Kc0 per draw (APY), one over K (dense); P's bytes once per 64-draw
        # group by each of the two kernels
        flop = (4.0 * nn * nc + 2.0 * nc * nc) * T if kind == "apy" else 2.0 * N * N * T
        out[kind + "_begin_s"] = [round(t, 6) for t in ts]
        out[kind + "_tflops_over_wall"] = round(flop / best / 1e12, 3)
        if kind == "apy":
            out["apy_P_GBps_over_wall"] = round(2.0 * ((T + 63) // 64) * nn * nc * 8.0 / best / 1e9, 1)
        s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
