"""Times the SNP back-solve of GBLUP (ngp_backsolve_*): W = K U (begin) and the column pass, by default at 10,000 animals x 100,000 SNPs
with 1,000 stored draws.  The column pass is timed for uint8 and float32 genotypes (the same arithmetic on four times the staged bytes).
Wall times of whole calls; the kernels' own times come from a kernel trace of this script.  Prints one JSON line.

    python tools/backsolve_time.py [--n 10000] [--p 100000] [--draws 1000]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--p", type=int, default=100000)
    ap.add_argument("--draws", type=int, default=1000)
    a = ap.parse_args()
    from ngp_pkg import load_pkg
    ngp = load_pkg()
    N, P, T = a.n, a.p, a.draws
    rng = np.random.default_rng(1)
    Z = np.asfortranarray(rng.integers(0, 3, size=(N, P), dtype=np.uint8))
    Z[0], Z[1] = 0, 1
    s = ngp.Sampler(device=0, seed=1)
    s.set_records(N)
    s.set_residual_prior(4.0, 0.5)
    t0 = time.perf_counter()
    s.grm_begin(N, 1)
    for c0 in range(0, P, 4096):
        s.grm_columns(Z[:, c0:c0 + 4096])
    s.grm_end(); s.grm_invert()
    t_grm = time.perf_counter() - t0
    s.add_random_set_dense(None, N, df=4.0, scale=0.5, varU0=1.0)
    s.set_y(rng.normal(size=N)); s.set_schedule(2 + T, 2, 1)
    s.enable_backsolve(0, T)
    t0 = time.perf_counter()
    s.run(2 + T)
    t_run = time.perf_counter() - t0
    out = dict(N=N, P=P, draws=T, grm_s=round(t_grm, 3), chain_s=round(t_run, 3))
    t0 = time.perf_counter()
    s._chk(s.L.ngp_backsolve_begin(s.h, C.c_int32(0)))
    out["begin_s"] = time.perf_counter() - t0
    out["begin_tflops"] = 2.0 * N * N * T / out["begin_s"] / 1e12
    s1 = None
    for name, M in (("u8", Z), ("f32", None)):
        if M is None:
            M = np.asfortranarray(Z, dtype=np.float32)
        s._chk(s.L.ngp_backsolve_begin(s.h, C.c_int32(0)))
        t0 = time.perf_counter()
        for c0 in range(0, P, 4096 * 8):
            A = M[:, c0:c0 + 4096 * 8]
            f = getattr(s.L, "ngp_backsolve_columns_" + name)
            s._chk(f(s.h, A.ctypes.data_as(C.c_void_p), C.c_int64(A.shape[1]), C.c_int64(N)))
        dt = time.perf_counter() - t0
        r1, r2, n = np.empty(P), np.empty(P), C.c_int64()
        s._chk(s.L.ngp_backsolve_end(s.h, C.c_int32(0), r1.ctypes.data_as(C.c_void_p), r2.ctypes.data_as(C.c_void_p), C.byref(n)))
        assert s1 is None or np.array_equal(s1, r1)   # the same bits from either input type
        s1 = r1
        out[f"columns_{name}_s"] = dt
        out[f"columns_{name}_tflops"] = 2.0 * N * P * T / dt / 1e12
        out[f"columns_{name}_staged_GBps"] = M.nbytes / dt / 1e9
        del M
    s.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
