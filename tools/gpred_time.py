"""One measured GBLUP prediction: python tools/gpred_time.py N P Nc T out.json -- N records x P SNPs (uniform codes 0/1/2, one byte
each), Nc candidates, T stored draws of a records-only GBLUP chain (burn 2).  Wall times of the phases (each ends in a device
synchronise inside the library) and the column pass's rate from its operation count 2 Nc N P; kernel times come from the same script
under rocprofv3 --kernel-trace --stats, in a run of its own."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ngp_pkg import load_pkg  # noqa: E402

N, P, Nc, T = (int(a) for a in sys.argv[1:5])
out = sys.argv[5]
ngp = load_pkg()
rng = np.random.default_rng(1)
Z = rng.integers(0, 3, size=(P, N), dtype=np.uint8).T
Zc = rng.integers(0, 3, size=(P, Nc), dtype=np.uint8).T
y = rng.normal(size=N) + 0.3 * (Z[:, 0].astype(np.float64) - 1.0)
t = {}
s = ngp.Sampler(device=0, seed=5)
s.set_records(N); s.set_residual_prior(4.0, 0.5)
t0 = time.perf_counter()
s.grm_begin(N, 1)
for c0 in range(0, P, 4096):
    s.grm_columns(Z[:, c0:c0 + 4096])
s.grm_end()
t["grm_build_s"] = time.perf_counter() - t0
t0 = time.perf_counter(); s.grm_invert(); t["grm_invert_s"] = time.perf_counter() - t0
s.add_random_set_dense(None, N, df=4.0, scale=0.5, varU0=1.0)
s.set_y(y); s.set_schedule(2 + T, 2, 1); s.enable_backsolve(0, T)
t0 = time.perf_counter(); s.run(2 + T); t["chain_s"] = time.perf_counter() - t0
print("chain done", t, flush=True)
s.gblup_predict(0, Z, Zc[:64])   # warm-up: code objects, staging
p8 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))
pd = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
t0 = time.perf_counter()
s._chk(s.L.ngp_gpred_begin(s.h, C.c_int32(0), C.c_int64(Nc)))
t["begin_s"] = time.perf_counter() - t0
t0 = time.perf_counter()
for c0 in range(0, P, 4096):
    A, B = Z[:, c0:c0 + 4096], Zc[:, c0:c0 + 4096]
    s._chk(s.L.ngp_gpred_columns_u8(s.h, p8(A), C.c_int64(N), p8(B), C.c_int64(Nc), C.c_int64(A.shape[1])))
t["column_pass_s"] = time.perf_counter() - t0
s1, s2, sc, gcc, n = np.empty(Nc), np.empty(Nc), np.empty(Nc), np.empty(Nc), C.c_int64()
t0 = time.perf_counter()
s._chk(s.L.ngp_gpred_end(s.h, C.c_int32(0), pd(s1), pd(s2), pd(sc), pd(gcc), C.byref(n)))
t["end_s"] = time.perf_counter() - t0
t["column_pass_tflops_wall"] = 2.0 * Nc * N * P / t["column_pass_s"] / 1e12
res = dict(N=N, P=P, Nc=Nc, T=int(n.value), **t, s_mean=float(sc.mean()), gcc_mean=float(gcc.mean()), sum_abs_mean=float(np.abs(s1).mean()),
           finite=bool(np.isfinite(s1).all() and np.isfinite(s2).all() and np.isfinite(sc).all()))
print(json.dumps(res), flush=True)
with open(out, "w") as f:
    json.dump(res, f, indent=1)
s.close()
