"""Timing of the GBLUP path on one device: seconds for G (and TFLOP/s = 2 N^2 P / time, counted as the full product), seconds for the
inverse, milliseconds per iteration of a model made of the dense set alone (a handle without genotype panel) and that time as a
multiple of 8 q^2 bytes / 8 TB/s, and the same model through the CSR engine (ngp_add_random_set with the dense array) at a q where
that is bearable (q <= 2,048).  Every GPU step is a child process of its own under its own time limit.

    python tools/gblup_time.py --N 10000 --P 100000 [--method 1] [--iters 50] [--csr-q 2048] [--csr-iters 3]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_BYTES_PER_S = 8.0e12


def genotypes(N, P, seed=7, chunk=4096):
    """Allele counts 0 / 1 / 2, uint8, Fortran order, drawn uniformly in column chunks (no timing here depends on the values; a billion
    binomial draws would cost more host time than everything that is measured)."""
    rng = np.random.default_rng(seed)
    M = np.empty((N, P), dtype=np.uint8, order="F")
    for c0 in range(0, P, chunk):
        n = min(chunk, P - c0)
        M[:, c0:c0 + n] = rng.integers(0, 3, size=(n, N), dtype=np.uint8).T
    return M


def build_K(s, N, P, method):
    M = genotypes(N, P)
    t0 = time.perf_counter()
    s.grm_begin(N, method)
    for c0 in range(0, P, 4096):
        s.grm_columns(M[:, c0:c0 + 4096])
    s.grm_end()
    t_g = time.perf_counter() - t0
    t0 = time.perf_counter()
    s.grm_invert()
    return t_g, time.perf_counter() - t0


def time_run(s, N, iters):
    rng = np.random.default_rng(1)
    s.set_y(rng.normal(size=N) * 2.0 + 5.0)
    s.set_residual_prior(4.0, 0.5)
    s.run(2)
    s.get_timing()
    s.run(iters)
    t = s.get_timing()
    return t["iter_ms"] / max(t["iters"], 1)


def step_dense(a):
    from ngp_pkg import load_pkg
    ngp = load_pkg()
    s = ngp.Sampler(device=0, seed=3, chain=0)
    t_g, t_inv = build_K(s, a.N, a.P, a.method)
    s.set_records(a.N)
    s.add_random_set_dense(None, a.N, varU0=1.0)
    ms = time_run(s, a.N, a.iters)
    floor_ms = 8.0 * a.N * a.N / HBM_BYTES_PER_S * 1e3
    print(json.dumps(dict(step="dense", N=a.N, P=a.P, method=a.method, grm_s=t_g, grm_tflops=2.0 * a.N * a.N * a.P / t_g / 1e12, inverse_s=t_inv,
                          dense_ms_per_iter=ms, hbm_floor_ms=floor_ms, times_hbm_floor=ms / floor_ms, launches_per_iter=(a.N + 63) // 64 + 4)))
    s.close()


def step_csr(a):
    from ngp_pkg import load_pkg
    ngp = load_pkg()
    q = a.csr_q
    s = ngp.Sampler(device=0, seed=3, chain=0)
    build_K(s, q, a.csr_P, a.method)
    K = s.grm_get()
    out = {}
    for engine in ("dense", "csr"):
        c = ngp.Sampler(device=0, seed=3, chain=0)
        c.set_records(q)
        if engine == "dense":
            c.add_random_set_dense(None, q, K=K, varU0=1.0)
        else:
            c.add_random_set(np.arange(q, dtype=np.int32), q, K=K, varU0=1.0)
        out[engine + "_ms_per_iter"] = time_run(c, q, a.iters if engine == "dense" else a.csr_iters)
        c.close()
    out.update(step="csr_vs_dense", q=q, speedup=out["csr_ms_per_iter"] / out["dense_ms_per_iter"])
    print(json.dumps(out))
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=10000)
    ap.add_argument("--P", type=int, default=100000)
    ap.add_argument("--method", type=int, default=1)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--csr-q", type=int, default=2048)
    ap.add_argument("--csr-P", type=int, default=8192)
    ap.add_argument("--csr-iters", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=420, help="seconds every GPU step may take")
    ap.add_argument("--step", choices=["dense", "csr"], help="(internal) run one step in this process")
    a = ap.parse_args()
    if a.step:
        return {"dense": step_dense, "csr": step_csr}[a.step](a)
    if a.csr_q > 2048:
        raise SystemExit("--csr-q: the one-lane CSR engine is not bearable above q = 2,048")
    steps = ["dense"] + (["csr"] if a.csr_q > 0 else [])
    for st in steps:  # a step that fails or runs out of time ends the tool: nothing more is started on the device
        cmd = [sys.executable, os.path.abspath(__file__), "--step", st] + sys.argv[1:]
        r = subprocess.run(cmd, timeout=a.timeout)
        if r.returncode != 0:
            raise SystemExit(f"step {st} failed with status {r.returncode}")


if __name__ == "__main__":
    main()
