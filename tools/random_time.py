"""Device time of the random-effect step (ngp_random.h) at N = 50,000: an identity set with q = 1,000 and a pedigree-like sparse K with
q = 50,000 and about 7 entries per row.  Times ngp_run of a small model with and without the set (same panel, same marker set) and
reports the difference per iteration, plus ngp_sample_random_set's wall time (which adds two PCIe copies of ycorr).

    python tools/random_time.py [--iters 50]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ngp_pkg import load_pkg  # noqa: E402


def ped_csr(q, seed=1):
    """A^-1 of a random pedigree (parents drawn among earlier animals, ~7 entries per row), as CSR."""
    rng = np.random.default_rng(seed)
    rows = [dict() for _ in range(q)]
    for i in range(q):
        if i >= 100:
            s_, d_ = rng.choice(i, 2, replace=False)
            idx, w = [i, int(s_), int(d_)], [1.0, -0.5, -0.5]
            c = 2.0
        else:
            idx, w, c = [i], [1.0], 1.0
        for a, wa in zip(idx, w):
            for b, wb in zip(idx, w):
                rows[a][b] = rows[a].get(b, 0.0) + c * wa * wb
    kp = np.zeros(q + 1, dtype=np.int64)
    kc, kv = [], []
    for l in range(q):
        cols = sorted(rows[l])
        kc += cols; kv += [rows[l][c] for c in cols]
        kp[l + 1] = len(kc)
    return kp, np.array(kc, dtype=np.int32), np.array(kv)


def run(ngp, N, P, iters, rnd):
    s = ngp.Sampler(device=0, seed=3, chain=0)
    s.generate_panel(N, P)
    s.add_marker_set(0, P, 0, 4.0, 0.001, [(0, P)], [0.002])
    if rnd is not None:
        level, q, K = rnd
        s.add_random_set(level, q, K=K, varU0=1.0)
    rng = np.random.default_rng(1)
    s.set_y(rng.normal(size=N) + 5.0)
    s.set_residual_prior(4.0, 0.5)
    s.run(5)
    s.get_timing()
    s.run(iters)
    t = s.get_timing()
    ms = t["iter_ms"] / max(t["iters"], 1)
    fine = None
    if rnd is not None:
        yc = rng.normal(size=N); u = np.zeros(rnd[1])
        s.sample_random_set(0, 1.0, yc, u, 1.0)
        t0 = time.perf_counter()
        for _ in range(5):
            s.sample_random_set(0, 1.0, yc, u, 1.0)
        fine = (time.perf_counter() - t0) / 5 * 1e3
    s.close()
    return ms, fine


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--N", type=int, default=50000)
    ap.add_argument("--P", type=int, default=2048)
    a = ap.parse_args()
    ngp = load_pkg()
    N = a.N
    rng = np.random.default_rng(7)
    base, _ = run(ngp, N, a.P, a.iters, None)
    out = dict(N=N, P=a.P, base_ms_per_iter=base)
    ident, fine_i = run(ngp, N, a.P, a.iters, (rng.integers(0, 1000, size=N).astype(np.int32), 1000, None))
    out.update(identity_q1000_us=(ident - base) * 1e3, identity_fine_seam_ms=fine_i)
    K = ped_csr(N)
    out["ped_nnz_per_row"] = float(len(K[1]) / N)
    ped, fine_p = run(ngp, N, a.P, max(a.iters // 5, 5), (np.arange(N, dtype=np.int32), N, K))
    out.update(pedigree_q50000_ms=ped - base, pedigree_fine_seam_ms=fine_p)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
