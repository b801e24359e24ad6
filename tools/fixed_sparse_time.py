"""Device time of ONE iteration with a fixed-effect set given as a sparse matrix (ngp_add_fixed_set_sparse; csrc/ngp_fixed_sparse.h).

A handle without a panel (ngp_set_records) with one (1|g) set of 50 levels; ngp_run(1) is then k_head, the fixed step, the random step and
the bookkeeping of an iteration, timed by the library's stream events around it (ngp_get_timing).  After a warm-up the iteration is
repeated and the median taken; the handles of one size alternate.  "floor" is the same handle without the fixed set: what the step
sits on.  Swept: the number of records, and a factor of 100, 5,000 and 100,000 levels (where the records allow a record per level), and a
block of two crossed factors (5,000 x 20 levels) with a covariate.  For context: the dense set (k_fixed) at 64 columns and 50,000 records
against the same design sparse, and whether the two are the same chain bit for bit.

    python tools/fixed_sparse_time.py [--records 50000,500000] [--reps 21] [--out profiles/fixed_sparse_time.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ngp_pkg import load_pkg  # noqa: E402


def factor(N, nlev, seed):
    """Codes -1 .. nlev - 2 (-1 the base level), every level with a record."""
    rng = np.random.default_rng(seed)
    code = np.concatenate([np.arange(nlev), rng.integers(0, nlev, size=N - nlev)]) - 1
    return code[rng.permutation(N)]


def handle(ngp, N, y, add=None):
    s = ngp.Sampler(device=0, seed=3, chain=0)
    s.set_records(N)
    if add is not None:
        add(s)
    s.add_random_set(np.random.default_rng(5).integers(0, 50, size=N), 50, varU0=1.0)
    s.set_y(y); s.set_residual_prior(4.0, 0.5)
    return s


def time_handles(hs, reps):
    for s in hs.values():
        s.run(2)                                       # warm-up: code objects, first launches
        s.get_timing()
    ts = {n: [] for n in hs}
    for _ in range(reps):                              # alternate the handles
        for n, s in hs.items():
            s.run(1)
            ts[n].append(s.get_timing()["iter_ms"])
    return {n: dict(ms_median=float(np.median(t)), ms_min=float(np.min(t)), ms_max=float(np.max(t))) for n, t in ts.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--records", default="50000,500000")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ngp = load_pkg()
    rows = []
    for N in (int(x) for x in a.records.split(",")):
        y = np.random.default_rng(1).normal(size=N) + 5.0
        designs = {f"factor{q}": ([factor(N, q, 2)], None) for q in (100, 5000, 100000) if q <= N}
        designs["crossed5000x20+cov"] = ([factor(N, 5000, 3), factor(N, 20, 4)], np.random.default_rng(6).normal(size=N))
        hs = {"floor": handle(ngp, N, y)}
        info = {}
        for name, (codes, cov) in designs.items():
            csc = ngp.factors_csc(codes, cov)
            info[name] = dict(ncol=int(csc[1]), nnz=int(len(csc[3])))
            hs[name] = handle(ngp, N, y, lambda s, c=csc: s.add_fixed_set_sparse(*c))
        t = time_handles(hs, a.reps)
        for name, s in hs.items():
            r = dict(records=N, design=name, **info.get(name, {}), **t[name])
            if name != "floor":
                r["step_ms_over_floor"] = r["ms_median"] - t["floor"]["ms_median"]
            rows.append(r)
            print(json.dumps(r), flush=True)
            s.close()
    # context: the dense set at 64 columns, 50,000 records, against the same design sparse
    N = 50000
    y = np.random.default_rng(1).normal(size=N) + 5.0
    code = factor(N, 65, 7)
    Xd = np.asfortranarray((code[:, None] == np.arange(64)[None, :]).astype(np.float64))
    hs = {"floor": handle(ngp, N, y), "dense64": handle(ngp, N, y, lambda s: s.add_fixed_set(Xd)),
          "sparse64": handle(ngp, N, y, lambda s: s.add_fixed_factors([code]))}
    t = time_handles(hs, a.reps)
    same = bool(np.array_equal(hs["dense64"].get_fixed()["b"], hs["sparse64"].get_fixed()["b"]) and
                np.array_equal(hs["dense64"].get_state()["ycorr"], hs["sparse64"].get_state()["ycorr"]))
    for name in ("floor", "dense64", "sparse64"):
        r = dict(records=N, design=name, context=True, same_bits=same, **t[name])
        if name != "floor":
            r["step_ms_over_floor"] = r["ms_median"] - t["floor"]["ms_median"]
        rows.append(r)
        print(json.dumps(r), flush=True)
        hs[name].close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
