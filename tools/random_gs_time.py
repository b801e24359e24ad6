"""Device time of ONE random step of a pedigree set under each Gauss-Seidel engine (ngp_random.h): serial (k_rand_gs) against
level-scheduled (k_rand_sched_*), on simulated pedigrees of two kinds -- overlapping generations (parents among the 5 F animals in
front, F founders) and discrete generations (generations of F animals, parents in the generation before) -- with F = q / 20.

A handle without a panel (ngp_set_records), one set, one record per animal (the youngest 500,000 animals where q is larger: the handle
takes no more records): ngp_run(1) is then k_head, the random step and the
bookkeeping of an iteration, timed by the library's stream events around it (ngp_get_timing).  After a warm-up the step is repeated and
the median taken; the two engines alternate.  "identity" is the same step over K = I (no Gauss-Seidel launch at all): the floor both
engines sit on.  K is A^-1 by Henderson's rules WITHOUT inbreeding (a = 2 for an animal with parents, 1 for a founder), built here with numpy: the tool times the engine,
whose cost depends on the pattern of K, and Meuwissen and Luo's walk over 10^6 animals of deep random pedigrees takes minutes.

--tuple k times a correlated (Tuple) set of k components instead (ngp_random_tuple.h): (ID, Dam[, Sire, ID]) levels of the same records
over the same K (founders' records have no dam: level -1); there is no "identity" floor then (a tuple set always runs an engine), and
the scalar set's serial / scheduled times of the same pedigree are measured beside it for the ratio.

    python tools/random_gs_time.py [--sizes 1000,20000,100000,1000000] [--reps 21] [--tuple k] [--out profiles/random_gs_time.json]
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ngp_pkg import load_pkg  # noqa: E402


MAX_RECORDS = 500000


def pedigree(q, kind, seed=1):
    """(sire, dam), 0-based, -1 unknown, parents in front of their offspring, the two parents different."""
    rng = np.random.default_rng(seed)
    F = max(q // 20, 4)
    i = np.arange(q)
    if kind == "overlapping":
        lo = np.maximum(i - 5 * F, 0)
        hi = i
    else:
        g = i // F
        lo, hi = (g - 1) * F, g * F
    span = hi - lo
    a = lo + np.floor(rng.random(q) * span).astype(np.int64)
    b = lo + np.floor(rng.random(q) * (span - 1)).astype(np.int64)
    b = np.where(b >= a, b + 1, b)
    s = np.where(i < F, -1, a)
    d = np.where(i < F, -1, b)
    return s, d


def ainv_no_inbreeding(s, d):
    """Henderson's rules with F = 0 as CSR (k_ptr, k_col, k_val), columns ascending."""
    q = len(s)
    i = np.arange(q)
    known = s >= 0
    r = [i, i[known], s[known], i[known], d[known], s[known], s[known], d[known], d[known]]
    c = [i, s[known], i[known], d[known], i[known], s[known], d[known], s[known], d[known]]
    a = np.where(known, 2.0, 1.0)
    ak = a[known]
    v = [a, -ak / 2, -ak / 2, -ak / 2, -ak / 2, ak / 4, ak / 4, ak / 4, ak / 4]
    r, c, v = np.concatenate(r), np.concatenate(c), np.concatenate(v)
    key = r * q + c
    o = np.argsort(key, kind="stable")
    key, v = key[o], v[o]
    first = np.concatenate([[True], key[1:] != key[:-1]])
    idx = np.nonzero(first)[0]
    val = np.add.reduceat(v, idx)
    rows, cols = key[idx] // q, key[idx] % q
    kp = np.zeros(q + 1, dtype=np.int64)
    np.add.at(kp, rows + 1, 1)
    return np.cumsum(kp), cols.astype(np.int32), val


def time_steps(s, reps):
    s.get_timing()
    out = []
    for _ in range(reps):
        s.run(1)
        out.append(s.get_timing()["iter_ms"])
    return out


def measure(ngp, q, kind, reps, tk=0):
    sd = pedigree(q, kind)
    K = ainv_no_inbreeding(*sd)
    rng = np.random.default_rng(3)
    N = min(q, MAX_RECORDS)
    y = rng.normal(size=N) + 5.0
    level = np.arange(q - N, q, dtype=np.int32)
    hs = {}
    names = ("identity", "serial", "scheduled") if not tk else ("serial", "scheduled", "tuple_serial", "tuple_scheduled")
    for name in names:
        s = ngp.Sampler(device=0, seed=3, chain=0)
        s.set_records(N)
        if name.startswith("tuple_"):
            levels = np.stack([level, sd[1][level], sd[0][level], level][:tk]).astype(np.int32)
            rid = s.add_random_set_tuple(levels, q, K=K, varU0=np.eye(tk) + 0.2)
            s.set_random_schedule(rid, name[6:])
        else:
            rid = s.add_random_set(level, q, K=None if name == "identity" else K, varU0=1.0)
            if name != "identity":
                s.set_random_schedule(rid, name)
        s.set_y(y); s.set_residual_prior(4.0, 0.5)
        hs[name] = (s, rid)
    info = hs["scheduled"][0].get_random_schedule(hs["scheduled"][1])
    tinfo = hs["tuple_scheduled"][0].get_random_schedule(hs["tuple_scheduled"][1]) if tk else None
    # the serial walk costs about a microsecond per level: fewer repeats where one step takes a second
    nrep = {n: (max(3, min(reps, int(2e6 / q))) if n.endswith("serial") else reps) for n in hs}
    for n, (s, _) in hs.items():
        s.run(2)                                       # warm-up: code objects, first launches
    same = np.array_equal(hs["serial"][0].get_random(0)["u"], hs["scheduled"][0].get_random(0)["u"])   # the same chain so far, bit for bit
    if tk:
        same = same and np.array_equal(hs["tuple_serial"][0].get_random_tuple(0)["u"], hs["tuple_scheduled"][0].get_random_tuple(0)["u"])
    ts = {n: [] for n in hs}
    for k in range(reps):                              # alternate the engines
        for n, (s, _) in hs.items():
            if k < nrep[n]:
                ts[n] += time_steps(s, 1)
    for s, _ in hs.values():
        s.close()
    res = dict(q=q, records=N, kind=kind, nnz_per_row=float(len(K[1]) / q), depths=info["depths"], launches=info["launches"], same_bits=bool(same))
    if tk:
        res.update(tuple_k=tk, tuple_depths=tinfo["depths"], tuple_launches=tinfo["launches"])
    for n in hs:
        res[n + "_ms_median"] = float(np.median(ts[n]))
        res[n + "_ms_min"] = float(np.min(ts[n]))
        res[n + "_ms_max"] = float(np.max(ts[n]))
        res[n + "_steps"] = len(ts[n])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="1000,20000,100000,1000000")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--tuple", type=int, default=0, dest="tk", help="time a correlated (Tuple) set of k = 2..4 components beside the scalar set")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ngp = load_pkg()
    rows = []
    for q in (int(x) for x in a.sizes.split(",")):
        for kind in ("overlapping", "discrete"):
            r = measure(ngp, q, kind, a.reps, a.tk)
            rows.append(r)
            print(json.dumps(r), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
