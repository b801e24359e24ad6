"""Device time of ONE step of a hybrid (single-step GBLUP) random-effect set (ngp_hybrid.h) beside the two engines it is made of, on
simulated pedigrees (random_gs_time.pedigree, overlapping generations; A^-1 without inbreeding as there): q animals of which n_g --
drawn from the younger half -- are genotyped and renumbered last.

    hybrid     ngp_add_random_set_hybrid over S = A^-1 (renumbered) and a dense n_g x n_g block D
    csr        ngp_add_random_set over the same S, level-scheduled (as the hybrid set's head is)
    dense      ngp_add_random_set_dense over the same T = D + S_tt
    floor_q, floor_ng   a set over K = I with q / n_g levels: k_head, the level terms, the update and the bookkeeping of an iteration,
                        which every one of the above contains once

A handle without a panel (ngp_set_records), one set, one record per level; ngp_run(1) timed by the library's stream events
(ngp_get_timing), the median of --reps steps after a warm-up, the handles taking turns.  Reported in microseconds per step:
ratio = hybrid / (csr + dense), and ratio_net with the floors taken off both sides (the sum holds two iterations' bookkeeping, the hybrid
step one).  D is a well-conditioned positive definite matrix made here; no time depends on its values.  Every size runs in a child
process of its own under its own time limit.

    python tools/singlestep_time.py [--sizes 100000:5000,20000:2000] [--reps 21] [--out profiles/singlestep_time.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def measure(q, ng, reps):
    import random_gs_time as GS
    from ngp_pkg import load_pkg
    ngp = load_pkg()
    K = GS.ainv_no_inbreeding(*GS.pedigree(q, "overlapping"))
    rng = np.random.default_rng(5)
    gpos = q // 2 + rng.permutation(q - q // 2)[:ng]
    kp, kc, kv = ngp.permute_csr(K, ngp.single_step_order(q, gpos))
    hd = q - ng
    B = rng.normal(size=(ng, 64))
    D = B @ B.T / 64.0 + 0.5 * np.eye(ng)
    D = (D + D.T) / 2.0                                     # (exactly symmetric, as the library requires)
    T = D.copy()
    nnz_th = 0
    for l in range(hd, q):                                  # T = D + S_tt, as the set-up folds it; the rest of a trailing row is S_th
        c, v = kc[kp[l]:kp[l + 1]], kv[kp[l]:kp[l + 1]]
        t = c >= hd
        T[l - hd, c[t] - hd] += v[t]
        nnz_th += int((~t).sum())
    S = (kp, kc, kv)
    hs = {}

    def handle(name, nlev, add):
        s = ngp.Sampler(device=0, seed=3, chain=0)
        s.set_records(nlev)
        rid = add(s, np.arange(nlev, dtype=np.int32))
        s.set_y(np.random.default_rng(3).normal(size=nlev) + 5.0); s.set_residual_prior(4.0, 0.5)
        hs[name] = (s, rid)

    handle("hybrid", q, lambda s, lv: s.add_random_set_hybrid(lv, q, S, ng, D=D, varU0=1.0))
    handle("csr", q, lambda s, lv: s.add_random_set(lv, q, K=S, varU0=1.0))
    handle("dense", ng, lambda s, lv: s.add_random_set_dense(lv, ng, K=T, varU0=1.0))
    handle("floor_q", q, lambda s, lv: s.add_random_set(lv, q, varU0=1.0))
    handle("floor_ng", ng, lambda s, lv: s.add_random_set(lv, ng, varU0=1.0))
    for n in ("hybrid", "csr"):
        hs[n][0].set_random_schedule(hs[n][1], "scheduled")
    info = hs["hybrid"][0].get_random_schedule(hs["hybrid"][1])
    for s, _ in hs.values():
        s.run(2)                                            # warm-up: code objects, first launches
    ts = {n: [] for n in hs}
    for _ in range(reps):                                   # the handles take turns
        for n, (s, _) in hs.items():
            s.get_timing()
            s.run(1)
            ts[n].append(s.get_timing()["iter_ms"] * 1e3)
    finite = bool(np.all(np.isfinite(hs["hybrid"][0].get_random(0)["u"])))
    for s, _ in hs.values():
        s.close()
    us = {n: float(np.median(t)) for n, t in ts.items()}
    res = dict(q=q, n_g=ng, nnz_S=int(kp[-1]), nnz_S_th=nnz_th, head_depths=info["depths"], head_launches=info["launches"],
               block_launches=(ng + 63) // 64, finite=finite, reps=reps)
    for n in hs:
        res[n + "_us"] = us[n]
        res[n + "_us_min"], res[n + "_us_max"] = float(np.min(ts[n])), float(np.max(ts[n]))
    res["sum_us"] = us["csr"] + us["dense"]
    res["ratio"] = us["hybrid"] / res["sum_us"]
    res["ratio_net"] = (us["hybrid"] - us["floor_q"]) / ((us["csr"] - us["floor_q"]) + (us["dense"] - us["floor_ng"]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000:5000,20000:2000", help="q:n_g pairs")
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=240, help="seconds every size may take")
    ap.add_argument("--one", default=None, help="(internal) measure one q:n_g pair in this process")
    a = ap.parse_args()
    if a.one:
        q, ng = (int(x) for x in a.one.split(":"))
        print(json.dumps(measure(q, ng, a.reps)), flush=True)
        return
    rows = []
    for pair in a.sizes.split(","):  # a size that fails or runs out of time ends the tool: nothing more is started on the device
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--one", pair, "--reps", str(a.reps)], timeout=a.timeout, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:
            raise SystemExit(f"size {pair} failed with status {r.returncode}")
        print(r.stdout.strip(), flush=True)
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
