"""Times the hold-out step (k_holdout_augment + k_holdout_accum, ngp_holdout.h) around the sweep:
python tools/holdout_time.py N P FRACTION K [iters]
A BayesPR model on a generated N x P panel with every iteration kept.  One chain is run `iters` iterations without a mask and then with
FRACTION of its rows held out (every 1/FRACTION-th row); the difference of the device time per iteration (ngp_get_timing) is the step.
K > 1: K fold-chains that share the panel through ngp_run_many, chain c holding out fold c of K (deal_folds), against the same K chains
without masks; the aggregate rate is K iterations per pass.  NGP_TOOL_SHARDS, NGP_TOOL_LAG as in tools/rc_chains_time.py.
NGP_TOOL_UNMASKED_ONLY=1 times the unmasked configurations alone and touches no hold-out entry point; with NGP_TOOL_ROOT=<a built
checkout of an earlier commit> the package is loaded from there, which gives the time before."""
import os, sys
import numpy as np
sys.path.insert(0, os.environ.get("NGP_TOOL_ROOT") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ngp_pkg import load_pkg
ngp = load_pkg()
N, P = int(sys.argv[1]), int(sys.argv[2])
frac, K = float(sys.argv[3]), int(sys.argv[4])
iters = int(sys.argv[5]) if len(sys.argv) > 5 else 50
env = os.environ.get
kw = dict(mode=1, lag=int(env("NGP_TOOL_LAG"))) if env("NGP_TOOL_LAG") else {}
unmasked_only = env("NGP_TOOL_UNMASKED_ONLY") == "1"


def build(K, masks):
    chains = []
    for c in range(K):
        s = ngp.Sampler(device=0, seed=1001, chain=c, **kw)
        if c == 0:
            if K > 1 or env("NGP_TOOL_SHARDS"): s.set_max_shards(int(env("NGP_TOOL_SHARDS", "0")) or s.shards_for_pass(K))
            s.generate_panel(N, P)
            rng = np.random.default_rng(1); bt = np.zeros(P); idx = rng.choice(P, max(10, P // 100), replace=False); bt[idx] = rng.normal(size=len(idx))
            g = s.xbeta(bt); build.y = 10 + g + np.random.default_rng(2).normal(size=N) * np.sqrt(g.var())
            build.v = 0.5 * build.y.var() / (s.mpm().sum() / N)
        else:
            s.share_panel(chains[0])
        s.add_marker_set(0, P, 0, 4.0, build.v * 0.5, [(0, P)], [build.v])
        if masks is not None:
            s.set_holdout(masks[c])
        s.set_y(build.y); s.set_residual_prior(4.0, 0.25 * build.y.var()); s.set_schedule(10 ** 9, 0, 1)   # every iteration is kept
        chains.append(s)
    return chains


def ms_per_iteration(chains):
    run = (lambda n: ngp.Sampler.run_many(chains, n)) if len(chains) > 1 else (lambda n: chains[0].run(n))
    run(5)
    chains[0].get_timing()
    l0 = chains[0].get_timing()["sweep_launches"]
    run(iters)
    t = chains[0].get_timing()
    fused = len(chains) > 1 and t["sweep_launches"] - l0 == iters
    ms = t["iter_ms"] / t["iters"]
    lay = chains[0].layout()
    for s in chains[::-1]: s.close()
    return ms, fused, lay


step = max(2, int(round(1.0 / frac)))
one_mask = [np.arange(0, N, step, dtype=np.int64)]
base, _, lay = ms_per_iteration(build(1, None))
line = f"holdout {N}x{P} (R={lay[0]} S={lay[1]}) one chain: unmasked {base:.4f} ms / iteration ({1e3 / base:.1f} it/s)"
if not unmasked_only:
    held, _, _ = ms_per_iteration(build(1, one_mask))
    line += f"; {len(one_mask[0])} of {N} rows held out {held:.4f} ms ({1e3 / held:.1f} it/s): the step costs {1e3 * (held - base):.1f} us"
print(line, flush=True)
if K > 1:
    plain, fused0, lay = ms_per_iteration(build(K, None))
    line = (f"holdout {N}x{P} (R={lay[0]} S={lay[1]}) {K} chains, {'one fused pass' if fused0 else 'NOT fused'}: unmasked {plain:.4f} ms / pass "
            f"({K * 1e3 / plain:.1f} it/s aggregate)")
    if not unmasked_only:
        fold = ngp.deal_folds(np.zeros(N), K, foldSeed=1)
        folds, fused1, _ = ms_per_iteration(build(K, [np.flatnonzero(fold == c) for c in range(K)]))
        line += (f"; {K} folds, {'one fused pass' if fused1 else 'NOT fused'}: {folds:.4f} ms / pass ({K * 1e3 / folds:.1f} it/s aggregate), "
                 f"{K * base / folds:.2f} x the rate of the folds one after another")
    print(line, flush=True)
