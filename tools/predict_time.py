"""Times the prediction pass (k_predict + k_predict_combine, ngp_predict.h) behind the sweep:
python tools/predict_time.py N P Np K [iters]
A BayesPR model on a generated N x P panel with every iteration kept is run `iters` iterations without and then with a prediction panel
of Np x P random allele counts; the difference of the device time per iteration (ngp_get_timing) is the pass.  K > 1: K chains that
share the panel through ngp_run_many -- ONE pass serves them where the sweeps fuse.  Bytes of a pass are 4 Np P (fp32 tiles) or Np P
(NGP_TOOL_STORAGE=u8); the rate is printed as a fraction of 8 TB/s.  The "before" is ngp_xbeta (k_xbeta / k_xbeta8: one thread per
row, strided reads) on a generated Np x P training panel, wall time of the call less its copies' share being small at these sizes.
NGP_TOOL_SHARDS, NGP_TOOL_LAG as in tools/rc_chains_time.py."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ngp_pkg import load_pkg
ngp = load_pkg()
N, P, Np, K = (int(a) for a in sys.argv[1:5])
iters = int(sys.argv[5]) if len(sys.argv) > 5 else 20
env = os.environ.get
storage = env("NGP_TOOL_STORAGE")
kw = dict(mode=1, lag=int(env("NGP_TOOL_LAG"))) if env("NGP_TOOL_LAG") else {}
chains = []
for c in range(K):
    s = ngp.Sampler(device=0, seed=1001 + c, chain=c, storage=storage, **kw)
    if c == 0:
        if K > 1 or env("NGP_TOOL_SHARDS"): s.set_max_shards(int(env("NGP_TOOL_SHARDS", "0")) or s.shards_for_pass(K))
        s.generate_panel(N, P)
        rng = np.random.default_rng(1); bt = np.zeros(P); idx = rng.choice(P, max(10, P // 100), replace=False); bt[idx] = rng.normal(size=len(idx))
        g = s.xbeta(bt); y = 10 + g + np.random.default_rng(2).normal(size=N) * np.sqrt(g.var())
        v = 0.5 * y.var() / (s.mpm().sum() / N)
    else:
        s.share_panel(chains[0])
    s.add_marker_set(0, P, 0, 4.0, v * 0.5, [(0, P)], [v])
    s.set_y(y + 0.01 * c); s.set_residual_prior(4.0, 0.25 * y.var()); s.set_schedule(10 ** 9, 0, 1)   # every iteration is kept
    chains.append(s)
run = (lambda n: ngp.Sampler.run_many(chains, n)) if K > 1 else (lambda n: chains[0].run(n))


def ms_per_iteration():
    run(3)
    chains[0].get_timing()
    run(iters)
    t = chains[0].get_timing()
    return t["iter_ms"] / t["iters"]


base = ms_per_iteration()
cc = max(64, min(P, (256 << 20) // Np) // 64 * 64)              # one chunk of random codes serves every column range
codes = np.asfortranarray(np.random.default_rng(5).integers(0, 3, size=(Np, cc)).astype(np.uint8))
t0 = time.perf_counter()
chains[0].begin_prediction_panel(Np)
for c0 in range(0, P, cc):
    chains[0].prediction_columns(c0, codes[:, :min(cc, P - c0)], centre=True)
chains[0].end_prediction_panel()
upload = time.perf_counter() - t0
with_pred = ms_per_iteration()
launches, served = chains[0].prediction_stats()
fused = K > 1 and served == K * launches
ms = with_pred - base
nbytes = (1 if storage == "u8" else 4) * Np * P
lay = chains[0].prediction_layout()
print(f"predict storage={storage or 'f32'} train {N}x{P} (R={chains[0].layout()[0]} S={chains[0].layout()[1]}) candidates Np={Np} (R={lay[1]} S={lay[2]}) chains={K} "
      f"{'one pass for all' if fused else ('alone' if K == 1 else 'a pass per chain')}: iteration {base:.3f} -> {with_pred:.3f} ms, pass {ms:.3f} ms, "
      f"{nbytes / 1e9:.2f} GB -> {nbytes / ms / 1e9:.2f} TB/s = {nbytes / ms / 1e9 / 8 * 100:.1f} % of 8 TB/s; per chain {ms / K:.3f} ms; upload {upload:.2f} s", flush=True)
for s in chains[::-1]: s.close()
if env("NGP_TOOL_BEFORE", "1") == "1":   # the utility kernel on a training panel of the same Np x P
    b = ngp.Sampler(device=0, seed=1, chain=0, storage=storage)
    b.generate_panel(Np, P)
    bt = np.random.default_rng(6).normal(size=P)
    b.xbeta(bt)
    t0 = time.perf_counter(); b.xbeta(bt); dt = (time.perf_counter() - t0) * 1e3
    print(f"before  storage={storage or 'f32'} ngp_xbeta on a {Np}x{P} training panel (R={b.layout()[0]} S={b.layout()[1]}): {dt:.3f} ms per call (host copies of beta and "
          f"the result included), {nbytes / dt / 1e9:.2f} TB/s = {nbytes / dt / 1e9 / 8 * 100:.1f} % of 8 TB/s", flush=True)
    b.close()
