"""Times K chains of a BayesRCpi model (3 annotations x 4 classes, the RC configuration of tools/method_time.py) over one copy of the
panel through ngp_run_many -- one fused launch per iteration (k_sweep_multi_rc) where the engine serves it, side by side otherwise:
python tools/rc_chains_time.py N P K [iters]
NGP_TOOL_STORAGE=u8: byte tiles; NGP_TOOL_LAG, NGP_TOOL_SHARDS: lag and max_shards (default: the library's, shards_for_pass(K));
NGP_TOOL_STREAMER: streamer variant (4 / 6: two / three shards per streamer workgroup, one chain); NGP_TOOL_MODE=0: per-block engine."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ngp_pkg import load_pkg
ngp = load_pkg()
N, P, K = (int(a) for a in sys.argv[1:4])
iters = int(sys.argv[4]) if len(sys.argv) > 4 else 10
env = os.environ.get
kw = {}
if env("NGP_TOOL_LAG") or env("NGP_TOOL_MODE"): kw.update(mode=int(env("NGP_TOOL_MODE", "1")), lag=int(env("NGP_TOOL_LAG", "1")))
if env("NGP_TOOL_STREAMER"): kw.update(streamer=int(env("NGP_TOOL_STREAMER")))
chains = []
for c in range(K):
    s = ngp.Sampler(device=0, seed=1001 + c, chain=c, storage=env("NGP_TOOL_STORAGE"), **kw)
    if c == 0:
        if K > 1 or env("NGP_TOOL_SHARDS"): s.set_max_shards(int(env("NGP_TOOL_SHARDS", "0")) or s.shards_for_pass(K))
        s.generate_panel(N, P)
        rng = np.random.default_rng(1); bt = np.zeros(P); idx = rng.choice(P, max(10, P // 100), replace=False); bt[idx] = rng.normal(size=len(idx))
        g = s.xbeta(bt); y = 10 + g + np.random.default_rng(2).normal(size=N) * np.sqrt(g.var())
        v = 0.5 * y.var() / (s.mpm().sum() / N)
        an = (np.random.default_rng(3).random((P, 3)) < 0.4).astype(np.int32); an[np.arange(P), np.random.default_rng(4).integers(0, 3, P)] = 1
    else:
        s.share_panel(chains[0])
    s.add_marker_set_rc(0, P, 4.0, v * 0.5, v, [0.0, 0.01, 0.1, 1.0], [0.95, 0.03, 0.015, 0.005], an, estPi=True)
    s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var())
    chains.append(s)
run = (lambda n: ngp.Sampler.run_many(chains, n)) if K > 1 else (lambda n: chains[0].run(n))
run(3)
t = time.perf_counter(); run(iters); dt = (time.perf_counter() - t) / iters
R, S, nb = chains[0].layout()
nz = np.mean([(s.get_state()["beta"][:P] != 0).mean() for s in chains])
persistent = chains[0].config()[0] == 1
grid = chains[0].census()["grid"] if persistent else 0   # (the per-block engine has no resident grid)
fused = K > 1 and grid > 1 + (S + 31) // 32 + S          # a fused launch holds K samplers and the reducers of K chains
print(f"RC chains={K} {'fused' if fused else ('alone' if K == 1 else 'side by side')} storage={env('NGP_TOOL_STORAGE', 'f32')} N={N} P={P} layout R={R} S={S} "
      f"streamer={chains[0].streamer()[0] if persistent else '-'} config={chains[0].config()} grid={grid}: {dt * 1e3:.3f} ms/pass, {K / dt:.2f} chain-iterations/s, "
      f"{dt / nb * 1e6:.2f} us/block   (non-zero effects {nz * 100:.2f} %)", flush=True)
for s in chains[::-1]: s.close()
