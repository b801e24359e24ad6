"""Times the genomic-variance pass (k_genvar and its small kernels, ngp_genvar.h) behind the sweep:
python tools/genvar_time.py N P W K [iters]
A BayesPR model of three marker sets on a generated N x P panel with every iteration kept is run `iters` iterations without and then
with the pass over windows of W SNPs (W = 0: set and total slots only); the difference of the device time per iteration
(ngp_get_timing) is the pass.  K > 1: K chains that share the panel through ngp_run_many -- ONE pass serves them where the sweeps
fuse.  Bytes of a pass are 4 N P (fp32 tiles) or N P (NGP_TOOL_STORAGE=u8); the rate is printed as a fraction of 8 TB/s.  The
yardstick is the prediction pass over a prediction panel of the same rows, columns and storage in the same process (NGP_TOOL_YARD=0
skips it).  NGP_TOOL_SHARDS, NGP_TOOL_LAG as in tools/predict_time.py.  The last line gives the fixed-point accuracy of the last
draw: V_g and the smallest window's V against the Float64 variance of ngp_xbeta's row sums (NGP_TOOL_ACCURACY=0 skips it).
NGP_TOOL_THIN=T keeps every T-th iteration instead of every one: the chain cost of the pass at that thinning."""
import os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ngp_pkg import load_pkg
ngp = load_pkg()
N, P, W, K = (int(a) for a in sys.argv[1:5])
iters = int(sys.argv[5]) if len(sys.argv) > 5 else 20
env = os.environ.get
storage = env("NGP_TOOL_STORAGE")
kw = dict(mode=1, lag=int(env("NGP_TOOL_LAG"))) if env("NGP_TOOL_LAG") else {}
cuts = [0, P // 3 // 64 * 64, 2 * P // 3 // 64 * 64, P]
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
    for a, b in zip(cuts[:-1], cuts[1:]):
        s.add_marker_set(a, b - a, 0, 4.0, v * 0.5, [(0, b - a)], [v])
    s.set_y(y + 0.01 * c); s.set_residual_prior(4.0, 0.25 * y.var()); s.set_schedule(10 ** 9, 0, int(env("NGP_TOOL_THIN", "1")))   # every iteration is kept (or every T-th)
    chains.append(s)
run = (lambda n: ngp.Sampler.run_many(chains, n)) if K > 1 else (lambda n: chains[0].run(n))


def ms_per_iteration():
    run(3)
    chains[0].get_timing()
    run(iters)
    t = chains[0].get_timing()
    return t["iter_ms"] / t["iters"]


base = ms_per_iteration()
for s in chains:
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        if W > 0:
            s.set_variance_windows(k, [(j, min(j + W, b - a)) for j in range(0, b - a, W)])
    s.enable_genomic_variance(True, 0.01, 0)
with_gv = ms_per_iteration()
launches, served = chains[0].genomic_variance_stats()
fused = K > 1 and served == K * launches
ms = with_gv - base
nbytes = (1 if storage == "u8" else 4) * N * P
R, S, _ = chains[0].layout()
nslots, nwin = chains[0].genomic_variance_layout()[:2]
print(f"genvar storage={storage or 'f32'} {N}x{P} (R={R} S={S}) windows of {W}: {nwin} windows, {nslots} slots, chains={K} "
      f"{'one pass for all' if fused else ('alone' if K == 1 else 'a pass per chain')}: iteration {base:.3f} -> {with_gv:.3f} ms, pass {ms:.3f} ms, "
      f"{nbytes / 1e9:.2f} GB -> {nbytes / ms / 1e9:.2f} TB/s = {nbytes / ms / 1e9 / 8 * 100:.1f} % of 8 TB/s; per chain {ms / K:.3f} ms", flush=True)
for s in chains:
    s.enable_genomic_variance(False)
if env("NGP_TOOL_YARD", "1") == "1":   # the prediction pass over the same rows, columns and storage
    cc = max(64, min(P, (256 << 20) // N) // 64 * 64)
    codes = np.asfortranarray(np.random.default_rng(5).integers(0, 3, size=(N, cc)).astype(np.uint8))
    chains[0].begin_prediction_panel(N)
    for c0 in range(0, P, cc):
        chains[0].prediction_columns(c0, codes[:, :min(cc, P - c0)], centre=True)
    chains[0].end_prediction_panel()
    yard = ms_per_iteration() - base
    print(f"yardstick k_predict over {N}x{P} candidates, chains={K}: pass {yard:.3f} ms, {nbytes / yard / 1e9:.2f} TB/s; genvar / predict = {ms / yard:.2f} "
          f"(target <= 1.25)", flush=True)
if env("NGP_TOOL_ACCURACY", "1") == "1":
    s = chains[0]
    s.enable_genomic_variance(True, 0.01, 0)
    for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        if W > 0:
            s.set_variance_windows(k, [(j, min(j + W, b - a)) for j in range(0, b - a, W)])
    run(1)
    last = s.genomic_variance_last()
    beta = s.get_state()["beta"]
    vg = s.xbeta(beta).var(ddof=1)
    line = f"accuracy: V_g device {last[-1]:.17g} float64 {vg:.17g} relative difference {abs(last[-1] - vg) / vg:.3e}"
    if W > 0:
        n0 = -(-cuts[1] // W)                                    # the windows of set 0 are slots 0 .. n0 - 1, window k on columns k W ..
        k = int(np.argmin(np.where(last[:n0] > 0, last[:n0], np.inf)))
        bw = np.zeros(P)
        bw[k * W:min(k * W + W, cuts[1])] = beta[k * W:min(k * W + W, cuts[1])]
        vw = s.xbeta(bw).var(ddof=1)
        line += f"; smallest window of set 0 (slot {k}) device {last[k]:.17g} float64 {vw:.17g} relative difference {abs(last[k] - vw) / vw:.3e}"
    print(line, flush=True)
for s in chains[::-1]: s.close()
