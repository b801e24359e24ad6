"""Times the convergence diagnostics (k_diag_gather + k_diag_update and k_diag_finalise, ngp_diag.h) behind the sweep:
python tools/diag_time.py N P LAGS[,LAGS...] [iters] [reps]
A BayesPR model of three marker sets on a generated N x P panel.  (0) Device events around 20 full-window updates (k_diag_gather +
k_diag_update at draw indices >= LAGS) and around 20 finalise kernels (ngp_debug_time_diagnostics): time per launch.  Bytes of an
update are (24 LAGS + 48) D from the shapes (per lag one row of ring and of C read and C written; x, x1, S1, S2, head, ring beside
them); the rate is printed beside the measured-copy bandwidth, 6.29 TB/s (SURVEY.md section 8 d).  (1) Every iteration kept (thin 1):
`iters` iterations without and with the diagnostics, alternating `reps` times in this one process; every "on" run starts behind LAGS
draws, so each of its updates runs over the full window.  The difference of the device time per iteration (the events of
ngp_get_timing around the run) is the cost per iteration, the spread of the "off" runs says what a difference means.  (2) thin 10, the
headline's schedule: it/s off and on, alternating the same way, full windows again.  (3) the whole ngp_get_diagnostics call under a
host clock (it ends in a device synchronise): the kernel, the allocation of its output and the nine D-vector copies to the host.  NGP_TOOL_SHARDS, NGP_TOOL_LAG as in
tools/predict_time.py."""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ngp_pkg import load_pkg
ngp = load_pkg()
N, P = (int(a) for a in sys.argv[1:3])
LAGS_LIST = [int(a) for a in sys.argv[3].split(",")]
LAGS = LAGS_LIST[0]
iters = int(sys.argv[4]) if len(sys.argv) > 4 else 40
reps = int(sys.argv[5]) if len(sys.argv) > 5 else 3
env = os.environ.get
COPY_TBS = 6.29
kw = dict(mode=1, lag=int(env("NGP_TOOL_LAG"))) if env("NGP_TOOL_LAG") else {}
cuts = [0, P // 3 // 64 * 64, 2 * P // 3 // 64 * 64, P]
s = ngp.Sampler(device=0, seed=1001, chain=0, **kw)
if env("NGP_TOOL_SHARDS"): s.set_max_shards(int(env("NGP_TOOL_SHARDS")))
s.generate_panel(N, P)
rng = np.random.default_rng(1); bt = np.zeros(P); idx = rng.choice(P, max(10, P // 100), replace=False); bt[idx] = rng.normal(size=len(idx))
g = s.xbeta(bt); y = 10 + g + np.random.default_rng(2).normal(size=N) * np.sqrt(g.var())
v = 0.5 * y.var() / (s.mpm().sum() / N)
for a, b in zip(cuts[:-1], cuts[1:]):
    s.add_marker_set(a, b - a, 0, 4.0, v * 0.5, [(0, b - a)], [v])
s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var())


def ms_per_iteration(n):
    s.get_timing()
    s.run(n)
    t = s.get_timing()
    return t["iter_ms"] / t["iters"]


def alternate(thin):
    """reps x (off, on) runs of `iters` iterations each; the diagnostics keep their state between the "on" runs."""
    s.set_schedule(10 ** 9, 0, thin)
    s.enable_diagnostics(False)
    s.run(max(3, thin))                                        # warm-up
    off, on = [], []
    for r in range(reps):
        s.enable_diagnostics(False)
        off.append(ms_per_iteration(iters))
        s.enable_diagnostics(True, LAGS, 0)
        s.run(thin * max(2, LAGS))                             # (first launches of the two kernels; LAGS draws, so that every update runs over the full window)
        on.append(ms_per_iteration(iters))
    return np.array(off), np.array(on)


R, S, _ = s.layout()
for LAGS in LAGS_LIST:
    s.set_schedule(10 ** 9, 0, 1)
    s.enable_diagnostics(True, LAGS, 0)
    s.run(LAGS + 2)
    D, _, _, _, words = s.diagnostics_layout()
    nbytes = (24 * LAGS + 48) * D
    ev = [s.debug_time_diagnostics(20) for _ in range(3)]
    k_upd = float(np.median([e[0] for e in ev]))
    print(f"diag {N}x{P} lags={LAGS} D={D}: device events, 3 x 20 launches: full-window update {np.round([e[0] for e in ev], 4).tolist()} ms, "
          f"{nbytes / 1e9:.3f} GB per update -> {nbytes / k_upd / 1e9:.2f} TB/s beside the measured-copy {COPY_TBS} TB/s ({nbytes / k_upd / 1e9 / COPY_TBS * 100:.0f} %); "
          f"finalise kernel {np.round([e[1] for e in ev], 4).tolist()} ms", flush=True)
    off, on = alternate(1)
    s.enable_diagnostics(True, LAGS, 0)
    upd = float(np.median(on) - np.median(off))
    print(f"diag {N}x{P} (R={R} S={S}) lags={LAGS} D={D} state {words * 8 / 1e9:.3f} GB; thin 1, {reps} x {iters} iterations alternating: off {np.round(off, 4).tolist()} ms "
          f"on {np.round(on, 4).tolist()} ms per iteration; cost per iteration = median on - median off = {upd:.4f} ms (off spread {off.max() - off.min():.4f} ms)", flush=True)
    off10, on10 = alternate(10)
    print(f"diag {N}x{P} lags={LAGS} thin 10: it/s off {np.round(1e3 / off10, 2).tolist()} on {np.round(1e3 / on10, 2).tolist()}; median off {1e3 / np.median(off10):.2f} "
          f"on {1e3 / np.median(on10):.2f} it/s; off spread {1e3 / off10.min() - 1e3 / off10.max():.2f} it/s; on - off = {1e3 / np.median(on10) - 1e3 / np.median(off10):+.2f} it/s "
          f"({(np.median(on10) - np.median(off10)) * 1e3:+.1f} us per iteration; a tenth of the update kernels' time is {k_upd * 100:.1f} us)", flush=True)
    s.enable_diagnostics(True, LAGS, 0)
    s.run(10 * min(LAGS + 3, 40))
    fin = []
    for _ in range(3):
        t0 = time.perf_counter(); d = s.diagnostics(); fin.append((time.perf_counter() - t0) * 1e3)
    print(f"diag {N}x{P} lags={LAGS} finalise after n = {d['n']} draws: ngp_get_diagnostics {np.round(fin, 3).tolist()} ms per call (kernel, output allocation "
          f"and 9 D-vector copies to the host); median ESS {np.median(d['ess']):.1f} of {d['n']}, truncated {int(d['truncated'].sum())} of {D}", flush=True)
s.close()
