"""The sweep plan of a panel: engine, layout, lag, near lags, streamer variant and grid for every rule of the planner.

Each case sets a generated panel (P = 256) on a fresh handle with the requests of the case and reads back what the library chose:
config() = (mode, lag D), layout() = (R, S), near(), streamer() = (variant, GEMV chains), and after one iteration census()["grid"]
(None in mode 0, which has no persistent sweep).  The expected values pin the planner of an MI355X (256 CUs); a change to any of them
is a change of the engine, not a refactor."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

P = 256

# name: (N, requests).  Requests: mode / lag (ngp_configure), streamer, storage, near, max_shards (an int, or ("chains", k) /
# ("pass", k): what shards_for_chains / shards_for_pass return).
CASES = {
    "mode0_forced": (10000, dict(mode=0, lag=8)),
    "phase_short_lag_auto": (10000, dict()),                      # 44-row shards: phase streamer, lag left automatic -> 6
    "phase_short_lag8": (10000, dict(mode=1, lag=8)),              # ... an explicit lag stays
    "phase_short_lag4": (10000, dict(mode=1, lag=4)),
    "phase_forced_rows84": (20000, dict(streamer=1)),              # 84-row shards, phase streamer on request
    "phase_tall_shards": (40000, dict(streamer=1)),                # shards over 128 rows: lag capped at 5, four near lags
    "phase_tall_shards_lag4": (40000, dict(streamer=1, mode=1, lag=4)),
    "rows_auto_64": (16000, dict()),                               # row-owning streamer from 64-row shards on
    "rows_auto_84": (20000, dict()),
    "rows_auto_lag8": (20000, dict(mode=1, lag=8)),                # register delay line: lag 6 at most
    "rows_auto_lag2": (20000, dict(mode=1, lag=2)),                # below lag 3: the phase streamer
    "rows_forced_short": (10000, dict(streamer=2)),
    "rows_tall_shards": (50000, dict()),                           # 204-row shards
    "tall_auto_v2": (70000, dict()),                               # over one resident wave of 256-row shards: V = 2
    "tall_forced_v2": (20000, dict(streamer=4)),
    "tall_forced_v3": (20000, dict(streamer=6)),
    "tall_forced_v3_shards": (20000, dict(streamer=6, max_shards=120)),
    "fallback_mode0": (70000, dict(mode=1, lag=2)),                # too tall for the persistent sweep without V > 1: mode 0
    "near_explicit_1": (10000, dict(near=1)),
    "near_explicit_4_rows": (20000, dict(near=4)),
    "shards_for_chains_3": (10000, dict(max_shards=("chains", 3))),
    "shards_for_pass_4": (10000, dict(max_shards=("pass", 4))),
    "shards_for_pass_8": (10000, dict(max_shards=("pass", 8))),
    "max_shards_100": (10000, dict(max_shards=100)),
    "u8_nt1_lag_auto": (2000, dict(storage=1)),                    # compact storage, one update task per lane
    "u8_nt1_lag12": (2000, dict(storage=1, mode=1, lag=12)),
    "u8_nt1_lag7": (2000, dict(storage=1, mode=1, lag=7)),
    "u8_nt1_lag5": (2000, dict(storage=1, mode=1, lag=5)),
    "u8_nt1_lag2": (2000, dict(storage=1, mode=1, lag=2)),
    "u8_nt1_tall_shards": (50000, dict(storage=1)),
    "u8_nt2_lag_auto": (80000, dict(storage=1)),                   # two update tasks
    "u8_nt2_lag6": (80000, dict(storage=1, mode=1, lag=6)),
    "u8_nt4_lag_auto": (120000, dict(storage=1)),                  # four update tasks
    "u8_near_1": (2000, dict(storage=1, near=1)),
    "u8_max_shards_60": (20000, dict(storage=1, max_shards=60)),
}

# (mode, D, R, S, near, variant, nchain, grid) as the planner chose them before it was gathered in one place
EXPECTED = {
    "fallback_mode0": (0, 1, 276, 254, 3, 0, 8, None),
    "max_shards_100": (1, 6, 100, 100, 2, 2, 7, 105),
    "mode0_forced": (0, 1, 44, 228, 3, 0, 8, None),
    "near_explicit_1": (1, 6, 44, 228, 1, 1, 8, 237),
    "near_explicit_4_rows": (1, 6, 84, 239, 4, 2, 7, 248),
    "phase_forced_rows84": (1, 6, 84, 239, 3, 1, 8, 248),
    "phase_short_lag4": (1, 4, 44, 228, 3, 1, 8, 237),
    "phase_short_lag8": (1, 8, 44, 228, 3, 1, 8, 237),
    "phase_short_lag_auto": (1, 6, 44, 228, 3, 1, 8, 237),
    "phase_tall_shards": (1, 5, 164, 244, 4, 1, 8, 253),
    "phase_tall_shards_lag4": (1, 4, 164, 244, 4, 1, 8, 253),
    "rows_auto_64": (1, 6, 68, 236, 2, 2, 7, 245),
    "rows_auto_84": (1, 6, 84, 239, 2, 2, 7, 248),
    "rows_auto_lag2": (1, 2, 84, 239, 3, 1, 8, 248),
    "rows_auto_lag8": (1, 6, 84, 239, 2, 2, 7, 248),
    "rows_forced_short": (1, 6, 44, 228, 3, 2, 7, 237),
    "rows_tall_shards": (1, 6, 204, 246, 2, 2, 7, 255),
    "shards_for_chains_3": (1, 6, 132, 76, 2, 2, 7, 80),
    "shards_for_pass_4": (1, 6, 44, 228, 3, 1, 8, 237),
    "shards_for_pass_8": (1, 6, 48, 209, 3, 1, 8, 217),
    "shared_owner": (1, 5, 200, 100, 1, 1, 8, 105),
    "tall_auto_v2": (1, 3, 148, 474, 2, 2, 7, 253),
    "tall_forced_v2": (1, 3, 44, 456, 3, 2, 7, 244),
    "tall_forced_v3": (1, 2, 36, 558, 3, 2, 7, 205),
    "tall_forced_v3_shards": (1, 2, 168, 120, 2, 2, 7, 45),
    "u8_max_shards_60": (1, 8, 336, 60, 2, 3, 7, 63),
    "u8_near_1": (1, 8, 16, 125, 1, 3, 7, 130),
    "u8_nt1_lag12": (1, 12, 16, 125, 3, 3, 7, 130),
    "u8_nt1_lag2": (1, 3, 16, 125, 3, 3, 7, 130),
    "u8_nt1_lag5": (1, 4, 16, 125, 3, 3, 7, 130),
    "u8_nt1_lag7": (1, 6, 16, 125, 3, 3, 7, 130),
    "u8_nt1_lag_auto": (1, 8, 16, 125, 3, 3, 7, 130),
    "u8_nt1_tall_shards": (1, 8, 208, 241, 2, 3, 7, 250),
    "u8_nt2_lag6": (1, 4, 336, 239, 2, 3, 7, 248),
    "u8_nt2_lag_auto": (1, 8, 336, 239, 2, 3, 7, 248),
    "u8_nt4_lag_auto": (1, 4, 496, 242, 2, 3, 7, 251),
}

# requests the library refuses: (N, requests, message)
REFUSED = {
    "u8_mode0": (2000, dict(storage=1, mode=0, lag=8), "compact storage runs in the persistent sweep"),
    "u8_too_tall": (240000, dict(storage=1), "N too large for one resident wave of streamers in compact storage"),
}


def configure(ngp, req):
    s = ngp.Sampler(device=0, seed=5, chain=0)
    if "mode" in req:
        s.configure(req["mode"], req["lag"])
    if "streamer" in req:
        s.set_streamer(req["streamer"])
    if "storage" in req:
        s.set_storage(req["storage"])
    if "near" in req:
        s.set_near(req["near"])
    ms = req.get("max_shards")
    if isinstance(ms, tuple):
        ms = s.shards_for_chains(ms[1]) if ms[0] == "chains" else s.shards_for_pass(ms[1])
    if ms is not None:
        s.set_max_shards(ms)
    return s


def observe(s, N):
    """config, layout, near lags, streamer and (after one iteration) the grid of a handle with a panel of N rows"""
    mode, D = s.config()
    R, S, _ = s.layout()
    near = s.near()
    variant, nchain = s.streamer()
    v = 0.01
    s.add_marker_set(0, P, 0, 4.0, v * 0.5, [(0, P)], [v])
    s.set_y(np.random.default_rng(1).normal(size=N))
    s.set_residual_prior(4.0, 0.5)
    s.set_schedule(1, 0, 1)
    s.run(1)
    grid = s.census()["grid"] if mode == 1 else None
    return (mode, D, R, S, near, variant, nchain, grid)


def measure(ngp, name):
    N, req = CASES[name]
    s = configure(ngp, req)
    s.generate_panel(N, P)
    return observe(s, N)


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan(ngp, name):
    assert measure(ngp, name) == EXPECTED[name]


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_plan_refused(ngp, name):
    N, req, msg = REFUSED[name]
    s = configure(ngp, req)
    with pytest.raises(Exception, match=msg):
        s.generate_panel(N, P)


def test_shared_panel_reports_the_owners_plan(ngp):
    """A handle that shares a panel takes its owner's plan, not one of its own requests (it has none here)."""
    N = 20000
    owner = configure(ngp, dict(mode=1, lag=5, near=1, max_shards=100, streamer=1))
    owner.generate_panel(N, P)
    h = ngp.Sampler(device=0, seed=6, chain=1)
    h.share_panel(owner)
    got = observe(h, N)
    assert got == EXPECTED["shared_owner"]
    assert observe(owner, N) == got
