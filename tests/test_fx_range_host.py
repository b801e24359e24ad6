"""The range contract of the sweep's fixed-point sums on the blocked oracle, CPU only.

1. Power-of-two scaling: the oracle's chain over 2^k y (prior scales and start variances 2^2k) is 2^k times its chain over y, bit
   for bit -- state after every iteration and posterior sums.  tests/test_gpu_fx_range.py holds the device to the same property.
   The terms of the wider model (a (1|g) random set, weights, held-out rows, censored rows, prediction, genomic variance) are
   cleared one at a time on their restatements under tests/ref_*.py at k = +-40 (the test_wide_* cases below) and then join the
   device case.  A BayesLV set is not exactly equivariant (its variance model takes logs of the squared effects, and
   log(4^k x) = log(x) + k log 4 rounds) and is left out for that reason, here and on the device.  Binary and ordinal traits hold
   varE at 1 and have no scale to move.
2. The scale rule restated in numpy, before and after the floor, walked along the oracle's chain of every small-head input: each
   input is outside the old limit at least twofold in its first iteration and at least fourfold inside the new one in every
   iteration.
3. The oracle's range check: refuses the tiny response under the rule before the floor (a test-only switch), accepts it under the
   rule in force."""
import math

import numpy as np
import pytest

import fx_range_cases as fx
from conftest import add_sets, make_problem

LAYOUT = dict(R=64, S=5, D=6, near=3)      # N = 300


def _oracle(O, X, seed=1001, chain=0, tform=0, u8=False, **layout):
    o = O.Oracle(order=1, seed=seed, chain=chain)
    lay = dict(LAYOUT, **layout)
    if u8:
        o.set_panel_u8(X, R=lay["R"], S=lay["S"], D=lay["D"], near=lay["near"], tform=tform)
    else:
        o.set_panel_f32(X, R=lay["R"], S=lay["S"], D=lay["D"], near=lay["near"], nchain=lay.get("nchain", 8), tform=tform)
    return o


def _rsets(spec):
    return [i for i, s in enumerate(spec) if isinstance(s[2], str) and s[2].startswith("R")]


def _scaling(O, X, y, v, spec, shifts, Xfix=None, u8=False, prior=(4.0, 1.0), **layout):
    res = {}
    for k in [0] + list(shifts):
        o = _oracle(O, X, u8=u8, **layout)
        fx.setup_scaled(o, spec, v, y, k, prior=prior, Xfix=Xfix)
        res[k] = fx.walk(o, _rsets(spec), Xfix is not None)
    for k in shifts:
        fx.assert_scaled(res[0], res[k], k)
    return res[0]


@pytest.mark.parametrize("kind,P", [("PR", 200), ("PR1", 200), ("B", 256), ("C", 200), ("R", 256)])
def test_marker_and_fixed_sets_scale_exactly(O, kind, P):
    N = 300
    X, y, bt, v = make_problem(O, N, P, seed=5)
    unit = _scaling(O, X, y, v, [(0, P, kind)], [-200, -40, -12, 12, 40, 200], Xfix=fx.fixed_columns(N), prior=(4.0, 0.25 * y.var()))
    assert not np.array_equal(unit[0][0]["beta"], unit[0][-1]["beta"]) and unit[1]["nKept"] == 2


def test_the_device_model_scales_exactly(O):
    """the model of the device cases (PR + BayesB + BayesR + a two-column fixed set, N = 400, P = 450)"""
    N, P = 400, 450
    X, y, bt, v = make_problem(O, N, P, seed=5)
    _scaling(O, X, y, v, [(0, 150, "PR"), (150, 170, "B"), (320, 130, "R")], [-200, -40, 40, 200], Xfix=fx.fixed_columns(N), prior=(4.0, 0.25 * y.var()),
             R=80, S=5)


def test_byte_tiles_scale_exactly(O):
    from test_gpu_compact import make_codes
    N, P = 300, 256
    G, y, v = make_codes(O, N, P)
    _scaling(O, G, y, v, [(0, 128, "R"), (128, 128, "B")], [-40, 12, 40, 200], u8=True, prior=(4.0, 0.25 * y.var()), near=2)


@pytest.mark.parametrize("tform", [0, 1], ids=["steps", "inverse_form"])
def test_tuple_sets_scale_exactly(O, ngp, tform):
    from test_tuple_main_oracle import add_tuple, tuple_problem
    N, nloc, k2 = 300, 75, 2
    Xp, y, vm, v, span, off = tuple_problem(O, ngp, N, nloc, k2, extra=40)
    regions = [(0, nloc // 3), (nloc // 3, nloc)]
    res = {}
    for k in (0, -40, 12, 40, 200):
        o = _oracle(O, Xp, seed=21, tform=tform)
        fx.setup_scaled(o, [(off, 40, "B")], v, y, k, prior=(4.0, 0.5), extra=lambda m, k: add_tuple(m, nloc, k2, np.ldexp(vm, 2 * k), regions))
        res[k] = fx.walk(o)
    for k in (-40, 12, 40, 200):
        fx.assert_scaled(res[0], res[k], k)


def test_the_floor_does_not_bind_in_an_ordinary_chain(O):
    """a response of order one: ycorr'ycorr at the head is far above W varE / 256 in every iteration, the exponent is the one from
    ycorr'ycorr alone (so every chain recorded before the floor stays bit for bit what it was)"""
    N, P = 300, 200
    X, y, bt, v = make_problem(O, N, P, seed=5)
    mpm_max = (X.astype(np.float64) ** 2).sum(axis=0).max()
    o = _oracle(O, X)
    add_sets(o, [(0, P, "PR")], v); o.set_y(y); o.set_residual_prior(4.0, 0.25 * y.var()); o.set_schedule(20, 4, 2)
    yc = y.copy()
    for it in range(20):
        yy = float(yc @ yc)
        o.run(1)
        st = o.get_state()
        assert fx.limit_new(mpm_max, yy, N, st["varE"]) == fx.limit_old(mpm_max, yy)
        assert yy > 32 * 2.0 ** -8 * N * st["varE"]          # ... and not by a hair: N varE is of the order of yy
        yc = st["ycorr"]


HOST_LAYOUTS = {  # shape -> an oracle layout for it (the device cases take the layout the library reports)
    "n300": dict(R=64, S=5, D=6, near=3), "n300_x4": dict(R=64, S=5, D=6, near=3),
    "n1500": dict(R=188, S=8, D=3, near=2, nchain=7), "n1500_x4": dict(R=188, S=8, D=3, near=2, nchain=7),
    "n300_bytes": dict(R=64, S=5, D=6, near=2), "n1500_bytes": dict(R=256, S=6, D=6, near=2),
}


def walk_small(O, name, shape, k=0, old_rule=False, out=None):
    """the oracle's chain of a small-head input; per iteration (head yy, varE, largest |x_j'ycorr|, largest shard partial, largest
    mpm_j |beta_j|, old limit, new limit), the residual and the shard partials as the iteration leaves them"""
    N, P, u8, _ = fx.SMALL_SHAPES[shape]
    lay = HOST_LAYOUTS[shape]
    Xp, X64 = fx.small_panel(O, shape)
    mpm = (X64 ** 2).sum(axis=0)
    o = _oracle(O, Xp, u8=u8, **lay)
    o.set_fx_rule(old_rule)
    fx.setup_small(o, name, N, P, k=k)
    rows = []
    yc = fx.small_y(name, N, k)
    R = lay["R"]
    for it in range(fx.NITER):
        yy = float(yc @ yc)
        o.run(1)
        st = o.get_state()
        yc = st["ycorr"]
        full = np.abs(X64.T @ yc).max()
        part = max(np.abs(X64[s:s + R].T @ yc[s:s + R]).max() for s in range(0, N, R))
        mb = (mpm * np.abs(st["beta"][:P])).max()
        rows.append((yy, st["varE"], full, part, mb, fx.limit_old(mpm.max(), yy), fx.limit_new(mpm.max(), yy, N, st["varE"])))
        if out is not None:
            out.append(st)
    resid = fx.small_y(name, N, k) - st["b"] - X64 @ st["beta"][:P]
    return rows, np.abs(st["ycorr"] - resid).max() / np.abs(resid).max()


@pytest.mark.parametrize("name,shape", fx.SMALL_CASES, ids=["%s-%s" % c for c in fx.SMALL_CASES])
def test_small_heads_are_outside_the_old_limit_and_inside_the_new(O, name, shape):
    rows, rel = walk_small(O, name, shape)
    print("\n%s / %s: ycorr against y - b - X beta %.1e relative" % (name, shape, rel))
    print("  it      head yy       varE   max|x'ycorr|  max|partial|  max mpm|beta|    old limit    new limit")
    for it, r in enumerate(rows):
        print("  %2d  %11.3e  %9.3e  %12.4g  %12.4g  %13.4g  %11.4g  %11.4g" % ((it + 1,) + r))
    yy, varE, full, part, mb, lo, ln = rows[0]
    assert full >= 2.0 * lo                                   # sharp: the first iteration's terms leave the old range twofold
    for yy, varE, full, part, mb, lo, ln in rows:
        assert 4.0 * max(full, part, mb) <= ln                # away from the edge: fourfold inside the new range, every iteration
    assert rel < 1e-9
    # the terms themselves (shard partials, far look-ahead terms) against the rule before the floor: the oracle's own check
    try:
        walk_small(O, name, shape, old_rule=True)
        refused = False
    except RuntimeError as e:
        assert "fixed-point range" in str(e)
        refused = True
    print("  under the rule before the floor the oracle %s" % ("refuses this input" if refused else "completes"))
    assert refused == ((name, shape) in fx.OLD_RULE_REFUSES)


@pytest.mark.parametrize("k", [-40, 40])
def test_tiny_response_scales_exactly(O, k):
    unit, scaled = [], []
    walk_small(O, "tiny_y", "n300", out=unit)
    walk_small(O, "tiny_y", "n300", k=k, out=scaled)
    for u, s in zip(unit, scaled):
        fx.assert_scaled_dict(u, s, k, "tiny_y")


def test_oracle_refuses_what_the_rule_before_the_floor_could_not_hold(O):
    """the oracle's range check (|term scale| >= 2^53, the device's abort 7): the tiny response under the rule before the floor is
    refused at the first iteration with an error that names the fixed-point range; under the rule in force the chain completes"""
    with pytest.raises(RuntimeError, match="fixed-point range"):
        walk_small(O, "tiny_y", "n300", old_rule=True)
    rows, rel = walk_small(O, "tiny_y", "n300")
    assert len(rows) == fx.NITER and rel < 1e-9
    # a chain of order one passes the check under either rule
    N, P = 300, 200
    X, y, bt, v = make_problem(O, N, P, seed=5)
    for old in (True, False):
        o = _oracle(O, X)
        o.set_fx_rule(old)
        add_sets(o, [(0, P, "B")], v); o.set_y(y); o.set_residual_prior(4.0, 0.25 * y.var()); o.run(6)
        assert o.get_state()["iter"] == 6


# ------------------------------------------------------------------------------------------------------------------------------
# the wider model, one term at a time on the restatements of tests/ref_*.py: each is exactly equivariant, so each is in the device
# case (tests/test_gpu_fx_range.py::test_the_wider_model_scales_exactly)
# ------------------------------------------------------------------------------------------------------------------------------
WIDE_K = (-40, 40)


def _wide_inputs(O, N=96, P=64):
    X, y, bt, v = make_problem(O, N, P, seed=5)
    rng = np.random.default_rng(17)
    w = 4.0 ** rng.integers(-1, 2, size=N)                   # power-of-four weights: the row scales sqrt(w) are powers of two
    return X, y, v, w, rng


def test_wide_weights_scale_exactly(O):
    """weighted residuals, the reference's order restated (ref_numpy_weighted.WeightedRefChain): BayesPR and BayesB sets"""
    from ref_numpy_weighted import WeightedRefChain
    X, y, v, w, rng = _wide_inputs(O)
    res = {}
    for k in (0,) + WIDE_K:
        c = WeightedRefChain(O, X, np.ldexp(y, k), w, 1001, 0)
        vk = math.ldexp(v, 2 * k)
        c.add_set(0, 32, 0, 4.0, vk * 0.5, [(0, 32)], [vk])
        c.add_set(32, 32, 1, 4.0, vk * 0.5, [(j, j + 1) for j in range(32)], [vk] * 32, pi0=0.2, estPi=True)
        c.E_df, c.E_scale = 4.0, math.ldexp(0.25 * y.var(), 2 * k)
        c.run(4)
        res[k] = c
    for k in WIDE_K:
        u, s = res[0], res[k]
        assert np.array_equal(np.ldexp(u.ycorr, k), s.ycorr) and np.ldexp(u.b[0], k) == s.b[0] and math.ldexp(u.varE, 2 * k) == s.varE
        for si in range(2):
            assert np.array_equal(np.ldexp(u.beta[si], k), s.beta[si]) and np.array_equal(u.delta[si], s.delta[si])
            assert np.array_equal(np.ldexp(u.varBeta[si], 2 * k), s.varBeta[si])


def test_wide_random_step_scales_exactly(O):
    """a (1|g) random set under weights, the device's order restated (ref_random.random_step_blocked)"""
    import ref_random as rr
    X, y, v, w, rng = _wide_inputs(O)
    N, q = len(y), 7
    level = rng.integers(0, q, size=N)
    rs = np.sqrt(w)
    zpz = rr.zpz_of(level, q, w)
    yt0 = rs * (y - y.mean()); u0 = rng.normal(size=q)
    unit = rr.random_step_blocked(O, 1001, 0, 3, 0, yt0, rs, level, q, None, zpz, u0, 2.5, 1.7, 4.0, 1.25)
    for k in WIDE_K:
        s = rr.random_step_blocked(O, 1001, 0, 3, 0, np.ldexp(yt0, k), rs, level, q, None, zpz, np.ldexp(u0, k), math.ldexp(2.5, 2 * k),
                                   math.ldexp(1.7, 2 * k), 4.0, math.ldexp(1.25, 2 * k))
        assert np.array_equal(np.ldexp(unit[0], k), s[0]) and np.array_equal(np.ldexp(unit[1], k), s[1]) and math.ldexp(unit[2], 2 * k) == s[2]


def test_wide_held_out_and_censored_rows_scale_exactly(O):
    """the augmentation steps of held-out rows (ref_holdout.step) and of censored rows (ref_liability.step), under weights"""
    import ref_holdout as rh
    import ref_liability as rl
    rng = np.random.default_rng(23)
    m = 12
    yaug, r, z = rng.normal(size=m) + 10.0, rng.normal(size=m), rng.normal(size=m)
    sH = 2.0 ** rng.integers(-1, 2, size=m).astype(np.float64)
    unit = rh.step(yaug, r, 1.7, z, sH)
    rows = np.arange(3, 3 + m)
    lo = np.where(rng.uniform(size=m) < 0.5, 9.5, -np.inf); hi = np.where(np.isfinite(lo), np.where(rng.uniform(size=m) < 0.5, np.inf, 11.0), 10.2)
    ul = rl.step(O, rows, yaug, r, 1.7, lo, hi, 1001, 0, 3, sH)
    assert ul[3] == 0
    for k in WIDE_K:
        s = rh.step(np.ldexp(yaug, k), np.ldexp(r, k), math.ldexp(1.7, 2 * k), z, sH)
        for a, b in zip(unit, s):
            assert np.array_equal(np.ldexp(a, k), b)
        s = rl.step(O, rows, np.ldexp(yaug, k), np.ldexp(r, k), math.ldexp(1.7, 2 * k), np.ldexp(lo, k), np.ldexp(hi, k), 1001, 0, 3, sH)
        for a, b in zip(ul[:3], s[:3]):
            assert np.array_equal(np.ldexp(a, k), b)


def test_wide_prediction_and_genomic_variance_scale_exactly(O):
    """g = X beta of one draw (ref_predict.predict_draw) scales with 2^k; the genomic variances V (ref_genvar.draw) with 2^2k, their
    exponents E move by k, and the shares q, the ratio r and the window indicators (ref_genvar.Sums.add) do not move"""
    import ref_genvar as rg
    import ref_predict as rp
    X, y, v, w, rng = _wide_inputs(O, N=40, P=96)
    beta = rng.normal(size=96) * (rng.uniform(size=96) < 0.3) * 0.1
    sets = [(0, 64), (64, 32)]
    windows = [[(0, 20), (30, 64)], [(0, 32)]]
    X64 = X.astype(np.float64)
    g0 = rp.predict_draw(X64, beta, sets)
    V0, E0 = rg.draw(X64, beta, sets, windows)
    S0 = rg.Sums(len(V0), 0.01)
    q0, r0 = S0.add(V0, 1.7)
    assert V0[-1] > 0.0
    for k in WIDE_K:
        assert np.array_equal(np.ldexp(g0, k), rp.predict_draw(X64, np.ldexp(beta, k), sets))
        V, E = rg.draw(X64, np.ldexp(beta, k), sets, windows)
        assert np.array_equal(np.ldexp(V0, 2 * k), V) and [e + k for e in E0] == E
        S = rg.Sums(len(V), 0.01)
        q, r = S.add(V, math.ldexp(1.7, 2 * k))
        assert np.array_equal(q0, q) and r0 == r and np.array_equal(S0.a[4], S.a[4])
