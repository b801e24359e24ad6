"""The range contract of the sweep's fixed-point sums on the device.

1. Power-of-two scaling is exact: a chain over 2^k y (prior scales and start variances 2^2k) is 2^k times the chain over y, bit for
   bit, after every iteration and in the posterior sums -- an oracle-free property that any absolute constant, fp32 intermediate or
   clamp in a kernel breaks.  tests/test_fx_range_host.py shows the same on the blocked oracle.
2. Fused chains of unlike scales: K chains over one panel whose responses differ by up to 2^400 have K different fixed-point
   scales in one launch; every chain equals the chain it is alone and 2^s times its unit chain.
3. Small head residuals complete: the inputs of tests/fx_range_cases.py, which the scale rule before the floor could not hold
   (tests/test_fx_range_host.py walks each on the oracle), run to the end, bit for bit the blocked oracle's chain.

The wider model (a (1|g) random set, weights, held-out and censored rows, prediction, genomic variance) scales exactly too, on the
default engine at k = +-40: every one of its terms is cleared on its restatement in the host file first.  A BayesLV set is in no
case: its variance model takes logs of the squared effects and is not exactly equivariant."""
import math

import numpy as np
import pytest

import fx_range_cases as fx
from conftest import make_problem

pytestmark = pytest.mark.gpu

ENGINES = {  # name -> (Sampler kwargs, near lags or None, max shards or None, byte tiles)
    "blocklaunch": (dict(mode=0, lag=1, streamer=1), None, None, False),
    "persist_lag6": (dict(mode=1, lag=6, streamer=1), None, None, False),
    "persist_lag8_near4": (dict(mode=1, lag=8, streamer=1), 4, None, False),
    "rows_lag6_near2": (dict(mode=1, lag=6, streamer=2), 2, None, False),
    "tall_v2": (dict(mode=1, lag=6, streamer=4), None, 8, False),       # N = 1500: 8 shards of 188 rows, two per workgroup
    "tall_v3": (dict(mode=1, lag=6, streamer=6), None, 9, False),       # N = 1000: 9 shards, three per workgroup
    "bytes": (dict(mode=1, lag=6, storage="u8"), None, None, True),
    "bytes_6_shards": (dict(mode=1, lag=6, storage="u8"), None, 6, True),
}
SPEC3 = [(0, 150, "PR"), (150, 170, "B"), (320, 130, "R")]


def device(ngp, panel, engine, seed=1001, chain=0, owner=None, form=None):
    kw, near, shards, u8 = ENGINES[engine]
    s = ngp.Sampler(device=0, seed=seed, chain=chain, **kw)
    if form is not None:
        s.set_chain_form(form)
    if near is not None:
        s.set_near(near)
    if owner is not None:
        s.share_panel(owner)
        return s
    if shards:
        s.set_max_shards(shards)
    s.set_panel(panel, centre=True) if u8 else s.set_panel(panel)
    return s


def oracle_like(O, s, panel, seed=1001, chain=0):
    """the blocked oracle on the layout the library reports for s"""
    o = O.Oracle(order=1, seed=seed, chain=chain)
    R, S, _ = s.layout()
    if s.storage() == 1:
        o.set_panel_u8(panel, R=R, S=S, D=s.config()[1], near=s.near(), tform=s.chain_form())
    else:
        o.set_panel_f32(panel, R=R, S=S, D=s.config()[1], near=s.near(), nchain=s.streamer()[1], tform=s.chain_form())
    return o


# ------------------------------------------------------------------------------------------------------------------------------
# 1. power-of-two scaling
# ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine,N", [("blocklaunch", 400), ("persist_lag6", 400), ("persist_lag8_near4", 400), ("rows_lag6_near2", 400),
                                      ("tall_v2", 1500), ("tall_v3", 1000), ("bytes", 400)])
def test_power_of_two_scaling_is_exact(ngp, O, engine, N):
    P = 450
    X, y, bt, v = make_problem(O, N, P, seed=5)
    if ENGINES[engine][3]:
        from test_gpu_compact import make_codes
        X, y, v = make_codes(O, N, P)
    Xfix = fx.fixed_columns(N)
    res = {}
    for k in (0, -200, -40, 40, 200):
        s = device(ngp, X, engine)
        if engine.startswith("tall"):
            V = ENGINES[engine][0]["streamer"] // 2
            assert s.streamer() == (2, 7) and s.config() == (1, 5 - V) and s.layout()[1] % V == 0
        elif engine != "bytes":
            kw = ENGINES[engine][0]
            assert s.config() == (kw["mode"], kw["lag"]) and s.streamer()[0] == (kw["streamer"] if kw["mode"] else 0)
        fx.setup_scaled(s, SPEC3, v, y, k, prior=(4.0, 0.25 * y.var()), Xfix=Xfix)
        res[k] = fx.walk(s, rsets=(2,), has_fixed=True)
    assert res[0][1]["nKept"] == 2 and np.abs(res[0][0][-1]["beta"]).max() > 0.0
    for k in (-200, -40, 40, 200):
        fx.assert_scaled(res[0], res[k], k)


def test_power_of_two_scaling_of_a_tuple_set_in_the_inverse_form(ngp, O):
    from test_tuple_main_oracle import add_tuple, tuple_problem
    N, nloc, k2 = 300, 75, 2
    Xp, y, vm, v, span, off = tuple_problem(O, ngp, N, nloc, k2, extra=40)
    regions = [(0, nloc // 3), (nloc // 3, nloc)]
    res = {}
    for k in (0, -200, -40, 40, 200):
        s = ngp.Sampler(device=0, seed=21, chain=0)
        s.set_chain_form(1)
        s.set_panel(Xp)
        assert s.chain_form() == 1
        fx.setup_scaled(s, [(off, 40, "B")], v, y, k, prior=(4.0, 0.5), extra=lambda m, k: add_tuple(m, nloc, k2, np.ldexp(vm, 2 * k), regions))
        res[k] = fx.walk(s)
    for k in (-200, -40, 40, 200):
        fx.assert_scaled(res[0], res[k], k)


# ------------------------------------------------------------------------------------------------------------------------------
# 2. fused chains of unlike scales
# ------------------------------------------------------------------------------------------------------------------------------
SHIFTS = [0, 40, -40, 13, -7, 200, -200, 1]


def _fused_problem(ngp, O, kind):
    """(panel, y, model(s, k): the k-th chain's sets, response and priors, ids of the BayesR sets): the shapes of
    tests/test_gpu_chains_per_pass.py; a Tuple pass of that size beside them"""
    if kind == "plain":
        X, y, bt, v = make_problem(O, 500, 640, seed=6)
        spec = [(0, 300, "PR"), (300, 200, "B"), (500, 140, "R")]
        return X, y, (lambda s, k: fx.setup_scaled(s, spec, v, y, k)), (2,)
    if kind == "rows":
        X, y, bt, v = make_problem(O, 700, 520, seed=8)
        spec = [(0, 260, "PR"), (260, 260, "B")]
        return X, y, (lambda s, k: fx.setup_scaled(s, spec, v, y, k)), ()
    if kind == "bytes":
        from test_gpu_compact import make_codes
        G, y, v = make_codes(O, 500, 450)
        return G, y, (lambda s, k: fx.setup_scaled(s, SPEC3, v, y, k)), (2,)
    from test_tuple_main_oracle import add_tuple, tuple_problem
    nloc, k2 = 75, 2
    Xp, y, vm, v, span, off = tuple_problem(O, ngp, 500, nloc, k2, extra=40)
    regions = [(0, nloc // 3), (nloc // 3, nloc)]
    return Xp, y, (lambda s, k: fx.setup_scaled(s, [(off, 40, "B")], v, y, k, prior=(4.0, 0.5),
                                                extra=lambda m, kk: add_tuple(m, nloc, k2, np.ldexp(vm, 2 * kk), regions))), ()


@pytest.mark.parametrize("kind,K,lag", [("plain", 2, None), ("plain", 3, 6), ("plain", 8, None), ("rows", 2, 6), ("bytes", 2, 8), ("bytes", 3, 8), ("tuple", 2, 8)])
def test_fused_chains_of_unlike_scales(ngp, O, kind, K, lag):
    panel, y, model, rsets = _fused_problem(ngp, O, kind)
    kw = dict(mode=1, lag=lag) if lag else {}
    if kind == "bytes":
        kw["storage"] = "u8"

    def chain(c, owner=None, shards=None):
        s = ngp.Sampler(device=0, seed=1001 + c, chain=c, **kw)
        if kind == "tuple":
            s.set_chain_form(1)
        if owner is not None:
            s.share_panel(owner)
            return s
        s.set_max_shards(shards)
        s.set_panel(panel, centre=True) if kind == "bytes" else s.set_panel(panel)
        return s

    fused = []
    for c in range(K):
        if c == 0:
            probe = ngp.Sampler(device=0, seed=1, chain=0, **kw)
            fused.append(chain(0, shards=6 if kind == "rows" else probe.shards_for_pass(K)))
        else:
            fused.append(chain(c, owner=fused[0]))
        model(fused[c], SHIFTS[c])
    R, S, _ = fused[0].layout()
    ngp.Sampler.run_many(fused, fx.NITER)
    # ONE launch served all chains (as tests/test_gpu_chains_per_pass.py counts its workgroups)
    if kind == "plain":
        assert fused[0].streamer()[0] == 1
        assert fused[0].census()["grid"] == K + (((K + 1) // 2) if K >= 4 else K) * ((S + 31) // 32) + S
    else:
        assert fused[0].census()["grid"] == K * (1 + (S + 31) // 32) + S
    for c in range(K):
        f = (fx.snapshot(fused[c], rsets), fx.sums(fused[c], rsets))
        got = {}
        for k in sorted({0, SHIFTS[c]}):                # the chain of this seed and chain id alone: at unit scale and at its own
            a = chain(c, shards=S)
            assert a.layout()[:2] == (R, S)
            model(a, k)
            a.run(fx.NITER)
            got[k] = (fx.snapshot(a, rsets), fx.sums(a, rsets))
        for part in (0, 1):
            fx.assert_scaled_dict(got[SHIFTS[c]][part], f[part], 0, "fused chain %d against itself alone" % c)
            fx.assert_scaled_dict(got[0][part], f[part], SHIFTS[c], "fused chain %d against its unit chain" % c)
    assert not np.array_equal(np.ldexp(fused[0].get_state()["beta"], SHIFTS[1]), fused[1].get_state()["beta"])   # different chains


# ------------------------------------------------------------------------------------------------------------------------------
# 3. small head residuals complete
# ------------------------------------------------------------------------------------------------------------------------------
SMALL_ENGINES = {  # shape of tests/fx_range_cases.py -> the engines that run it
    "n300": ["persist_lag6", "rows_lag6_near2", "blocklaunch"], "n300_x4": ["persist_lag6", "rows_lag6_near2", "blocklaunch"],
    "n1500": ["tall_v2"], "n1500_x4": ["tall_v2"], "n300_bytes": ["bytes"], "n1500_bytes": ["bytes_6_shards"],
}
SMALL_RUNS = [(n, s, e) for n, s in fx.SMALL_CASES for e in SMALL_ENGINES[s]]


def _holds_together(s, st, y):
    resid = y - st["b"] - s.xbeta(st["beta"])
    assert np.abs(st["ycorr"] - resid).max() <= 1e-9 * np.abs(resid).max()


@pytest.mark.parametrize("name,shape,engine", SMALL_RUNS, ids=["%s-%s-%s" % r for r in SMALL_RUNS])
def test_small_head_residuals_complete(ngp, O, name, shape, engine):
    N, P, u8, _ = fx.SMALL_SHAPES[shape]
    panel, _ = fx.small_panel(O, shape)
    s = device(ngp, panel, engine)
    if engine == "tall_v2":
        assert s.streamer() == (2, 7) and s.config() == (1, 3)
    o = oracle_like(O, s, panel)
    fx.setup_small(o, name, N, P)
    if name != "fine_seam_zero":
        fx.setup_small(s, name, N, P)
        for m in (s, o):
            m.run(fx.NITER)
        a, b = s.get_state(), o.get_state()
        for key in ("ycorr", "beta", "delta", "varBeta"):
            assert np.array_equal(a[key], b[key][:len(a[key])]), key
        assert a["varE"] == b["varE"] and a["b"] == b["b"] and a["iter"] == b["iter"] == fx.NITER
        pa, pb = s.get_posterior_sums(), o.get_posterior_sums()
        for key in ("sum_beta", "sum_beta2", "sum_varBeta"):
            assert np.array_equal(pa[key], pb[key]), key
        assert pa["sum_varE"] == pb["sum_varE"] and pa["sum_b"] == pb["sum_b"] and pa["nKept"] == 2
        _holds_together(s, a, fx.small_y(name, N))
        return
    # the fine seam: six calls of ngp_sweep_set, the caller's arrays carried from call to call, from a zero residual and zero effects
    varE = fx.SMALL_HEADS[name][2]
    s.add_marker_set(0, P, 0, fx.SMALL_SET["df"], fx.SMALL_SET["scale"], [(0, P)], [fx.SMALL_SET["vb0"]])
    ycorr, beta, vb = np.zeros(N), np.zeros(P), np.array([fx.SMALL_SET["vb0"]])
    for it in range(fx.NITER):
        s.sweep_set(0, varE, ycorr, beta, vb)
        o.run(1)
        b = o.get_state()
        assert np.array_equal(ycorr, b["ycorr"]) and np.array_equal(beta, b["beta"][:P]) and vb[0] == b["varBeta"][0], it
    resid = -s.xbeta(beta)
    assert np.abs(ycorr - resid).max() <= 1e-9 * np.abs(resid).max()


@pytest.mark.parametrize("name,shape", [("tiny_y", "n300"), ("zero_y_wide_prior", "n300_x4"), ("zero_y_fixed_varE", "n300_x4")])
def test_small_head_residuals_complete_in_a_fused_pair(ngp, O, name, shape):
    N, P, u8, _ = fx.SMALL_SHAPES[shape]
    panel, _ = fx.small_panel(O, shape)
    probe = ngp.Sampler(device=0, seed=1, chain=0)
    fused = []
    for c in range(2):
        s = ngp.Sampler(device=0, seed=1001 + c, chain=c)
        if c == 0:
            s.set_max_shards(probe.shards_for_pass(2)); s.set_panel(panel)
        else:
            s.share_panel(fused[0])
        fx.setup_small(s, name, N, P)
        fused.append(s)
    S = fused[0].layout()[1]
    ngp.Sampler.run_many(fused, fx.NITER)
    assert fused[0].census()["grid"] == 2 + 2 * ((S + 31) // 32) + S
    for c in range(2):
        o = oracle_like(O, fused[0], panel, seed=1001 + c, chain=c)
        fx.setup_small(o, name, N, P)
        o.run(fx.NITER)
        a, b = fused[c].get_state(), o.get_state()
        for key in ("ycorr", "beta", "delta", "varBeta"):
            assert np.array_equal(a[key], b[key][:len(a[key])]), (c, key)
        assert a["varE"] == b["varE"] and a["b"] == b["b"] and a["iter"] == fx.NITER
        _holds_together(fused[c], a, fx.small_y(name, N))


@pytest.mark.parametrize("k", [-40, 40])
def test_tiny_response_scales_exactly(ngp, O, k):
    N, P, u8, _ = fx.SMALL_SHAPES["n300"]
    panel, _ = fx.small_panel(O, "n300")
    res = {}
    for kk in (0, k):
        s = device(ngp, panel, "persist_lag6")
        fx.setup_small(s, "tiny_y", N, P, k=kk)
        res[kk] = fx.walk(s)
    fx.assert_scaled(res[0], res[k], k)


# ------------------------------------------------------------------------------------------------------------------------------
# 1'. the wider model on the default engine: every term tests/test_fx_range_host.py cleared on its restatement
# ------------------------------------------------------------------------------------------------------------------------------
def _wide_chain(ngp, O, k, weighted):
    """weighted: power-of-four residual weights and no genomic variance (the library forms none over row-scaled tiles); else the
    genomic variance of two sets' windows, the sets and the total"""
    N, P = 400, 450
    X, y, bt, v = make_problem(O, N, P, seed=5)
    rng = np.random.default_rng(31)
    w = rng.choice([0.25, 1.0, 4.0, 16.0], size=N)           # powers of four: the row scales are powers of two
    level = rng.integers(0, 9, size=N)
    H = np.arange(5, N, 20).astype(np.int64)                  # 20 held-out rows
    A = np.arange(2, N, 10).astype(np.int64)                  # 40 censored rows, none of them held out
    kk = np.arange(len(A)) % 3
    sd = y.std()
    lo = np.where(kk == 0, y[A] - 0.3 * sd, np.where(kk == 1, -np.inf, y[A] - 0.2 * sd))
    hi = np.where(kk == 0, np.inf, np.where(kk == 1, y[A] + 0.3 * sd, y[A] + 0.4 * sd))
    Xnew, _ = O.generate_panel(30, P, seed=77)                # 30 new individuals
    s = ngp.Sampler(device=0, seed=1001, chain=0)
    if weighted:
        s.set_residual_weights(w)
    s.set_panel(X)
    s.set_prediction_panel(Xnew)
    fx.add_sets(s, SPEC3, math.ldexp(v, 2 * k))
    s.add_fixed_set(fx.fixed_columns(N))
    s.add_random_set(level, 9, varU0=math.ldexp(0.3 * y.var(), 2 * k))
    if not weighted:
        s.set_variance_windows(0, [(0, 40), (60, 150)]); s.set_variance_windows(2, [(0, 130)])
        s.enable_genomic_variance(True, 0.01)
    s.set_holdout(H)
    s.set_censored(A, np.ldexp(lo, k), np.ldexp(hi, k))
    s.set_y(np.ldexp(y, k)); s.set_residual_prior(4.0, math.ldexp(0.25 * y.var(), 2 * k)); s.set_schedule(*fx.SCHEDULE)
    hist, ps = fx.walk(s, rsets=(2,), has_fixed=True)
    return dict(hist=hist, sums=ps, random=s.get_random(0), holdout=s.holdout_state(), liab=s.liability_state(), pred=s.prediction(),
                pred_sums=s.prediction_sums(), gv=None if weighted else s.genomic_variance_sums(), fell=s.liability_fallthrough())


def _same(a, b, p, what):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert np.isfinite(b).all() and np.array_equal(np.ldexp(a, p), b), what


@pytest.mark.parametrize("weighted", [True, False], ids=["weights", "genomic_variance"])
def test_the_wider_model_scales_exactly(ngp, O, weighted):
    """a (1|g) random set, held-out rows, censored rows, prediction of new individuals and either power-of-four weights or genomic
    variance beside the marker and fixed sets, on the default engine: effects, predictions and fitted values scale with 2^k, variances with
    2^2k, and the shares q, the ratio r and the window posterior probabilities do not move"""
    unit = _wide_chain(ngp, O, 0, weighted)
    assert unit["fell"] == 0 and unit["holdout"]["n_fit"].sum() == 40.0 and unit["sums"]["nKept"] == 2
    assert weighted or (unit["gv"]["nKept"] == 2 and unit["gv"]["sumV"][-1] > 0.0)
    for k in (-40, 40):
        r = _wide_chain(ngp, O, k, weighted)
        fx.assert_scaled((unit["hist"], unit["sums"]), (r["hist"], r["sums"]), k)
        u, s = unit["random"], r["random"]
        for key, p in (("u", k), ("sum_u", k), ("varU", 2 * k), ("sum_varU", 2 * k)):
            _same(u[key], s[key], p, key)
        for key, p in (("rows", 0), ("yaug", k), ("sum_fit", k), ("sum_fit2", 2 * k), ("n_fit", 0)):
            _same(unit["holdout"][key], r["holdout"][key], p, key)
        _same(unit["liab"]["rows"], r["liab"]["rows"], 0, "censored rows"); _same(unit["liab"]["liab"], r["liab"]["liab"], k, "liab")
        assert r["fell"] == 0
        _same(unit["pred"]["mean"], r["pred"]["mean"], k, "prediction mean"); _same(unit["pred"]["sd"], r["pred"]["sd"], k, "prediction sd")
        _same(unit["pred_sums"]["sum"], r["pred_sums"]["sum"], k, "prediction sum"); _same(unit["pred_sums"]["sum2"], r["pred_sums"]["sum2"], 2 * k, "prediction sum2")
        if weighted:
            continue
        # V, q = V / V_total, the window indicators q > threshold (WPPA = count / nKept) and r = V_total / (V_total + varE)
        for key, p in (("sumV", 2 * k), ("sumV2", 4 * k), ("sumQ", 0), ("sumQ2", 0), ("count", 0), ("last", 2 * k), ("ratio", 0)):
            _same(unit["gv"][key], r["gv"][key], p, key)
        assert r["gv"]["nKept"] == 2
