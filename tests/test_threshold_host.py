"""Ordered traits on the scale of the trait, the parts that need no device: the symbols and the stream kind, the two new headers'
discipline, the restated normal distribution function against scipy, the restated Cowles step on a hand-made state, the mirror's
argument checks, the cross-validation scores against a direct computation, the layout tails and the Julia bindings."""
import os
import re

import numpy as np
import pytest
from scipy import special

import ref_threshold as RT
from test_julia_shim_static import C2J, c_declarations, julia_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nextgp.jl_amd", "csrc")
NEW = ["ngp_set_threshold_step", "ngp_get_threshold_step", "ngp_set_threshold_step_state", "ngp_enable_class_probabilities",
       "ngp_get_class_probabilities", "ngp_set_class_probabilities", "ngp_debug_pnorm"]
INF = np.inf
TOL = 4e-12                      # per term; 2^18 terms keep log R within about 1e-6
GRID_A = np.arange(-37.0, 8.0 + 1e-9, 0.25)
WIDTHS = (1e-3, 0.01, 0.1, 1.0, 5.0, INF)


def grid_intervals():
    """Every interval of the accuracy grid and its mirror image."""
    out = []
    for a in GRID_A:
        for w in WIDTHS:
            out.append((a, a + w))
            out.append((-(a + w), -a))
    return out


def scipy_lpdiff(a, b):
    """log(Phi(b) - Phi(a)) from log_ndtr on the side that does not cancel."""
    if a >= 0:
        a, b = -b, -a
    lb, la = special.log_ndtr(b), special.log_ndtr(a)
    return lb + np.log1p(-np.exp(la - lb))


def test_symbols_stream_kind_and_abi_version(ngp):
    hdr = open(os.path.join(ROOT, "include", "nextgp_hip.h")).read()
    assert "#define NGP_ABI_VERSION 4" in hdr
    decl = c_declarations()
    for s in NEW:
        assert s in ngp.SYMBOLS and s in decl, s
    assert decl["ngp_set_threshold_step"] == ["ngp_handle*", "int32_t", "double"]
    assert decl["ngp_get_threshold_step"] == ["ngp_handle*", "int32_t*", "double*", "int64_t*", "int64_t*"]
    assert decl["ngp_set_threshold_step_state"] == ["ngp_handle*", "double", "int64_t", "int64_t"]
    assert decl["ngp_enable_class_probabilities"] == ["ngp_handle*", "int32_t"]
    assert decl["ngp_get_class_probabilities"] == ["ngp_handle*", "double*", "int64_t", "int32_t"]
    assert decl["ngp_set_class_probabilities"] == ["ngp_handle*", "double*", "int64_t", "int32_t"]
    assert decl["ngp_debug_pnorm"] == ["ngp_handle*", "int32_t", "double*", "double*", "int64_t", "double*"]
    src = open(os.path.join(CSRC, "ngp_api.hip")).read()
    for s in NEW:                                                   # every entry point behind the exception barrier
        assert re.search(r"\nint32_t " + s + r"\([^)]*\) \{\n    NGP_TRY\n", src), s
    thr_h = open(os.path.join(CSRC, "ngp_threshold.h")).read()
    assert re.search(r"^#define NGP_KIND_THRESHOLD_MH 24\b", thr_h, flags=re.M) and RT.KIND_THRESHOLD_MH == 24
    kinds = re.findall(r"^#define NGP_KIND_\w+ (\d+)\b", open(os.path.join(CSRC, "ngp_rng.h")).read(), flags=re.M)
    assert "24" not in kinds                                        # no other stream has the kind
    assert re.search(r"^#define NGP_THR_WG 1024\b", thr_h, flags=re.M) and RT.WG == 1024
    assert re.search(r"^#define NGP_THR_TARGET 0\.44\b", thr_h, flags=re.M) and RT.TARGET == 0.44
    assert "#define NGP_THR_LS_MIN (-20.0)" in thr_h and "#define NGP_THR_LS_MAX 0.0" in thr_h and (RT.LS_MIN, RT.LS_MAX) == (-20.0, 0.0)
    for name in ("k_threshold_terms", "k_threshold_decide", "k_holdout_prob"):
        assert name in thr_h and name in src, name
    assert ngp.THRESHOLD_STEPS == {"albert-chib": 0, "cowles": 1}


def test_the_new_headers_keep_the_draw_layers_discipline():
    """No inline assembly, no open loop, no contraction, no floating-point atomic, no libm call; and the sweep units know neither."""
    for h in ("ngp_pnorm.h", "ngp_threshold.h"):
        k = open(os.path.join(CSRC, h)).read()
        assert "#pragma clang fp contract(off)" in k, h
        code = re.sub(r"//[^\n]*", "", k)
        assert "asm" not in code and "while" not in code and "for (;;)" not in code and "goto" not in code, h
        assert "atomic" not in code.replace("rng_tnormal", ""), h
        for fn in ("exp(", "log(", "erf", "pow(", "sqrt("):
            for m in re.finditer(re.escape(fn), code):
                assert code[max(0, m.start() - 4):m.start()] == "det_", (h, fn, code[m.start() - 20:m.start() + 10])
    for unit in ("ngp_sweep.h", "ngp_sweep_inst.hip", "ngp_sweep_body.inc", "ngp_sweep_multi_body.inc", "ngp_sweep_args.h"):
        txt = open(os.path.join(CSRC, unit)).read()
        assert "ngp_pnorm" not in txt and "ngp_threshold" not in txt and "liab" not in txt, unit
    api = open(os.path.join(CSRC, "ngp_api.hip")).read()
    assert '#include "ngp_threshold.h"' in api


def test_pnorm_and_lpdiff_agree_with_scipy_on_the_grid(O):
    """4e-12 max(1, |value|) on a in [-37, 8] step 0.25, widths 1e-3 .. 5 and +inf, and the mirrored intervals; the measured maximum
    is 8.5e-14."""
    worst = 0.0
    for a in GRID_A:
        got, want = RT.pnorm(O, a), special.ndtr(a)
        assert abs(got - want) <= TOL * want, a                      # relative: the lower tail keeps its digits
        assert abs(np.log(got) - special.log_ndtr(a)) <= TOL * max(1.0, abs(special.log_ndtr(a))), a
    for a, b in grid_intervals():
        got, want = RT.lpdiff(O, a, b), scipy_lpdiff(a, b)
        err = abs(got - want) / max(1.0, abs(want))
        worst = max(worst, err)
        assert err <= TOL, (a, b, got, want)
    print("largest error of lpdiff on the grid:", worst)
    assert worst < 1e-12
    iv = np.array(grid_intervals() + [(1.0, 1.0), (np.nan, 0.0), (-INF, INF), (40.0, 41.0)])   # the vector forms are the scalar ones
    assert np.array_equal(RT.lpdiff_v(O, iv[:, 0], iv[:, 1]), [RT.lpdiff(O, a, b) for a, b in iv])
    xs = np.concatenate([GRID_A, [np.nan, INF, -INF, 39.0]])
    assert np.array_equal(RT.pnorm_v(O, xs), [RT.pnorm(O, v) for v in xs], equal_nan=True)


def test_pnorm_and_lpdiff_at_the_extremes(O):
    assert RT.pnorm(O, -INF) == 0.0 and RT.pnorm(O, INF) == 1.0 and np.isnan(RT.pnorm(O, np.nan))
    assert RT.pnorm(O, 0.0) == 0.5 and RT.pnorm(O, -40.0) == 0.0 and RT.pnorm(O, 40.0) == 1.0
    assert RT.lpdiff(O, -INF, INF) == 0.0
    for a, b in ((1.0, 1.0), (2.0, 1.0), (np.nan, 1.0), (0.0, np.nan), (INF, INF), (-INF, -INF), (40.0, 41.0)):
        assert RT.lpdiff(O, a, b) == -INF, (a, b)
    x = np.linspace(-6.0, 6.0, 25)                                   # both sides of the three switches |x| = sqrt 2, 8 sqrt 2
    for v in list(x) + [-np.sqrt(2.0), np.sqrt(2.0), -8.0 * np.sqrt(2.0) - 1e-9, -8.0 * np.sqrt(2.0) + 1e-9]:
        assert abs(RT.pnorm(O, v) - special.ndtr(v)) <= 4e-16 + 1e-15 * special.ndtr(v), v
    assert abs(RT.lpdiff(O, -1.0, 2.0) - np.log(special.ndtr(2.0) - special.ndtr(-1.0))) < 1e-15


# ---- the restated step on a hand-made state, C = 4 ----
CLS = np.array([1, 1, 2, 2, 2, 3, 3, 4, 4, 4])
LIAB = np.array([-1.2, -0.3, 0.2, 0.5, 0.6, 0.9, 1.3, 1.7, 2.2, 3.0])
RES = np.array([-0.4, 0.1, -0.2, 0.3, 0.1, -0.1, 0.2, 0.0, 0.4, 0.9])
THR = np.array([-INF, 0.0, 0.75, 1.5, INF])


def test_proposal_streams_order_and_collapse(O):
    g, ok = RT.propose(O, THR, 4, 0.25, 7, 0, 3)
    z2, f2 = RT.tnormal(O, RT.Uniforms(O, 7, 0, 3, 24, 2), (0.0 - 0.75) / 0.25, (1.5 - 0.75) / 0.25)
    assert not f2 and g[2] == 0.75 + 0.25 * z2                       # t_2 between g_1 = 0 and the OLD t_3
    z3, f3 = RT.tnormal(O, RT.Uniforms(O, 7, 0, 3, 24, 3), (g[2] - 1.5) / 0.25, INF)
    assert not f3 and g[3] == 1.5 + 0.25 * z3 and ok                 # t_3 above the NEW t_2
    assert np.array_equal(g[[0, 1, 4]], THR[[0, 1, 4]]) and 0.0 < g[2] < g[3]
    # a draw that lands on its lower bound: g_3 = t_3 + sigma (g_2 - t_3) / sigma = g_2 (all dyadic), not strictly ordered
    g, ok = RT.propose(O, THR, 4, 0.5, 7, 0, 3, draw=lambda c, a, b: 0.0 if c == 2 else a)
    assert g[2] == 0.75 and g[3] == 0.75 and not ok
    g, ok = RT.propose(O, THR, 4, 0.5, 7, 0, 3, draw=lambda c, a, b: b if c == 2 else 1.0)   # ... and on its upper bound: g_2 = old t_3
    assert g[2] == 1.5 and not ok
    g, ok = RT.propose(O, THR, 4, 0.5, 7, 0, 3, draw=lambda c, a, b: np.nan)                 # a NaN is out of order
    assert not ok


def test_terms_partials_and_correction(O):
    g = np.array([-INF, 0.0, 0.75, 1.25, INF])                       # only t_3 moves: classes 1 and 2 keep both thresholds
    t = RT.row_terms(O, THR, g, CLS, LIAB, RES)
    assert np.all(t[CLS <= 2] == 0.0) and not np.signbit(t[CLS <= 2]).any() and np.all(t[CLS >= 3] != 0.0)
    fit = LIAB - RES
    want = [np.log(special.ndtr(g[c] - f) - special.ndtr(g[c - 1] - f)) - np.log(special.ndtr(THR[c] - f) - special.ndtr(THR[c - 1] - f))
            for c, f in zip(CLS, fit)]
    assert np.allclose(t, want, rtol=0, atol=1e-13)
    s = np.array([2.0, 0.5, 1.0, 4.0, 1.0, 2.0, 0.25, 1.0, 8.0, 1.0])  # row scales: sd = 1 / s
    tw = RT.row_terms(O, THR, g, CLS, LIAB, RES, 1.0, s)
    k = 6
    assert abs(tw[k] - (np.log(special.ndtr((g[3] - fit[k]) * s[k]) - special.ndtr((g[2] - fit[k]) * s[k]))
                        - np.log(special.ndtr((THR[3] - fit[k]) * s[k]) - special.ndtr((THR[2] - fit[k]) * s[k])))) < 1e-13
    assert np.array_equal(RT.row_terms(O, THR, g, CLS, LIAB, RES, 1.0, np.ones(10)), t)   # scales of one: the same bits
    # the reduction tree: two workgroups for 1,500 rows, the second ragged; the order is the butterfly's, not numpy's
    rng = np.random.default_rng(1)
    v = rng.normal(size=1500)
    p = RT.partials(v)
    assert p.shape == (2,) and abs(p[0] - v[:1024].sum()) < 1e-11 and abs(p[1] - v[1024:].sum()) < 1e-11
    x = v[:64].copy()
    lvl = x
    for off in (32, 16, 8, 4, 2, 1):
        lvl = lvl[:off] + lvl[off:2 * off]
    assert RT.partials(x)[0] == lvl[0]
    w = np.zeros(1024); w[::64] = np.arange(1.0, 17.0) * 0.1           # one value per wave: the wave sums are added in index order
    acc = np.float64(0.1)
    for k in range(2, 17):
        acc = acc + np.float64(k) * 0.1
    assert RT.partials(w)[0] == acc
    corr = RT.correction(O, THR, g, 4, 0.5)
    fwd = np.log(special.ndtr((INF - 1.5) / 0.5) - special.ndtr((0.75 - 1.5) / 0.5)) + np.log(special.ndtr((1.5 - 0.75) / 0.5) - special.ndtr((0.0 - 0.75) / 0.5))
    rev = np.log(1.0 - special.ndtr((0.75 - 1.25) / 0.5)) + np.log(special.ndtr((1.25 - 0.75) / 0.5) - special.ndtr((0.0 - 0.75) / 0.5))
    assert abs(corr - (fwd - rev)) < 1e-14
    assert RT.correction(O, THR, THR, 4, 0.5) == 0.0                 # nothing moved: forward and reverse are one interval


def test_forced_accept_forced_reject_and_adaptation(O):
    draw = lambda c, a, b: -0.5 if c == 2 else 0.25                  # noqa: E731  g_2 = 0.5, g_3 = 1.625 with sigma = 0.5
    g, ok = RT.propose(O, THR, 4, 0.5, 7, 0, 3, draw)
    assert ok and g[2] == 0.5 and g[3] == 1.625
    part = RT.partials(RT.row_terms(O, THR, g, CLS, LIAB, RES))
    L = part[0] + RT.correction(O, THR, g, 4, 0.5)
    assert L < -0.01                                                 # t_2 = 0.5 cuts into class 2 (a record fitted at 0.5): a worse state
    u_acc, u_rej = np.exp(L) * 0.5, min(np.exp(L) * 1.5, 0.999)
    thr1, sg1, tr1, ac1, took = RT.step(O, THR, CLS, LIAB, RES, 4, 0.5, 10, 4, False, 7, 0, 3, draw=draw, u=u_acc)
    assert took and np.array_equal(thr1, g) and (sg1, tr1, ac1) == (0.5, 11, 5)
    thr2, sg2, tr2, ac2, took = RT.step(O, THR, CLS, LIAB, RES, 4, 0.5, 10, 4, False, 7, 0, 3, draw=draw, u=u_rej)
    assert not took and np.array_equal(thr2, THR) and (sg2, tr2, ac2) == (0.5, 11, 4)
    # a collapsed proposal is rejected whatever u is, and nothing is evaluated (no partials exist)
    thr3, sg3, tr3, ac3, took = RT.step(O, THR, CLS, LIAB, RES, 4, 0.5, 10, 4, False, 7, 0, 3, draw=lambda c, a, b: 0.0 if c == 2 else a, u=1e-300)
    assert not took and np.array_equal(thr3, THR) and (tr3, ac3) == (11, 4)
    # a NaN sum rejects
    assert not RT.decide(O, THR, g, True, np.array([np.nan]), 4, 0.5, 0, 0, False, 7, 0, 3, u=1e-300)[4]
    # the decision's own uniform: the first of stream (seed, chain, iter, 24, 1)
    u = O.draws(7, 0, 3, 24, 1, 0, 1)[0]
    assert RT.decide(O, THR, g, True, part, 4, 0.5, 0, 0, False, 7, 0, 3)[4] == (np.log(u) < L)
    # adaptation: log sigma moves by (taken - 0.44) / sqrt(tries'), and stays inside its bounds
    _, sg_a, _, _, _ = RT.step(O, THR, CLS, LIAB, RES, 4, 0.5, 15, 4, True, 7, 0, 3, draw=draw, u=u_acc)
    _, sg_r, _, _, _ = RT.step(O, THR, CLS, LIAB, RES, 4, 0.5, 15, 4, True, 7, 0, 3, draw=draw, u=u_rej)
    assert abs(sg_a - 0.5 * np.exp(0.56 / 4.0)) < 1e-15 and abs(sg_r - 0.5 * np.exp(-0.44 / 4.0)) < 1e-15
    assert RT.decide(O, THR, g, True, part, 4, 1.0, 0, 0, True, 7, 0, 3, u=u_acc)[1] == 1.0            # log sigma <= 0
    assert abs(RT.decide(O, THR, g, False, None, 4, np.exp(-20.0), 0, 0, True, 7, 0, 3)[1] - np.exp(-20.0)) < 1e-22
    assert RT.sigma_start(400) == 0.05 and RT.sigma_start(50) == 1.0 / np.sqrt(50.0)


def test_class_probabilities_of_the_restatement(O):
    fit = np.array([-2.0, 0.1, 0.8, 1.6, 45.0])
    p = RT.class_probs(O, THR, 4, fit)
    assert np.all(np.abs(p.sum(axis=1) - 1.0) < 1e-12) and np.all(p >= 0.0)
    want = special.ndtr(THR[None, 1:] - fit[:, None]) - special.ndtr(THR[None, :-1] - fit[:, None])
    assert np.allclose(p[:4], want[:4], rtol=0, atol=1e-15)
    assert p[4].tolist() == [0.0, 0.0, 0.0, 1.0]                     # an interval without mass is 0, not NaN
    assert np.array_equal(RT.class_probs(O, THR, 4, fit, 1.0, np.ones(5)), p)


def test_class_metrics_against_a_direct_computation(ngp):
    rng = np.random.default_rng(5)
    for C_ in (2, 3, 5):
        n = 200
        p = rng.dirichlet(np.ones(C_), size=n)
        p[:20] = np.round(p[:20], 1); p[:20] /= np.maximum(p[:20].sum(axis=1, keepdims=True), 1e-9)   # ties among the scores
        obs = rng.integers(1, C_ + 1, size=n)
        got, want = ngp.class_metrics(p, obs), RT.cv_metrics(p, obs, C_)
        assert got["n"] == n and set(got) - {"n"} == set(want)
        for k in want:
            assert abs(got[k] - want[k]) < 1e-12, (C_, k)
    perfect = np.eye(3)[[0, 1, 2, 1]]
    m = ngp.class_metrics(perfect, [1, 2, 3, 2])
    assert m["brier"] == 0.0 and m["logloss"] == 0.0 and m["class_accuracy"] == 1.0 and "auc" not in m
    m = ngp.class_metrics(np.array([[0.9, 0.1], [0.2, 0.8], [0.6, 0.4], [0.6, 0.4]]), [1, 2, 2, 1])
    assert m["auc"] == (2 + 1.5) / 4 and m["class_accuracy"] == 0.75 and abs(m["brier"] - (0.02 + 0.08 + 0.72 + 0.32) / 4) < 1e-15
    assert np.isfinite(ngp.class_metrics(np.array([[1.0, 0.0]]), [2])["logloss"]) and np.isnan(ngp.class_metrics(np.array([[1.0, 0.0]]), [2])["auc"])
    freq = np.tile([0.5, 0.3, 0.2], (10, 1))                            # the class-frequency predictor's Brier score is 1 - sum f^2
    assert abs(ngp.class_metrics(freq, [1] * 5 + [2] * 3 + [3] * 2)["brier"] - (1 - 0.38)) < 1e-15


def test_runlmem_arguments_are_checked_before_any_device_work(ngp, tmp_path):
    rng = np.random.default_rng(3)
    N = 30
    A = rng.integers(0, 3, size=(N, 20)).astype(np.uint8)
    np.save(tmp_path / "a.npy", A)
    f = f'y ~ 1 + SNP(M1,"{tmp_path / "a.npy"}")'
    y2 = (rng.normal(size=N) > 0).astype(np.float64)
    y3 = np.arange(N) % 3.0
    k = [0]

    def run(y, **kw):
        k[0] += 1
        return ngp.runLMEM(f, {"y": y}, 4, 2, 1, outFolder=str(tmp_path / f"o{k[0]}"), **kw)

    with pytest.raises(ValueError, match="thresholdStep"):
        run(y3, trait="categorical", thresholdStep="metropolis")
    with pytest.raises(ValueError, match="thresholdStep"):
        run(rng.normal(size=N), thresholdStep="cowles")
    with pytest.raises(ValueError, match="classProb"):
        run(rng.normal(size=N), classProb=True, folds=2)
    with pytest.raises(ValueError, match="two classes"):
        run(y2, trait="categorical", thresholdStep="cowles")
    with pytest.raises(ValueError, match="classProb"):
        run(y3, trait="categorical", classProb=True)                  # no held-out record to report on
    with pytest.raises(ValueError, match="classProb"):
        run(y3, trait="categorical", classProb="yes", folds=2)
    assert not any((tmp_path / f"o{i}").exists() for i in range(1, k[0] + 1))


def test_layout_tails_and_the_guards_of_the_new_segments():
    txt = open(os.path.join(CSRC, "ngp_state.h")).read()
    assert "inline const Layout ordered_posterior_tail = {{SEG_SUM_PROB}};" in txt
    assert "inline const Layout ordered_snapshot_tail = {{SEG_THR_STEP}, {SEG_SUM_PROB}};" in txt
    assert "for (const Layout *part : {&L, tail, ordered_tail_of(L)})" in txt
    api = open(os.path.join(CSRC, "ngp_api.hip")).read()
    body = api[api.index("void describe(ngp_handle *h, ChainState &st) {"):api.index("static_assert(offsetof(DSet, piHat1)")]
    assert "if (lb.ts_mode == 1) st.dev(SEG_THR_STEP," in body and "if (lb.d_sum_prob) st.dev(SEG_SUM_PROB," in body
    assert api.count("SEG_THR_STEP") == 1 and api.count("SEG_SUM_PROB") == 1
    it = api[api.index("void iteration_pre("):api.index("int iteration_post(")]
    assert it.index("if (!resume_mid) {") < it.index("k_threshold_terms") < it.index("k_threshold_decide") < it.index("k_liability_augment")
    assert "lb.ts_adapt && h->iter + 1 <= h->burnIn" in it
    post = api[api.index("int iteration_post("):api.index("int one_iteration(")]
    assert post.index("k_holdout_accum") < post.index("k_holdout_prob") and post.index("if (do_accum) {") < post.index("k_holdout_prob")
    assert "if (w == 0) return digest;" in api                       # mode 0 without probabilities: the digest of every earlier snapshot


def test_julia_binds_the_new_entry_points():
    decl = c_declarations()
    calls = {name: (ret, types, vals) for name, ret, types, vals in julia_ccalls()}
    for s in NEW:
        if s.startswith("ngp_debug_"):
            continue
        assert s in calls, s
        ret, types, vals = calls[s]
        assert ret == "Int32" and len(types) == len(decl[s]) == len(vals)
        assert all(jt in C2J[ct] for jt, ct in zip(types, decl[s])), s
