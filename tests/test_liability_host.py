"""Liability traits, the parts that need no device: the symbols and stream kinds, the restatement of the truncated normal against
scipy's law on every branch, the start values, the threshold step, the mirror's argument checks, the layout tails and the Julia bindings."""
import os
import re

import numpy as np
import pytest
from scipy import stats

import pivot_models as PM
import ref_liability as RL
from test_julia_shim_static import C2J, c_declarations, julia_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nextgp.jl_amd", "csrc")
NEW = ["ngp_set_liability_classes", "ngp_set_liability_bounds", "ngp_get_liability_layout", "ngp_get_liability", "ngp_set_liability_state",
       "ngp_get_liability_stats", "ngp_fix_residual_variance", "ngp_tnormal_indexed"]
INF = np.inf
# every branch of the sampler: normal rejection, tail at 0, far tail, mirrored tail, uniform proposal beside a, exponential proposal with
# an upper bound, uniform proposal across 0, normal rejection across 0
BOUNDS = [(-1.0, INF), (0.0, INF), (7.0, INF), (-INF, -3.0), (2.0, 2.01), (5.0, 9.0), (-0.5, 0.7), (-3.0, 4.0)]


def test_symbols_stream_kinds_and_abi_version(ngp):
    hdr = open(os.path.join(ROOT, "include", "nextgp_hip.h")).read()
    assert "#define NGP_ABI_VERSION 4" in hdr
    decl = c_declarations()
    for s in NEW:
        assert s in ngp.SYMBOLS and s in decl, s
    assert decl["ngp_set_liability_classes"] == ["ngp_handle*", "int32_t*", "int32_t"]
    assert decl["ngp_set_liability_bounds"] == ["ngp_handle*", "int64_t*", "double*", "double*", "int64_t"]
    assert decl["ngp_fix_residual_variance"] == ["ngp_handle*", "double"]
    assert decl["ngp_tnormal_indexed"] == ["ngp_handle*", "uint64_t", "uint64_t", "uint64_t", "double*", "double*", "int64_t", "double*"]
    src = open(os.path.join(CSRC, "ngp_api.hip")).read()
    for s in NEW:                                                   # every entry point behind the exception barrier
        assert re.search(r"\nint32_t " + s + r"\([^)]*\) \{\n    NGP_TRY\n", src), s
    rng_h = open(os.path.join(CSRC, "ngp_rng.h")).read()
    assert re.search(r"^#define NGP_KIND_LIABILITY 22\b", rng_h, flags=re.M) and re.search(r"^#define NGP_KIND_THRESHOLD 23\b", rng_h, flags=re.M)
    assert RL.KIND_LIABILITY == 22 and RL.KIND_THRESHOLD == 23
    k = open(os.path.join(CSRC, "ngp_liability.h")).read()
    for name in ("rng_tnormal", "k_tnormal_indexed", "k_thresholds", "k_liability_augment", "NGP_KIND_LIABILITY", "NGP_KIND_THRESHOLD"):
        assert name in k, name
    assert "#define NGP_TN_ROUNDS 256" in k and RL.ROUNDS == 256     # every loop is bounded
    code = re.sub(r"//[^\n]*", "", k)
    assert "asm" not in code and "while" not in code and "for (;;)" not in code
    for unit in ("ngp_sweep.h", "ngp_sweep_inst.hip", "ngp_sweep_body.inc", "ngp_sweep_multi_body.inc"):   # the sweep units do not know it
        assert "liab" not in open(os.path.join(CSRC, unit)).read()


@pytest.mark.parametrize("a,b", BOUNDS)
def test_truncated_normal_follows_its_law_on_every_branch(O, a, b):
    """1,500 draws of keyed streams per interval against scipy's truncnorm; every draw lies inside, none falls through."""
    n = 1500
    z = np.empty(n)
    for i in range(n):
        z[i], fell = RL.tnormal_stream(O, 77, 0, 3, RL.KIND_LIABILITY, i, a, b)
        assert not fell
    assert np.all(z > a) and np.all(z < b)
    p = float(stats.kstest(z, stats.truncnorm(a, b).cdf).pvalue)
    print(f"({a}, {b}): KS p = {p:.4f}")
    assert p > PM.KS_MIN, p


def test_branches_are_the_ones_the_bounds_were_chosen_for(O):
    """The switch point of 0 <= a < b in the written operation order; (2, 2.01) takes the uniform proposal, (5, 9) the exponential one."""
    for a in (0.0, 2.0, 5.0):
        lim, aa = RL.switch_point(O, np.float64(a))
        want = a + 2.0 * np.sqrt(np.e) / (a + np.sqrt(a * a + 4.0)) * np.exp((a * a - a * np.sqrt(a * a + 4.0)) / 4.0)
        assert abs(lim - want) < 1e-14 and aa == a * a
    assert 2.01 <= RL.switch_point(O, np.float64(2.0))[0] and 9.0 > RL.switch_point(O, np.float64(5.0))[0]
    assert 0.7 - -0.5 <= RL.SQRT_2PI < 4.0 - -3.0
    assert RL.SQRT_2PI == np.sqrt(2.0 * np.pi) and RL.TWO_SQRT_E == 2.0 * np.sqrt(np.e)
    # a uniform stream is consumed in order: one uniform per round of a rejection from the normal, two per round of a proposal
    u = RL.Uniforms(O, 5, 0, 1, 22, 9)
    z, _ = RL.tnormal(O, u, -1.0, INF)
    first = O.draws(5, 0, 1, 22, 9, 0, 8)
    k = next(i for i in range(8) if O.ppnd16(first[i]) > -1.0)
    assert z == O.ppnd16(first[k]) and u.k == k + 1
    u = RL.Uniforms(O, 5, 0, 1, 22, 9)
    RL.tnormal(O, u, 2.0, 2.01)
    assert u.k % 2 == 0 and u.k >= 2


def test_bounds_that_cannot_be_sampled_fall_through_and_never_loop(O):
    u = RL.FromGenerator(np.random.default_rng(1))
    for a, b, want in ((np.nan, 1.0, 1.0), (0.0, np.nan, 0.0), (np.nan, np.nan, 0.0), (2.0, 2.0, 2.0), (3.0, 1.0, 2.0), (INF, INF, 0.0), (-INF, -INF, 0.0)):
        z, fell = RL.tnormal(O, u, a, b)
        assert fell and z == want, (a, b, z)
    assert u.rng.random() == np.random.default_rng(1).random()       # ... without taking a uniform


def test_start_values(O):
    cls = np.array([1, 3, 2, 2, 4, 1, 2, 3, 3, 3])
    thr, liab = RL.start_classes(O, cls, 4)
    q = [O.ppnd16(0.2), O.ppnd16(0.5), O.ppnd16(0.9)]
    assert thr[0] == -INF and thr[1] == 0.0 and thr[4] == INF and thr[2] == q[1] - q[0] and thr[3] == q[2] - q[0]
    assert liab[0] == -0.5 and liab[4] == thr[3] + 0.5 and liab[2] == (0.0 + thr[2]) / 2.0 and liab[1] == (thr[2] + thr[3]) / 2.0
    for c in range(1, 5):
        assert np.all((liab[cls == c] > thr[c - 1]) & (liab[cls == c] <= thr[c]))
    thr2, liab2 = RL.start_classes(O, np.array([1, 2, 2]), 2)        # binary: one threshold, at 0
    assert np.array_equal(thr2, [-INF, 0.0, INF]) and np.array_equal(liab2, [-0.5, 0.5, 0.5])
    assert np.array_equal(RL.start_bounds([1.0, -INF, -2.0], [INF, 3.0, 4.0]), [1.0, 3.0, 1.0])


def test_threshold_step(O):
    cls = np.array([1, 2, 2, 3, 3, 4])
    liab = np.array([-1.0, 0.2, 0.6, 0.9, 1.4, 2.5])
    thr = np.array([-INF, 0.0, 0.7, 2.0, INF])
    new = RL.thresholds(O, thr, cls, liab, 4, 9, 1, 5)
    u2, u3 = O.draws(9, 1, 5, 23, 2, 0, 1)[0], O.draws(9, 1, 5, 23, 3, 0, 1)[0]
    t2 = 0.6 + u2 * (0.9 - 0.6)                                    # between the largest of class 2 and the smallest of class 3
    t3 = 1.4 + u3 * (2.0 - 1.4)                                    # the old t_4 side is open: min(inf, 2.5) ... but t_3 <= min of class 4
    assert new[2] == t2 and np.array_equal(new[[0, 1, 4]], thr[[0, 1, 4]])
    assert new[3] == 1.4 + u3 * (2.5 - 1.4) and t3 < new[3]
    assert np.array_equal(thr, [-INF, 0.0, 0.7, 2.0, INF])           # (the argument is not changed)
    # the new t_{c-1} bounds t_c from below when no liability of class c lies above it
    liab_b = np.array([-1.0, 0.2, 0.6, 0.61, 0.62, 2.5])
    nb = RL.thresholds(O, thr, cls, liab_b, 4, 9, 1, 5)
    assert nb[3] == max(nb[2], 0.62) + u3 * (2.5 - max(nb[2], 0.62))


def test_augmentation_step_keeps_every_liability_in_its_interval(O):
    rows = np.array([0, 3, 4, 9])
    liab = np.array([0.5, -0.5, 2.0, 1.0])
    r = np.array([0.3, -0.1, 0.4, 0.2])
    lo = np.array([0.0, -INF, 1.5, 1.0]); hi = np.array([INF, 0.0, 2.5, INF])
    same, e, ep, fell = RL.step(O, rows, liab, r, 0.0, lo, hi, 3, 0, 1)
    assert np.array_equal(same, liab) and e is None and ep is None and fell == 0      # varE == 0: nothing is touched
    new, e, ep, fell = RL.step(O, rows, liab, r, 2.25, lo, hi, 3, 0, 2)
    assert fell == 0 and ep is not None and np.array_equal(e, ep) and np.all(new >= lo) and np.all(new <= hi)
    assert np.array_equal(new, (liab - r) + e)
    z0, _ = RL.tnormal_stream(O, 3, 0, 2, 22, 9, (1.0 - (1.0 - 0.2)) / 1.5, INF)     # keyed by the row (9), not by its place (3)
    assert e[3] == 1.5 * z0
    s = np.array([2.0, 0.5, 1.0, 4.0])
    new_w, e_w, ep_w, _ = RL.step(O, rows, liab, r, 2.25, lo, hi, 3, 0, 2, s_A=s)
    assert np.array_equal(ep_w, e_w / s) and np.array_equal(new_w, (liab - r) + ep_w) and e_w[2] == e[2]
    ones, e1, ep1, _ = RL.step(O, rows, liab, r, 2.25, lo, hi, 3, 0, 2, s_A=np.ones(4))
    assert np.array_equal(ones, new) and np.array_equal(e1, e)                        # weights of one: the same bits


def test_mirror_argument_checks(ngp):
    """Every bad class vector or bound list is a ValueError from host checks -- this test runs where there is no device."""
    c = ngp.check_classes([1, 2, 2, 3], 4)
    assert c.dtype == np.int32 and c.tolist() == [1, 2, 2, 3]
    for bad, kw in (([1, 2, 3], {}), ([1.5, 2, 2, 1], {}), ([1, 1, 1, 1], {}), ([1, 2, 3, 9], {}), ([1, 2, 2, 1], dict(C_=9))):
        with pytest.raises(ValueError, match="classes"):
            ngp.check_classes(bad, 4, **kw)
    codes, vals = ngp.class_codes([0.0, 2.0, np.nan, 1.0, 2.0])
    assert codes.tolist() == [1, 3, 0, 2, 3] and vals.tolist() == [0.0, 1.0, 2.0]
    for bad in ([1.0, 1.0, np.nan], list(range(9))):
        with pytest.raises(ValueError, match="categorical"):
            ngp.class_codes(bad)
    r, lo, hi = ngp.check_bounds([0, 3], [1.0, -INF], [INF, 2.0], 5)
    assert r.dtype == np.int64 and lo.tolist() == [1.0, -INF] and hi.tolist() == [INF, 2.0]
    for rows, lo, hi in (([3, 0], [0.0, 0.0], [1.0, 1.0]), ([0, 5], [0.0, 0.0], [1.0, 1.0]), ([0], [1.0], [1.0]), ([0], [-INF], [INF]), ([], [], []),
                         ([0, 1], [0.0], [1.0])):
        with pytest.raises(ValueError, match="censored"):
            ngp.check_bounds(rows, lo, hi, 5)
    rows, lo, hi = ngp.censored_bounds([1.0, 2.0, np.nan, 0.5, -INF], [1.0, np.nan, 3.0, 0.7, 4.0])
    assert rows.tolist() == [1, 2, 3, 4] and lo.tolist() == [2.0, -INF, 0.5, -INF] and hi.tolist() == [INF, 3.0, 0.7, 4.0]
    for lower, upper in (([2.0], [1.0]), ([np.nan], [np.nan]), ([1.0, 2.0], [1.0])):
        with pytest.raises(ValueError, match="censored"):
            ngp.censored_bounds(lower, upper)


def test_layout_tails_and_the_guard_of_the_new_segments():
    """The three tables are untouched (tests/test_holdout_host.py pins them); liabilities follow two of them as tails, described in one
    place under the condition that the chain has liabilities, so that a chain without them is written byte for byte as before."""
    txt = open(os.path.join(CSRC, "ngp_state.h")).read()
    assert re.search(r"inline const Layout liability_posterior_tail = \{\{SEG_SUM_THR\}, \{SEG_SUM_THR2\}\};", txt)
    assert re.search(r"inline const Layout liability_snapshot_tail = \{\{SEG_LIAB, SEG_THR, SEG_SUM_THR, SEG_SUM_THR2\}\};", txt)
    assert re.search(r"inline const Layout liability_sample_tail = \{\{SEG_THR_SMP\}\};", txt)
    assert "&L == &posterior_layout ? &liability_posterior_tail : &L == &snapshot_body_layout ? &liability_snapshot_tail" in txt
    assert "&L == &sample_layout ? &liability_sample_tail : nullptr" in txt
    api = open(os.path.join(CSRC, "ngp_api.hip")).read()
    body = api[api.index("void describe(ngp_handle *h, ChainState &st) {"):api.index("static_assert(offsetof(DSet, piHat1)")]
    guard = body.index("if (h->cm.lb.on()) {")
    for seg in ("SEG_LIAB", "SEG_THR", "SEG_SUM_THR", "SEG_SUM_THR2"):
        assert body.count(seg + ",") == 1 and body.index(seg + ",") > guard, seg
    assert api.count("SEG_LIAB") == 1
    assert "h->fix_varE > 0.0 ? 0 : 1" in api                       # k_head's draw_varE argument
    it = api[api.index("void iteration_pre("):api.index("int iteration_post(")]
    assert it.index("k_thresholds") < it.index("k_liability_augment") < it.index("k_holdout_augment") < it.index("k_head")
    assert it.index("if (!resume_mid) {") < it.index("k_thresholds")  # a sweep launched again after its census does not augment twice


def test_julia_binds_the_liability_entry_points():
    decl = c_declarations()
    calls = {name: (ret, types, vals) for name, ret, types, vals in julia_ccalls()}
    for s in NEW:
        assert s in calls, s
        ret, types, vals = calls[s]
        assert ret == "Int32" and len(types) == len(decl[s]) == len(vals)
        assert all(jt in C2J[ct] for jt, ct in zip(types, decl[s])), s


def test_autocorrelation_time_of_the_restatement():
    rng = np.random.default_rng(4)
    x = rng.normal(size=20000)
    assert abs(RL.autocorrelation_time(x) - 1.0) < 0.2
    y = np.empty(20000); y[0] = 0.0
    for i in range(1, 20000):
        y[i] = 0.8 * y[i - 1] + x[i]
    assert abs(RL.autocorrelation_time(y) - 9.0) < 2.5              # AR(1), f = 0.8: (1 + f) / (1 - f) = 9


def test_runlmem_liability_arguments_are_checked_before_any_device_work(ngp, tmp_path):
    """Every keyword clash and every bad response is a ValueError from host checks -- this test runs where there is no device."""
    rng = np.random.default_rng(3)
    N = 30
    A = rng.integers(0, 3, size=(N, 20)).astype(np.uint8)
    np.save(tmp_path / "a.npy", A)
    f = f'y ~ 1 + SNP(M1,"{tmp_path / "a.npy"}")'
    yb = (rng.normal(size=N) > 0).astype(np.float64)
    k = [0]

    def run(y=yb, **kw):
        k[0] += 1
        return ngp.runLMEM(f, {"y": y, "lo": np.zeros(N), "hi": np.ones(N)}, 4, 2, 1, outFolder=str(tmp_path / f"o{k[0]}"), **kw)

    with pytest.raises(ValueError, match="trait"):
        run(trait="poisson")
    with pytest.raises(ValueError, match="value 1"):
        run(trait="categorical", VCV={"e": ngp.Random("I", 2.0)})
    with pytest.raises(ValueError, match="distinct values"):
        run(y=rng.normal(size=N), trait="categorical")
    with pytest.raises(ValueError, match="distinct values"):
        run(y=np.ones(N), trait="categorical")
    ym = yb.copy(); ym[4] = np.nan
    with pytest.raises(ValueError, match="no response"):
        run(y=ym, trait="categorical")
    with pytest.raises(ValueError, match="not both"):
        run(trait="categorical", censored={"lower": "lo", "upper": "hi"})
    with pytest.raises(ValueError, match="censored"):
        run(censored={"lower": "lo"})
    with pytest.raises(ValueError, match="censored"):
        run(censored={"lower": "hi", "upper": "lo"})                       # lower > upper
    with pytest.raises(ValueError, match="no record is censored"):
        run(censored={"lower": "lo", "upper": "lo"})
    with pytest.raises(ValueError, match="one entry per record"):
        run(censored={"lower": np.zeros(3), "upper": np.ones(3)})
    with pytest.raises(ValueError, match="held out as well"):
        run(censored={"lower": "lo", "upper": "hi"}, holdout=[2])
