"""Liability traits on the device (include/nextgp_hip.h, "liability traits"; DESIGN.md section 2, "Liability traits"): binary and ordered
classes and censored records by data augmentation, ycorr_i <- e_i with e from a truncated normal.  The reference has nothing of this kind;
what is checked here is the arithmetic DESIGN.md fixes, restated in tests/ref_liability.py: the draw layer bit for bit, the augmented
chain IS the ordinary chain on the augmented data bit for bit, the threshold step, the laws of three intercept-only models against
quadrature, and the formats."""
import ctypes as C
import os

import numpy as np
import pytest

import ref_liability as RL
from conftest import add_sets
from test_gpu_compact import make_codes
from test_liability_host import BOUNDS

pytestmark = pytest.mark.gpu

INF = np.inf
SCHED = (12, 4, 2)                        # kept: 6, 8, 10, 12
SEED = 1001


def same_state(a, b):
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def set_ycorr(s, ycorr, st):
    """ngp_set_state with the residual alone (every other array NULL: they stay as they are)."""
    yc = np.ascontiguousarray(ycorr, dtype=np.float64)
    s._chk(s.L.ngp_set_state(s.h, yc.ctypes.data_as(C.POINTER(C.c_double)), None, None, None, None, C.c_double(st["varE"]), C.c_double(st["b"]),
                             C.c_int64(st["iter"])))


def full_state(s):
    st = s.get_state()
    st["fixed"] = s.get_fixed()["b"]
    st["class_pi"] = s.get_class_state(0)["piHat"]
    return st


def thr_full(ls, C_):
    """thr[0 .. C] with the infinite ends from the C - 1 thresholds the ABI reports."""
    return np.concatenate([[-INF], ls["thr"], [INF]]) if C_ >= 2 else None


def test_draw_layer_bit_for_bit(ngp, O):
    """64 draws of every interval of the host test's list in one launch (8 x 64 = 512 lanes: two workgroups), streams (seed, chain, 4, 22,
    100 + i): equal to the restatement bit for bit, the fall-through counter stays 0; bounds that cannot be sampled (NaN, a >= b) return
    at once, count, and hang nothing."""
    s = ngp.Sampler(device=0, seed=SEED, chain=3)
    a = np.repeat([p[0] for p in BOUNDS], 64); b = np.repeat([p[1] for p in BOUNDS], 64)
    z = s.tnormal_indexed(4, RL.KIND_LIABILITY, 100, a, b)
    want = np.array([RL.tnormal_stream(O, SEED, 3, 4, RL.KIND_LIABILITY, 100 + i, a[i], b[i])[0] for i in range(len(a))])
    assert np.array_equal(z, want)
    assert np.all(z > a) and np.all(z < b) and s.liability_fallthrough() == 0
    bad_a = np.array([np.nan, 0.0, 2.0, 3.0, INF]); bad_b = np.array([1.0, np.nan, 2.0, 1.0, INF])
    zb = s.tnormal_indexed(4, RL.KIND_LIABILITY, 0, bad_a, bad_b)
    assert np.array_equal(zb, [1.0, 0.0, 2.0, 2.0, 0.0]) and s.liability_fallthrough() == 5


# ---- the augmented chain is the ordinary chain on the augmented data ----
# N = 700, P = 128 (two 64-SNP blocks), 600 augmented rows: three workgroups of the kernel.  The weights are powers of four, so that the row
# scales are powers of two and scaling a residual and unscaling it again changes no bit (the comparison chain is driven through
# ngp_get_state / ngp_set_state, which unscale and scale).
CASES = {
    "classes_fp32": dict(kind="classes"),
    "classes_u8": dict(kind="classes", storage="u8"),
    "classes_weights_of_one": dict(kind="classes", weights="ones"),
    "bounds_fp32": dict(kind="bounds"),
    "bounds_u8": dict(kind="bounds", storage="u8"),
    "bounds_weights": dict(kind="bounds", weights="real"),
}


def problem(O, N=700, P=128, m=600):
    G, y, v = make_codes(O, N, P)
    rng = np.random.default_rng(N + P)
    A = np.sort(np.concatenate([[0, N - 1], rng.choice(np.arange(1, N - 1), size=m - 2, replace=False)])).astype(np.int64)
    Xf = rng.normal(size=(N, 2))
    return G, y, v, A, Xf


def base(ngp, G, v, Xf, w=None, storage=None, chain_id=0, owner=None, shards=0):
    s = ngp.Sampler(device=0, seed=SEED, chain=chain_id, storage=storage)
    if owner is not None:
        s.share_panel(owner)
    else:
        if w is not None:
            s.set_residual_weights(w)
        if shards:
            s.set_max_shards(shards)
        s.set_panel(G, centre=True)
    add_sets(s, [(0, G.shape[1], "R")], v)
    s.add_fixed_set(Xf)
    return s


def censoring(y, A):
    """Bounds of the rows A around y: a third right-censored below y, a third left-censored, a third in an interval."""
    k = np.arange(len(A)) % 3
    sd = y.std()
    lo = np.where(k == 0, y[A] - 0.3 * sd, np.where(k == 1, -INF, y[A] - 0.2 * sd))
    hi = np.where(k == 0, INF, np.where(k == 1, y[A] + 0.3 * sd, y[A] + 0.4 * sd))
    return lo, hi


@pytest.mark.parametrize("case", list(CASES))
def test_augmented_chain_is_the_ordinary_chain_on_the_augmented_data(ngp, O, case):
    """Handle A carries the liabilities, handle B none (classes: ngp_fix_residual_variance(1); bounds: varE sampled).  Before every
    iteration B's residual of the augmented rows is replaced from outside by what the restatement draws (kind 22 keyed by the ROW, thresholds
    of kind 23 first); then both run one iteration.  Every part of the state agrees bit for bit after every step, liab and thr follow the
    restatement, and weights of one give the bits of the unweighted chain."""
    c = CASES[case]
    G, y, v, A, Xf = problem(O)
    N = len(y)
    w = None if "weights" not in c else (np.ones(N) if c["weights"] == "ones" else np.random.default_rng(5).choice([0.25, 1.0, 4.0, 16.0], size=N))
    s_A = None if w is None else np.sqrt(w[A])
    a = base(ngp, G, v, Xf, w=w, storage=c.get("storage")); b = base(ngp, G, v, Xf, w=w, storage=c.get("storage"))
    if c["kind"] == "classes":
        C_ = 3
        cls = (1 + (y > np.quantile(y, 0.3)) + (y > np.quantile(y, 0.8))).astype(np.int32)
        H = np.setdiff1d(np.arange(N), A)
        a.set_holdout(H); b.set_holdout(H)                               # the other 100 rows are held out: A is what is left
        garbage = cls.copy(); garbage[H] = -77
        a.set_classes(garbage, C_)
        thr, liab = RL.start_classes(O, cls[A], C_)
        y0 = np.zeros(N); y0[A] = liab; y0[H] = np.nan
        b.fix_residual_variance(1.0)
        a.set_y(np.full(N, np.nan)); b.set_y(y0)                         # y is read at no row of a
        assert a.liability_layout() == (600, 3)
    else:
        C_, cls = 0, None
        lo, hi = censoring(y, A)
        a.set_censored(A, lo, hi)
        liab = RL.start_bounds(lo, hi)
        y0 = y.copy(); y0[A] = liab
        ya = y.copy(); ya[A] = np.nan                                     # y is read off the censored rows only
        a.set_y(ya); b.set_y(y0)
        assert a.liability_layout() == (600, 0)
    for s in (a, b):
        s.set_residual_prior(4.0, 0.25 * float(y.var())); s.set_schedule(*SCHED)
    ls = a.liability_state()
    assert np.array_equal(ls["rows"], A) and np.array_equal(ls["liab"], liab)
    if C_:
        assert np.array_equal(thr_full(ls, C_), thr)
    drew = 0
    for t in range(1, 7):
        stA, stB = full_state(a), full_state(b)
        same_state(stA, stB)
        if C_:
            assert stA["varE"] == 1.0
            thr = RL.thresholds(O, thr, cls[A], liab, C_, SEED, 0, t)
            lo, hi = thr[cls[A] - 1], thr[cls[A]]
        liab, e, ep, fell = RL.step(O, A, liab, stB["ycorr"][A], stB["varE"], lo, hi, SEED, 0, t, s_A)
        assert fell == 0
        if e is not None:
            yc = stB["ycorr"].copy(); yc[A] = ep
            set_ycorr(b, yc, stB)
            drew += 1
        else:
            assert t == 1 and not C_                                      # a fresh censored chain: varE == 0, nothing is touched
        a.run(1); b.run(1)
        ls = a.liability_state()
        assert np.array_equal(ls["liab"], liab), t
        if C_:
            assert np.array_equal(thr_full(ls, C_), thr), t
    same_state(full_state(a), full_state(b))
    assert drew == (6 if C_ else 5) and np.all(liab >= lo) and np.all(liab <= hi) and a.liability_fallthrough() == 0
    if c.get("weights") == "ones":                                       # the same bits as without weights
        u = base(ngp, G, v, Xf)
        u.set_holdout(H); u.set_classes(cls, C_); u.set_y(np.zeros(N)); u.set_residual_prior(4.0, 0.25 * float(y.var())); u.set_schedule(*SCHED)
        u.run(6)
        same_state(full_state(u), full_state(a)); same_state(u.liability_state(), a.liability_state())


@pytest.mark.parametrize("N", [40, 1500])
def test_thresholds(ngp, O, N):
    """C = 4, intercept only, N = 40 (less than a wave) and 1,500 (more than the workgroup's 1,024 lanes): thr after every iteration is the
    restatement's step from the liabilities before it, and the sums over kept iterations are what Python adds up."""
    rng = np.random.default_rng(N)
    cls = rng.integers(1, 5, size=N).astype(np.int32)
    s = ngp.Sampler(device=0, seed=SEED, chain=2)
    s.set_records(N)
    s.set_classes(cls)
    s.set_y(np.zeros(N)); s.set_schedule(*SCHED)
    assert s.liability_layout() == (N, 4)
    thr, liab = RL.start_classes(O, cls, 4)
    s1 = np.zeros(3); s2 = np.zeros(3)
    for t in range(1, SCHED[0] + 1):
        ls = s.liability_state()
        assert np.array_equal(ls["liab"], liab) or t > 1
        thr = RL.thresholds(O, thr_full(ls, 4), cls, ls["liab"], 4, SEED, 2, t)
        s.run(1)
        got = s.liability_state()
        assert np.array_equal(thr_full(got, 4), thr), t
        assert thr[1] == 0.0 and thr[1] < thr[2] < thr[3]
        for c in range(1, 5):
            assert np.all((got["liab"][cls == c] >= thr[c - 1]) & (got["liab"][cls == c] <= thr[c]))
        if t >= 6 and t % 2 == 0:
            s1[1:] = s1[1:] + thr[2:4]; s2[1:] = s2[1:] + thr[2:4] * thr[2:4]
    assert np.array_equal(got["sum_thr"], s1) and np.array_equal(got["sum_thr2"], s2) and s1[0] == 0.0
    assert s.get_posterior_sums()["nKept"] == 4 and np.all(s.get_trace(1)["varE"] == 1.0) and s.liability_fallthrough() == 0


def test_two_classes_have_one_threshold_at_zero(ngp, O):
    N = 70
    cls = (1 + (np.arange(N) % 3 == 0)).astype(np.int32)
    s = ngp.Sampler(device=0, seed=SEED, chain=0)
    s.set_records(N)
    s.set_classes(cls)
    s.set_y(np.zeros(N)); s.set_schedule(*SCHED)
    assert s.liability_layout() == (N, 2)
    s.run(12)
    ls = s.liability_state()
    assert np.array_equal(ls["thr"], [0.0]) and np.array_equal(ls["sum_thr"], [0.0]) and np.array_equal(ls["sum_thr2"], [0.0])
    assert np.all(ls["liab"][cls == 1] <= 0.0) and np.all(ls["liab"][cls == 2] >= 0.0)
    plain = ngp.Sampler(device=0, seed=SEED, chain=0)
    plain.set_records(N)
    assert s.posterior_len() == plain.posterior_len() + 2              # sum_thr[1] | sum_thr2[1] behind everything a chain had


# ---- the laws of three intercept-only models against quadrature ----
def law_bound(sd, tau, n_kept):
    return 6.0 * sd * np.sqrt(tau / n_kept)


# integrated autocorrelation times of the restatement's chains (ref_liability.simulate_*, numpy's generator, 20,000 kept draws each)
TAU = dict(binary_b=2.2, ordinal_b=16.4, ordinal_t2=53.7, censored_b=1.2, censored_varE=2.1)


def run_law(ngp, L, setup, y):
    s = ngp.Sampler(device=0, seed=L["seed"], chain=0)
    s.set_records(len(y))
    setup(s)
    s.set_y(y)
    if "e_df" in L:
        s.set_residual_prior(L["e_df"], L["e_scale"])
    n = L["burn"] + L["kept"]
    s.set_schedule(n, L["burn"], 1)
    s.run(n)
    ps = s.get_posterior_sums()
    assert ps["nKept"] == L["kept"] and s.liability_fallthrough() == 0
    return s, ps


def test_law_binary(ngp):
    """N = 60, intercept only: the mean of b over 4,000 kept draws against the posterior mean of Phi(b)^n1 (1 - Phi(b))^n0 by quadrature,
    within 6 posterior SDs sqrt(tau / nKept).  tau = 2.2, measured on ref_liability.simulate_classes (numpy's generator)."""
    L = RL.law_binary()
    s, ps = run_law(ngp, L, lambda s: s.set_classes(L["cls"]), np.zeros(60))
    mean, sd = RL.posterior_binary(L["cls"])
    got, tol = ps["sum_b"] / ps["nKept"], law_bound(sd, TAU["binary_b"], L["kept"])
    print("binary: mean b", got, "quadrature", mean, "sd", sd, "tol", tol)
    assert abs(got - mean) <= tol and ps["sum_varE"] == L["kept"]


def test_law_three_classes(ngp):
    """C = 3, N = 60: the means of (b, t_2) against 2-D quadrature; tau = 16.4 and 53.7 (simulate_classes)."""
    L = RL.law_ordinal()
    s, ps = run_law(ngp, L, lambda s: s.set_classes(L["cls"]), np.zeros(60))
    (mb, sb), (mt, st_) = RL.posterior_ordinal(L["cls"])
    ls = s.liability_state()
    got_b, got_t = ps["sum_b"] / ps["nKept"], ls["sum_thr"][1] / ps["nKept"]
    tb, tt = law_bound(sb, TAU["ordinal_b"], L["kept"]), law_bound(st_, TAU["ordinal_t2"], L["kept"])
    print("ordinal: mean b", got_b, "quadrature", mb, "tol", tb, "| mean t2", got_t, "quadrature", mt, "tol", tt)
    assert abs(got_b - mb) <= tb and abs(got_t - mt) <= tt
    sd_t = np.sqrt(ls["sum_thr2"][1] / ps["nKept"] - got_t ** 2)
    assert 0.5 * st_ < sd_t < 2.0 * st_


def test_law_right_censored_gaussian(ngp):
    """N = 60, the records above 3.5 known only to exceed it: the means of (b, varE) against 2-D quadrature; tau = 1.2 and
    2.1 (simulate_censored)."""
    L = RL.law_censored()
    y = L["y"].copy(); y[L["rows"]] = np.nan
    s, ps = run_law(ngp, L, lambda s: s.set_censored(L["rows"], L["lo"], L["hi"]), y)
    (mb, sb), (mv, sv) = RL.posterior_censored(L["y"], L["rows"], L["lo"], L["e_df"], L["e_scale"])
    got_b, got_v = ps["sum_b"] / ps["nKept"], ps["sum_varE"] / ps["nKept"]
    tb, tv = law_bound(sb, TAU["censored_b"], L["kept"]), law_bound(sv, TAU["censored_varE"], L["kept"])
    print("censored: mean b", got_b, "quadrature", mb, "tol", tb, "| mean varE", got_v, "quadrature", mv, "tol", tv)
    assert abs(got_b - mb) <= tb and abs(got_v - mv) <= tv
    assert np.all(s.liability_state()["liab"] >= 3.5)


# ---- held-out rows beside liabilities, fused chains, pooled sums ----
def fold_chain(ngp, G, v, Xf, cls, H, chain_id, owner=None, shards=0, sched=(10, 2, 2)):
    s = base(ngp, G, v, Xf, chain_id=chain_id, owner=owner, shards=shards)
    s.set_holdout(H); s.set_classes(cls, 3)
    s.set_y(np.zeros(G.shape[0])); s.set_schedule(*sched)
    return s


def test_fused_fold_chains_and_the_pooled_threshold_sums(ngp, O):
    N, P, sched = 300, 256, (10, 2, 2)
    G, y, v = make_codes(O, N, P)
    Xf = np.random.default_rng(3).normal(size=(N, 2))
    cls = (1 + (y > np.quantile(y, 0.3)) + (y > np.quantile(y, 0.8))).astype(np.int32)
    fold = ngp.deal_folds(y, 2, foldSeed=2)
    masks = [np.flatnonzero(fold == c) for c in range(2)]
    shards = ngp.Sampler(device=0).shards_for_pass(2)
    fused = []
    for c in range(2):
        g = cls.copy(); g[masks[c]] = 1000 + c                       # held-out class entries are garbage: they are not read
        fused.append(fold_chain(ngp, G, v, Xf, g, masks[c], c, owner=fused[0] if c else None, shards=shards))
    R, S, _ = fused[0].layout()
    fused[0].get_timing()
    l0 = fused[0].get_timing()["sweep_launches"]
    ngp.Sampler.run_many(fused, sched[0])
    fused_one_launch = fused[0].get_timing()["sweep_launches"] - l0 == sched[0]
    states = []
    for c in range(2):
        alone = fold_chain(ngp, G, v, Xf, cls, masks[c], c, shards=S)
        assert alone.layout()[:2] == (R, S)
        alone.run(sched[0])
        same_state(full_state(fused[c]), full_state(alone))
        same_state(fused[c].liability_state(), alone.liability_state()); same_state(fused[c].holdout_state(), alone.holdout_state())
        states.append(alone.liability_state())
    print("fused: one launch per iteration served both chains:", fused_one_launch)
    n0 = fused[0].posterior_len()
    ngp.Sampler.allreduce_posterior(fused)
    for f in fused:
        ls = f.liability_state()
        assert np.array_equal(ls["sum_thr"], states[0]["sum_thr"] + states[1]["sum_thr"])
        assert np.array_equal(ls["sum_thr2"], states[0]["sum_thr2"] + states[1]["sum_thr2"])
    assert fused[0].posterior_len() == n0 and states[0]["sum_thr"][1] > 0.0
    plain = base(ngp, G, v, Xf, chain_id=7, owner=fused[0])           # a chain without liabilities is another model to the pool and to a call
    plain.set_y(y); plain.set_schedule(*sched)
    with pytest.raises(ngp.NextGPHipError, match="do not share one model"):
        ngp.Sampler.allreduce_posterior([fused[0], plain])
    with pytest.raises(ngp.NextGPHipError, match="all carry liability traits"):
        ngp.Sampler.run_many([fused[0], plain], 1)


# ---- resume and refusals ----
def small(ngp, O, kind, chain_id=0, other=False, sched=SCHED):
    N, P = 100, 192
    G, y, v = make_codes(O, N, P)
    s = ngp.Sampler(device=0, seed=SEED, chain=chain_id)
    s.set_panel(G, centre=True)
    add_sets(s, [(0, P, "PR")], v)
    if kind == "classes":
        cls = (1 + (y > np.quantile(y, 0.3)) + (y > np.quantile(y, 0.8))).astype(np.int32)
        if other:
            cls[5] = 1 + cls[5] % 3
        s.set_classes(cls, 3)
    elif kind == "bounds":
        A = np.arange(0, N, 3).astype(np.int64)
        lo = y[A] - 0.5
        s.set_censored(A, lo + (0.25 if other else 0.0), np.full(len(A), INF))
    s.set_y(y); s.set_residual_prior(4.0, 0.25 * float(y.var())); s.set_schedule(*sched)
    return s


@pytest.mark.parametrize("kind", ["classes", "bounds"])
def test_snapshot_resume_and_refusal(ngp, O, tmp_path, kind):
    ref = small(ngp, O, kind)
    ref.run(10)
    a = small(ngp, O, kind)
    a.run(7)
    path = os.fspath(tmp_path / "snap.bin")
    a.save_snapshot(path)
    b = small(ngp, O, kind)
    b.load_snapshot(path)
    same_state(b.get_state(), a.get_state()); same_state(b.liability_state(), a.liability_state())
    b.run(3)
    same_state(b.get_state(), ref.get_state()); same_state(b.liability_state(), ref.liability_state())
    same_state(b.get_posterior_sums(), ref.get_posterior_sums())
    with pytest.raises(ngp.NextGPHipError, match="liability rows, classes or bounds differ"):
        small(ngp, O, kind, other=True).load_snapshot(path)
    with pytest.raises(ngp.NextGPHipError, match="liability"):
        small(ngp, O, "bounds" if kind == "classes" else "classes").load_snapshot(path)
    none = small(ngp, O, None)
    with pytest.raises(ngp.NextGPHipError, match="liability traits"):
        none.load_snapshot(path)
    none.run(2)
    plain = os.fspath(tmp_path / "plain.bin")
    none.save_snapshot(plain)
    with pytest.raises(ngp.NextGPHipError, match="liability traits"):
        small(ngp, O, kind).load_snapshot(plain)
    # the state through the getters and setters: get -> set on a fresh chain -> continue
    c = small(ngp, O, kind)
    c.set_state(a.get_state()); c.set_posterior_sums(a.get_posterior_sums()); c.set_liability_state(a.liability_state())
    c.run(3)
    same_state(c.get_state(), ref.get_state()); same_state(c.liability_state(), ref.liability_state())


def test_a_census_failure_does_not_augment_twice(ngp, O):
    sched = (8, 2, 1)
    ref = small(ngp, O, "classes", sched=sched)
    ref.run(8)
    d = small(ngp, O, "classes", sched=sched)
    d.debug_fail_census(3)
    d.run(8)
    assert d.census()["retries"] == 1
    same_state(d.get_state(), ref.get_state()); same_state(d.liability_state(), ref.liability_state())


def test_no_liabilities_is_no_change_and_refusals_leave_a_handle_that_runs(ngp, O, tmp_path):
    ref = small(ngp, O, None)
    ref.get_timing(); ref.run(12)
    launches = ref.get_timing()["sweep_launches"]
    ref.save_snapshot(os.fspath(tmp_path / "ref.bin"))
    N, P = 100, 192
    G, y, v = make_codes(O, N, P)
    s = ngp.Sampler(device=0, seed=SEED, chain=0)
    s.set_panel(G, centre=True)
    add_sets(s, [(0, P, "PR")], v)
    s.set_holdout([7])
    ok = np.ones(N, dtype=np.int32); ok[::2] = 2
    only_held = ok.copy(); only_held[:] = 1; only_held[7] = 2            # class 2 has no record that is not held out
    for cls, C_ in ((only_held, 2), (ok, 9), (np.zeros(N, dtype=np.int32), 2), (ok, 1)):
        with pytest.raises((ngp.NextGPHipError, ValueError)):
            s.set_classes(cls, C_)
    for rows, lo, hi in (([3], [1.0], [1.0]), ([3], [2.0], [1.0]), ([7], [0.0], [1.0]), ([3], [-INF], [INF])):
        with pytest.raises((ngp.NextGPHipError, ValueError)):
            s.set_censored(rows, lo, hi)
    s.set_classes(ok, 2)
    with pytest.raises(ngp.NextGPHipError, match="remove them first"):
        s.set_censored([3], [0.0], [1.0])
    with pytest.raises(ngp.NextGPHipError, match="probit scale"):
        s.fix_residual_variance(2.0)
    s.set_classes(None); s.set_censored(None, None, None); s.set_holdout(None)
    assert s.liability_layout() == (0, 0)
    s.set_y(y); s.set_residual_prior(4.0, 0.25 * float(y.var())); s.set_schedule(*SCHED)
    for call in (lambda: s.set_classes(ok, 2), lambda: s.set_censored([3], [0.0], [1.0])):
        with pytest.raises(ngp.NextGPHipError, match="before ngp_set_y"):
            call()
    with pytest.raises(ngp.NextGPHipError, match="no liability traits"):
        s.liability_state()
    s.get_timing(); s.run(12)                                        # every refusal left a handle that still runs -- the parent's chain
    same_state(s.get_state(), ref.get_state())
    assert s.posterior_len() == ref.posterior_len() == 3 * 192 + 1 + 2 + 3 and s.get_timing()["sweep_launches"] == launches
    s.save_snapshot(os.fspath(tmp_path / "s.bin"))
    assert (tmp_path / "s.bin").read_bytes() == (tmp_path / "ref.bin").read_bytes()
    # a fixed residual variance alone: held from set_y on, reported by the trace, flagged in the snapshot
    f = small(ngp, O, None)
    f.fix_residual_variance(0.75); f.set_y(y)
    f.run(5)
    assert f.get_state()["varE"] == 0.75 and np.all(f.get_trace(5)["varE"] == 0.75)
    f.save_snapshot(os.fspath(tmp_path / "f.bin"))
    with pytest.raises(ngp.NextGPHipError, match="fixed at another value, or sampled"):
        ref.load_snapshot(os.fspath(tmp_path / "f.bin"))
    f.fix_residual_variance(0.0); f.run(2)
    assert f.get_state()["varE"] != 0.75


# ---- runLMEM end to end ----
def test_runlmem_categorical_and_censored(ngp, O, tmp_path):
    N, P = 200, 192
    G, y, v = make_codes(O, N, P)
    np.savetxt(tmp_path / "m.txt", G, fmt="%d")
    f = f'y ~ 1 + SNP(M1,"{tmp_path / "m.txt"}")'
    VCV = {"M1": ngp.BayesPR(9999, v / y.var())}
    z = (y - y.mean()) / y.std()
    # two classes
    yb = np.where(z > 0.2, 5.0, 2.0)                                       # the class values are labels: sorted, they become 1 and 2
    res = ngp.runLMEM(f, {"y": yb}, 40, 8, 2, VCV=VCV, outFolder=str(tmp_path / "bin"), trait="categorical")
    assert res["nKept"] == 16 and res["varE"] == 1.0 and res["classes"].tolist() == [2.0, 5.0] and len(res["thresholds"]["mean"]) == 0
    ve = np.loadtxt(tmp_path / "bin" / "varEOut", skiprows=1)
    assert len(ve) == 16 and np.all(ve == 1.0)
    s = res["sampler"]
    assert s.liability_layout() == (N, 2) and s.liability_fallthrough() == 0
    ls = s.liability_state()
    assert np.all(ls["liab"][yb == 5.0] >= 0.0) and np.all(ls["liab"][yb == 2.0] <= 0.0)
    assert np.corrcoef(G.astype(np.float64) @ res["sets"]["M1"]["beta"], z)[0, 1] > 0      # the effects point the way of the liability
    # four classes: the thresholds are increasing, their means come from the device's sums
    y4 = np.digitize(z, [-0.7, 0.1, 0.9]).astype(np.float64)
    res4 = ngp.runLMEM(f, {"y": y4}, 40, 8, 2, VCV={**VCV, "e": ngp.Random("I", 1.0)}, outFolder=str(tmp_path / "four"), trait="categorical")
    ls4 = res4["sampler"].liability_state()
    th = res4["thresholds"]
    assert np.array_equal(th["mean"], ls4["sum_thr"][1:] / 16) and len(th["mean"]) == 2 and 0.0 < th["mean"][0] < th["mean"][1]
    assert np.all(th["sd"] >= 0.0) and res4["varE"] == 1.0 and res4["classes"].tolist() == [0.0, 1.0, 2.0, 3.0]
    rows = (tmp_path / "four" / "thresholdOut").read_text().splitlines()
    assert rows[0] == "t2\tt3" and len(rows) == 17                          # the header row is pinned: t2 .. t{C-1}
    tr = np.array([[float(x) for x in r.split("\t")] for r in rows[1:]])
    acc = np.zeros(2)
    for r in tr:                                                           # the device's sums: draw after draw, left to right
        acc = acc + r
    assert np.array_equal(th["mean"], acc / 16) and np.array_equal(tr[-1], ls4["thr"][1:]) and np.all(tr[:, 0] < tr[:, 1])
    assert (tmp_path / "four" / "varEOut").read_text().splitlines()[0] == "e" and not (tmp_path / "bin" / "thresholdOut").exists()
    assert not (tmp_path / "four" / "samples.ngpsmp").exists()
    assert np.all(np.loadtxt(tmp_path / "four" / "varEOut", skiprows=1) == 1.0)
    # censored: the response column is ignored on the censored records, exact records take lower == upper
    cut = np.quantile(y, 0.7)
    lower = np.where(y > cut, cut, y); upper = np.where(y > cut, np.inf, y)
    junk = np.where(y > cut, 1e9, np.nan)                                  # the response column itself is not what is read
    VCVc = {"M1": ngp.BayesPR(9999, v), "e": ngp.Random("I", 0.25 * y.var())}
    resc = ngp.runLMEM(f, {"y": junk, "lo": lower, "hi": upper}, 40, 8, 2, VCV=VCVc, outFolder=str(tmp_path / "cens"),
                       censored={"lower": "lo", "upper": "hi"})
    sc = resc["sampler"]
    m, C_ = sc.liability_layout()
    assert m == int((y > cut).sum()) and C_ == 0 and np.all(sc.liability_state()["liab"] >= cut) and 0.0 < resc["varE"] < 10.0 * y.var()
    assert "thresholds" not in resc and sc.liability_fallthrough() == 0
    # two folds of the binary trait: fold-chains over one panel, every record validated on the liability scale
    resf = ngp.runLMEM(f, {"y": yb}, 40, 8, 2, VCV=VCV, outFolder=str(tmp_path / "folds"), trait="categorical", folds=2, samples="none")
    cv = resf["cv"]
    assert np.all(np.isfinite(cv["yhat"])) and len(resf["chains"]) == 2 and all(len(r["thresholds"]["mean"]) == 0 for r in resf["chains"])
    assert [smp.liability_layout() for smp in resf["samplers"]] == [(N // 2, 2)] * 2
    assert np.corrcoef(cv["yhat"], z)[0, 1] > 0


def test_sample_file_carries_the_thresholds_of_three_or_more_classes(ngp, O, tmp_path):
    """"NGPSMP05": a record of an ordered trait ends with t_2 .. t_{C-1}; two classes and censored records write the file of a chain
    without liabilities (same magic, same record length)."""
    N = 50
    rng = np.random.default_rng(2)
    recs = {}
    for name, setup in (("plain", None), ("two", lambda s: s.set_classes((1 + rng.integers(0, 2, N)).astype(np.int32), 2)),
                        ("four", lambda s: s.set_classes((1 + np.arange(N) % 4).astype(np.int32), 4))):
        s = ngp.Sampler(device=0, seed=SEED, chain=0)
        s.set_records(N)
        s.add_random_set(np.arange(N) % 5, 5, varU0=0.3)
        if setup:
            setup(s)
        s.set_y(rng.normal(size=N)); s.set_schedule(*SCHED)
        path = os.fspath(tmp_path / f"{name}.ngpsmp")
        s.set_sample_file(path)
        got = []
        for t in range(SCHED[0]):
            s.run(1)
            if name == "four" and t + 1 >= 6 and (t + 1) % 2 == 0:
                got.append(s.liability_state()["thr"][1:].copy())
        s.set_sample_file(None)
        recs[name] = (open(path, "rb").read(), ngp.read_sample_file(path), got)
    assert recs["plain"][0][:8] == recs["two"][0][:8] == b"NGPSMP02" and recs["four"][0][:8] == b"NGPSMP05"
    assert len(recs["plain"][0]) == len(recs["two"][0]) and "thr" not in recs["two"][1]
    four = recs["four"][1]
    assert np.array_equal(four["iter"], [6, 8, 10, 12]) and np.array_equal(four["thr"], np.array(recs["four"][2])) and np.all(four["varE"] == 1.0)
    assert len(recs["four"][0]) == len(recs["plain"][0]) + 3 * 8 + 4 * 16       # nlv = 0, nrc = 0 and nthr in the header; two doubles a record
    one = list(ngp._lib.iter_sample_file(os.fspath(tmp_path / "four.ngpsmp")))
    assert np.array_equal(np.array([r["thr"] for r in one]), four["thr"])
