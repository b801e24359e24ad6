"""Held-out records on the device (include/nextgp_hip.h, "held-out records"; DESIGN.md section 2, "Held-out records"): a record without a
phenotype stays in the panel and its phenotype is redrawn every iteration from its conditional, ycorr_i <- e_i.  The reference has
nothing of this kind; what is checked here is the arithmetic DESIGN.md fixes, restated in tests/ref_holdout.py: the masked chain IS the
ordinary chain on the augmented data, bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

import ref_holdout as RH
from conftest import add_sets
from test_gpu_compact import make_codes

pytestmark = pytest.mark.gpu

SCHED = (12, 4, 2)                        # kept: 6, 8, 10, 12
KEYS = ("ycorr", "beta", "delta", "varBeta", "piHat", "varE", "b", "iter")


def kept(it, sched=SCHED):
    n, burn, thin = sched
    return burn + thin <= it <= n and (it - burn) % thin == 0


def mask(N, m, seed=11):
    """m held-out rows of N: the first, the last and m - 2 others."""
    inner = np.random.default_rng(seed).choice(np.arange(1, N - 1), size=m - 2, replace=False)
    return np.sort(np.concatenate([[0, N - 1], inner])).astype(np.int64)


# the shapes of the first test: N = 100 (the last shard is padded where the layout's rows do not divide it), P = 192 is three 64-SNP blocks, 25 rows held out; the weights are
# powers of four, so that the row scales are powers of two and scaling a residual and unscaling it again changes no bit (the comparison
# chain is driven through ngp_get_state / ngp_set_state, which unscale and scale)
CASES = {
    "fp32": dict(N=100, P=192, m=25),                         # (fp32 tiles: 25 shards of 4 rows, L == N)
    "fp32_padded": dict(N=100, P=192, m=25, shards=7, padded=True),   # at most 7 shards: L > N, the padding rows are live
    "u8": dict(N=100, P=192, m=25, storage="u8", padded=True),   # byte tiles: shards of 16 rows, L = 112
    "weights": dict(N=100, P=192, m=25, weights=True),
    "mixed": dict(N=100, P=192, m=25, mixed=True),            # BayesR + one fixed-effect set + a (1|g) set
    "two_workgroups": dict(N=700, P=128, m=300),              # 300 held-out rows: two workgroups of 256 lanes
}


def problem(O, N, P, weights=False):
    G, y, v = make_codes(O, N, P)
    w = np.random.default_rng(N + P).choice([0.25, 1.0, 4.0, 16.0], size=N) if weights else None
    return G, y, v, w


def chain(ngp, G, y, v, H=None, w=None, storage=None, mixed=False, seed=1001, chain_id=0, sched=SCHED, owner=None, shards=0, vy=None):
    vy = float(np.nanvar(y)) if vy is None else vy    # (chains that are compared get the same priors: pass vy where their y differ)
    s = ngp.Sampler(device=0, seed=seed, chain=chain_id, storage=storage)
    if owner is not None:
        s.share_panel(owner)
    else:
        if w is not None:
            s.set_residual_weights(w)
        if shards:
            s.set_max_shards(shards)
        s.set_panel(G, centre=True)
    N, P = G.shape
    if mixed:
        rng = np.random.default_rng(9)
        add_sets(s, [(0, P, "R")], v)
        s.add_fixed_set(rng.normal(size=(N, 2)))
        s.add_random_set(rng.integers(0, 5, size=N), 5, varU0=0.2 * vy)
    else:
        add_sets(s, [(0, P, "PR")], v)
    if H is not None:
        s.set_holdout(H)
    s.set_y(y); s.set_residual_prior(4.0, 0.25 * vy); s.set_schedule(*sched)
    return s


def full_state(s, mixed=False):
    st = s.get_state()
    if mixed:
        st["fixed"] = s.get_fixed()["b"]
        r = s.get_random(0)
        st["u"], st["varU"] = r["u"], r["varU"]
        st["class_pi"] = s.get_class_state(0)["piHat"]
    return st


def same_state(a, b):
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def set_ycorr(s, ycorr, st):
    """ngp_set_state with the residual alone (every other array NULL: they stay as they are)."""
    yc = np.ascontiguousarray(ycorr, dtype=np.float64)
    s._chk(s.L.ngp_set_state(s.h, yc.ctypes.data_as(C.POINTER(C.c_double)), None, None, None, None, C.c_double(st["varE"]), C.c_double(st["b"]),
                             C.c_int64(st["iter"])))


@pytest.mark.parametrize("case", list(CASES))
def test_masked_chain_is_the_ordinary_chain_on_the_augmented_data(ngp, O, case):
    """Handle A carries the mask (NaN on the held-out rows), handle B none and the observed mean there.  Before every iteration B's
    residual of the held-out rows is replaced from outside by sqrt(varE) z, z the normals of stream kind 21 keyed by the row (with
    weights: by that value unscaled, which ngp_set_state scales back to the same bits); then both run one iteration.  Every part of the
    state agrees bit for bit after every step, and yaug follows the restatement."""
    c = CASES[case]
    N, P, mixed = c["N"], c["P"], c.get("mixed", False)
    G, y, v, w = problem(O, N, P, c.get("weights", False))
    H = mask(N, c["m"])
    assert H[0] == 0 and H[-1] == N - 1 and len(H) == c["m"]
    y_nan = y.copy(); y_nan[H] = np.nan
    y0, yaug = RH.start(y_nan, H)
    A = chain(ngp, G, y_nan, v, H=H, w=w, storage=c.get("storage"), mixed=mixed, vy=y.var(), shards=c.get("shards", 0))
    B = chain(ngp, G, y0, v, w=w, storage=c.get("storage"), mixed=mixed, vy=y.var(), shards=c.get("shards", 0))
    R, S, _ = A.layout()
    if c.get("padded"):
        assert R * S > N                                                    # padding rows are live
    assert np.array_equal(A.holdout_rows(), H) and np.array_equal(A.holdout_state()["yaug"], yaug)
    s_H = None if w is None else np.sqrt(w[H])
    drew = 0
    for t in range(1, 7):
        stA, stB = full_state(A, mixed), full_state(B, mixed)
        same_state(stA, stB)
        z = B.draws_indexed(t, RH.KIND_AUGMENT, 0, 1, N)[H]
        yaug, e, ep = RH.step(yaug, stB["ycorr"][H], stB["varE"], z, s_H)
        if e is not None:
            yc = stB["ycorr"].copy(); yc[H] = ep
            set_ycorr(B, yc, stB)
            drew += 1
        else:
            assert t == 1
        A.run(1); B.run(1)
        assert np.array_equal(A.holdout_state()["yaug"], yaug), t
    same_state(full_state(A, mixed), full_state(B, mixed))
    assert drew == 5 and np.all(np.isfinite(yaug)) and np.abs(yaug - y0[H]).max() > 0


def test_held_out_phenotypes_are_never_read(ngp, O):
    G, y, v, _ = problem(O, 100, 192)
    H = mask(100, 25)
    ya, yb = y.copy(), y.copy()
    ya[H] = np.nan; yb[H] = 1e6
    a, b = chain(ngp, G, ya, v, H=H, vy=y.var()), chain(ngp, G, yb, v, H=H, vy=y.var())
    a.run(20); b.run(20)
    sa, sb = a.get_state(), b.get_state()
    same_state(sa, sb)
    ha, hb = a.holdout_state(), b.holdout_state()
    same_state(ha, hb)
    assert all(np.all(np.isfinite(sa[k])) for k in KEYS) and all(np.all(np.isfinite(ha[k])) for k in ha)
    assert sa["iter"] == 20 and np.abs(sa["ycorr"]).max() < 1e3


def test_sums_over_kept_draws(ngp, O):
    """With thinning: what Python accumulates from the state after every kept iteration equals the device's sums bit for bit (the same
    operations in the same order), n_fit counts the kept draws, rows off the mask stay exactly zero."""
    N = 100
    G, y, v, _ = problem(O, N, 192)
    H = mask(N, 25)
    y[H] = np.nan
    s = chain(ngp, G, y, v, H=H)
    s1 = np.zeros(N); s2 = np.zeros(N); nf = np.zeros(N)
    for it in range(1, SCHED[0] + 1):
        s.run(1)
        if kept(it):
            RH.accumulate(s1, s2, nf, H, s.holdout_state()["yaug"], s.get_state()["ycorr"][H])
        elif it == 5:
            assert not s.holdout_state()["n_fit"].any()                     # burn-in: nothing yet
    hs = s.holdout_state()
    assert np.array_equal(hs["sum_fit"], s1) and np.array_equal(hs["sum_fit2"], s2) and np.array_equal(hs["n_fit"], nf)
    off = np.setdiff1d(np.arange(N), H)
    assert np.all(hs["n_fit"][H] == 4) and not hs["n_fit"][off].any() and not hs["sum_fit"][off].any() and not hs["sum_fit2"][off].any()
    ho = s.holdout()
    m = s1[H] / 4
    assert np.array_equal(ho["rows"], H) and np.array_equal(ho["mean"], m) and np.array_equal(ho["sd"], np.sqrt(np.maximum(0.0, s2[H] / 4 - m * m)))
    s.set_y(y)                                                              # zeroed wherever sum_beta is
    z = s.holdout_state()
    assert not z["n_fit"].any() and not z["sum_fit"].any() and not z["sum_fit2"].any()


def _law_y():
    y = 3.0 + np.random.default_rng(41).normal(size=64)
    y[LAW["H"]] = np.nan
    return y


LAW = dict(H=np.arange(2, 64, 4).astype(np.int64), burn=500, kept=4000, e_scale=0.5, seed=7, y=_law_y)


def test_law_of_the_intercept_only_model(ngp):
    """Records only, intercept only, 16 of 64 records held out: the posterior of b is N(ybar_obs, varE / n_obs), and augmentation adds
    lag-1 autocorrelation of about f = 16 / 64 to its chain.  mean(b) and the mean fitted value of every held-out record over 4,000 kept
    draws lie within 6 sqrt(v (1 + f) / ((1 - f) n_obs nKept)) of ybar_obs, v the mean varE (derived, not measured;
    tests/test_holdout_host.py holds the restatement to the same bound)."""
    y, H = LAW["y"](), LAW["H"]
    assert len(H) == 16 and np.all(np.isnan(y[H]))
    s = ngp.Sampler(device=0, seed=LAW["seed"], chain=0)
    s.set_records(64)
    s.set_holdout(H)
    s.set_y(y); s.set_residual_prior(4.0, LAW["e_scale"]); s.set_schedule(LAW["burn"] + LAW["kept"], LAW["burn"], 1)
    s.run(LAW["burn"] + LAW["kept"])
    ps, ho = s.get_posterior_sums(), s.holdout()
    assert ps["nKept"] == LAW["kept"] and np.all(ho["n"] == LAW["kept"])
    vbar = ps["sum_varE"] / ps["nKept"]
    tol = RH.law_bound(vbar, 16 / 64, 48, LAW["kept"])
    yb = RH.ybar_obs(y, H)
    print("law: ybar_obs", yb, "mean b", ps["sum_b"] / ps["nKept"], "mean varE", vbar, "tol", tol, "max |fit - ybar|", np.abs(ho["mean"] - yb).max())
    assert abs(ps["sum_b"] / ps["nKept"] - yb) <= tol
    assert np.all(np.abs(ho["mean"] - yb) <= tol)
    assert 0.5 < vbar < 2.0                                                 # (the data were drawn with variance 1)


def test_fused_fold_chains_and_the_pooled_sums(ngp, O):
    """Four chains over one shared panel, each with its own mask, through run_many: every chain is the chain it is alone, and
    allreduce_posterior leaves the elementwise sums of the four chains' hold-out sums on every handle."""
    N, P, K, sched = 300, 256, 4, (10, 2, 2)
    G, y, v, _ = problem(O, N, P)
    fold = ngp.deal_folds(y, K, foldSeed=2)
    masks = [np.flatnonzero(fold == c) for c in range(K)]
    shards = ngp.Sampler(device=0).shards_for_pass(K)
    fused = []
    for c in range(K):
        fused.append(chain(ngp, G, y, v, H=masks[c], chain_id=c, sched=sched, owner=fused[0] if c else None, shards=shards))
    assert [len(f.holdout_rows()) for f in fused] == [75] * 4                # a sharer does not inherit the owner's mask: each has its own
    R, S, _ = fused[0].layout()
    fused[0].get_timing()
    l0 = fused[0].get_timing()["sweep_launches"]
    ngp.Sampler.run_many(fused, sched[0])
    assert fused[0].get_timing()["sweep_launches"] - l0 == sched[0]          # ONE launch per iteration served the four chains
    states = []
    for c in range(K):
        alone = chain(ngp, G, y, v, H=masks[c], chain_id=c, sched=sched, shards=S)
        assert alone.layout()[:2] == (R, S)
        alone.run(sched[0])
        same_state(fused[c].get_state(), alone.get_state())
        same_state(fused[c].holdout_state(), alone.holdout_state())
        states.append(alone.holdout_state())
    n0 = fused[0].posterior_len()
    ngp.Sampler.allreduce_posterior(fused)
    tot = {k: states[0][k] + states[1][k] + states[2][k] + states[3][k] for k in ("sum_fit", "sum_fit2", "n_fit")}
    for f in fused:
        hs = f.holdout_state()
        assert all(np.array_equal(hs[k], tot[k]) for k in tot)
    assert np.all(tot["n_fit"] == 4) and fused[0].posterior_len() == n0
    cv = fused[0].holdout()                                                 # every record, validated by the chain that held it out
    assert np.array_equal(cv["rows"], np.arange(N)) and np.corrcoef(cv["mean"], y)[0, 1] > 0
    plain = chain(ngp, G, y, v, chain_id=7, sched=sched, owner=fused[0])      # a chain without a mask is another model to the pool
    with pytest.raises(ngp.NextGPHipError, match="do not share one model"):
        ngp.Sampler.allreduce_posterior([fused[0], plain])


def test_snapshot_resume_and_refusal(ngp, O, tmp_path):
    G, y, v, _ = problem(O, 100, 192)
    H = mask(100, 25)
    y[H] = np.nan
    ref = chain(ngp, G, y, v, H=H)
    ref.run(10)
    a = chain(ngp, G, y, v, H=H)
    a.run(7)
    path = os.fspath(tmp_path / "snap.bin")
    a.save_snapshot(path)
    b = chain(ngp, G, y, v, H=H)
    b.load_snapshot(path)
    same_state(b.get_state(), a.get_state()); same_state(b.holdout_state(), a.holdout_state())
    b.run(3)
    same_state(b.get_state(), ref.get_state()); same_state(b.holdout_state(), ref.holdout_state())
    same_state({k: v_ for k, v_ in b.get_posterior_sums().items()}, ref.get_posterior_sums())
    y_full = np.where(np.isnan(y), 0.0, y)
    H2 = np.sort(np.append(H[:-1], 98))
    assert len(H2) == len(H) and not np.array_equal(H2, H)
    other = chain(ngp, G, y_full, v, H=H2)                                  # another mask of the same size
    with pytest.raises(ngp.NextGPHipError, match="held-out records differ"):
        other.load_snapshot(path)
    none = chain(ngp, G, y_full, v)
    with pytest.raises(ngp.NextGPHipError, match="held-out records"):
        none.load_snapshot(path)
    none.run(2)
    plain = os.fspath(tmp_path / "plain.bin")
    none.save_snapshot(plain)
    with pytest.raises(ngp.NextGPHipError, match="held-out records"):
        other.load_snapshot(plain)
    # the state through the getters and setters: get -> set on a fresh chain -> continue
    c = chain(ngp, G, y, v, H=H)
    c.set_state(a.get_state()); c.set_posterior_sums(a.get_posterior_sums()); c.set_holdout_state(a.holdout_state())
    c.run(3)
    same_state(c.get_state(), ref.get_state()); same_state(c.holdout_state(), ref.holdout_state())


def test_a_census_failure_leaves_the_masked_chain_as_it_is(ngp, O):
    """The sweep of iteration 3 ends at its census once and is run again: the head -- and with it the augmentation -- is not, and the
    kernels queued behind the failed launch changed nothing."""
    G, y, v, _ = problem(O, 100, 192)
    H = mask(100, 25)
    y[H] = np.nan
    sched = (8, 2, 1)
    ref = chain(ngp, G, y, v, H=H, sched=sched)
    ref.run(8)
    d = chain(ngp, G, y, v, H=H, sched=sched)
    d.debug_fail_census(3)
    d.run(8)
    assert d.census()["retries"] == 1
    same_state(d.get_state(), ref.get_state()); same_state(d.holdout_state(), ref.holdout_state())


def test_no_mask_is_no_change(ngp, O, tmp_path):
    """set_holdout(None) and m = 0: state, packed posterior length, snapshot bytes and launch count of a handle that never heard of the
    call; a NaN phenotype is still refused there."""
    G, y, v, _ = problem(O, 100, 192)
    ref = chain(ngp, G, y, v)
    ref.get_timing(); ref.run(12)
    launches = ref.get_timing()["sweep_launches"]                           # (reading the counters clears them)
    assert launches > 0
    ref.save_snapshot(os.fspath(tmp_path / "ref.bin"))
    for how in (None, []):
        s = ngp.Sampler(device=0, seed=1001, chain=0)
        s.set_panel(G, centre=True)
        add_sets(s, [(0, 192, "PR")], v)
        s.set_holdout(how)
        assert len(s.holdout_rows()) == 0
        s.set_y(y); s.set_residual_prior(4.0, 0.25 * float(np.nanvar(y))); s.set_schedule(*SCHED)   # (chain()'s prior)
        s.get_timing(); s.run(12)
        same_state(s.get_state(), ref.get_state())
        assert s.posterior_len() == ref.posterior_len() == 3 * 192 + 1 + 2 + 3
        assert s.get_timing()["sweep_launches"] == launches
        s.save_snapshot(os.fspath(tmp_path / "s.bin"))
        assert (tmp_path / "s.bin").read_bytes() == (tmp_path / "ref.bin").read_bytes()
        with pytest.raises(ngp.NextGPHipError, match="no hold-out set"):
            s.holdout_state()
        bad = y.copy(); bad[3] = np.nan
        with pytest.raises(ngp.NextGPHipError, match="non-finite phenotype"):
            s.set_y(bad)
    # with a mask: a NaN outside it is refused all the same, and so are bad masks and a mask behind set_y
    s = ngp.Sampler(device=0, seed=1001, chain=0)
    s.set_panel(G, centre=True)
    add_sets(s, [(0, 192, "PR")], v)
    for rows in ([3, 3], [4, 3], [-1, 2], [0, 100], list(range(100))):
        with pytest.raises(ngp.NextGPHipError):
            s.set_holdout(rows)
    s.set_holdout([3, 50])
    bad = y.copy(); bad[4] = np.nan
    with pytest.raises(ngp.NextGPHipError, match="non-finite phenotype"):
        s.set_y(bad)
    assert s.posterior_len() == ref.posterior_len() + 3 * 100
    s.set_y(y)
    with pytest.raises(ngp.NextGPHipError, match="before ngp_set_y"):
        s.set_holdout([1])


def test_runlmem_folds_and_missing(ngp, O, tmp_path):
    N, P = 60, 128
    G, y, v, _ = problem(O, N, P)
    np.savetxt(tmp_path / "m.txt", G, fmt="%d")
    f = f'y ~ 1 + SNP(M1,"{tmp_path / "m.txt"}")'
    VCV = {"M1": ngp.BayesPR(9999, v), "e": ngp.Random("I", 0.25 * y.var())}
    out = tmp_path / "cv"
    res = ngp.runLMEM(f, {"y": y}, 20, 4, 2, VCV=VCV, outFolder=str(out), folds=3, foldSeed=5, samples="none")
    cv = res["cv"]
    assert (out / "cvPredict.txt").exists() and all((out / f"chain{c}").is_dir() for c in range(3)) and not (out / "holdoutPredict.txt").exists()
    rows = np.loadtxt(out / "cvPredict.txt", skiprows=1)
    assert sorted(rows[:, 0].astype(int).tolist()) == list(range(1, N + 1))  # every observed record once
    assert np.array_equal(cv["fold"], ngp.deal_folds(y, 3, foldSeed=5)) and cv["pooled_over_folds"] is True
    order = np.argsort(rows[:, 0])
    assert np.array_equal(rows[order, 1], cv["fold"]) and np.array_equal(rows[order, 3], cv["yhat"]) and np.array_equal(rows[order, 2], y)
    for c in range(3):                                                      # each chain's own means, on its fold
        own = res["chains"][c]["holdout"]
        assert np.array_equal(own["rows"], np.flatnonzero(cv["fold"] == c)) and np.all(own["n"] == 8)
        assert np.array_equal(cv["yhat"][own["rows"]], own["mean"]) and np.array_equal(cv["sd"][own["rows"]], own["sd"])
    assert np.all(np.isfinite(cv["yhat"])) and -1.0 <= cv["accuracy"] <= 1.0 and len(cv["per_fold"]) == 3
    assert cv["accuracy"] == pytest.approx(np.corrcoef(cv["yhat"], y)[0, 1]) and cv["mse"] == pytest.approx(np.mean((y - cv["yhat"]) ** 2))
    assert cv["slope"] == pytest.approx(np.polyfit(cv["yhat"], y, 1)[0])
    # missing="holdout": exactly the records without a response are predicted; the default still refuses them
    ym = y.copy(); ym[[7, 33]] = np.nan
    out2 = tmp_path / "miss"
    res2 = ngp.runLMEM(f, {"y": ym}, 20, 4, 2, VCV=VCV, outFolder=str(out2), missing="holdout", samples="none")
    assert np.array_equal(res2["holdout"]["rows"], [7, 33]) and np.all(res2["holdout"]["n"] == 8) and np.all(np.isfinite(res2["holdout"]["yhat"]))
    rows2 = np.loadtxt(out2 / "holdoutPredict.txt", skiprows=1)
    assert rows2[:, 0].tolist() == [8.0, 34.0] and np.array_equal(rows2[:, 2], res2["holdout"]["yhat"]) and np.all(np.isnan(rows2[:, 1]))
    assert "cv" not in res2
    # both: the folds are dealt among the records with a response, every fold-chain also holds out the two without
    res3 = ngp.runLMEM(f, {"y": ym}, 20, 4, 2, VCV=VCV, outFolder=str(tmp_path / "both"), missing="holdout", folds=3, samples="none")
    assert np.array_equal(res3["holdout"]["rows"], [7, 33]) and np.all(res3["holdout"]["n"] == 24)    # pooled over the three chains
    assert np.all(res3["cv"]["fold"][[7, 33]] == -1) and np.all(np.isnan(res3["cv"]["yhat"][[7, 33]]))
    assert np.isfinite(np.delete(res3["cv"]["yhat"], [7, 33])).all() and len(np.loadtxt(tmp_path / "both" / "cvPredict.txt", skiprows=1)) == N - 2
    with pytest.raises(ngp.NextGPHipError, match="non-finite phenotype"):
        ngp.runLMEM(f, {"y": ym}, 20, 4, 2, VCV=VCV, outFolder=str(tmp_path / "err"), samples="none")
