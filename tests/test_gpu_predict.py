"""Prediction of new individuals on the device (include/nextgp_hip.h, "prediction"; DESIGN.md section 2, "Prediction"): a second
panel beside the training panel, and behind every kept iteration one pass that accumulates g = X_new beta per marker set.  The
reference has no such step -- its user multiplies posterior means on the host (summaryMCMC, src/misc.jl:241-244, gives the means) and
gets no SD; what is checked here is the arithmetic DESIGN.md fixes, restated in tests/ref_predict.py, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import ref_predict as RP
from conftest import add_sets
from test_gpu_compact import make_codes
from test_gpu_bayesrc_engines import TALL_SHAPES

pytestmark = pytest.mark.gpu

P = 330                                  # five 64-column blocks and a tail of ten lanes
# two sets that meet inside block 1, columns 192..255 nobody owns, then a Tuple set (k = 2, 37 loci: block 4 whole, ten lanes of block 5)
SPEC = [(0, 100, "PR"), (100, 92, "B")]
SETS_TUPLE = [(0, 100), (100, 92), (256, 74)]
SPEC_R = SPEC + [(256, 74, "R")]         # the same columns without a Tuple set (engines and fused kernels whose samplers carry none)
ENGINES = {
    "persistent": (dict(), 300, 0, True),
    "perblock": (dict(mode=0, lag=1), 300, 0, True),
    "u8": (dict(storage="u8"), 300, 0, True),
    "tall": (dict(mode=1, lag=6, streamer=4), TALL_SHAPES[2][0], TALL_SHAPES[2][1], False),
}
SCHED = (12, 4, 2)                       # kept: 6, 8, 10, 12


def kept(it, sched=SCHED):
    n, burn, thin = sched
    return burn + thin <= it <= n and (it - burn) % thin == 0


def codes(Np, ncol=P, seed=77):
    return np.random.default_rng(seed).integers(0, 3, size=(Np, ncol)).astype(np.uint8)


def add_model(s, v, tuple_set):
    add_sets(s, SPEC if tuple_set else SPEC_R, v)
    if tuple_set:
        vm = np.array([[v, 0.3 * v], [0.3 * v, v]])
        s.add_marker_set_tuple(256, 37, 2, 5.0, vm * 2.0, [(0, 37)], vm)


def sampler(ngp, O, engine, seed=1001, chain=0, sched=SCHED, P_=P):
    kw, N, shards, tuple_set = ENGINES[engine]
    G, y, v = make_codes(O, N, P_)
    s = ngp.Sampler(device=0, seed=seed, chain=chain, **kw)
    if shards:
        s.set_max_shards(shards)
    s.set_panel(G, centre=True)
    return s, G, y, v, tuple_set


def finish(s, y, v, tuple_set, sched=SCHED):
    add_model(s, v, tuple_set)
    s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var()); s.set_schedule(*sched)


def stored(s, Gp):
    """(X, mean) as ref_predict takes them: what the prediction tiles of s hold for the codes Gp uploaded with centre=True."""
    if s.storage() == 1:
        return Gp.astype(np.float64), s.means()
    return RP.stored_f32(Gp, s.means()), None


def run_and_restate(s, X, mean, sets, niter, sched=SCHED):
    """The chain one iteration at a time; the restatement of every kept draw from the effects the device holds after it."""
    s1 = np.zeros((len(sets) + 1, X.shape[0])); s2 = np.zeros_like(s1)
    lasts, betas = [], []
    for it in range(1, niter + 1):
        s.run(1)
        if kept(it, sched):
            beta = s.get_state()["beta"]
            g = RP.predict_draw(X, beta, sets, mean)
            RP.accumulate(s1, s2, g)
            lasts.append((g, s.prediction_last()))
            betas.append(beta)
    return s1, s2, lasts, betas


@pytest.mark.parametrize("Np", [1, 63, 257, 300])
@pytest.mark.parametrize("engine", list(ENGINES))
def test_bit_for_bit_against_the_restatement(ngp, O, engine, Np):
    """ngp_get_prediction_last after every kept iteration and the sums after 12 iterations with thinning equal tests/ref_predict.py
    bit for bit, on every engine and storage; the input form of the prediction columns (u8 / f64 / f32) does not matter.  The last row
    is the sum of the set rows in set order.  Linearity: sum[total] / nKept against the prediction from sum_beta / nKept -- both are
    within ref_predict.bound of the exact sums for their own effects, the accumulation adds nKept roundings of the same size, so the
    difference stays inside nKept x the bound taken with max_d |beta_d| per column (which dominates every draw's and the mean's)."""
    s, G, y, v, tuple_set = sampler(ngp, O, engine)
    Gp = codes(Np)
    compact = s.storage() == 1
    s.begin_prediction_panel(Np)
    if compact or Np == 1:
        s.prediction_columns(0, Gp, centre=True)
    else:                                  # column ranges in any order, another input type each
        s.prediction_columns(200, Gp[:, 200:].astype(np.float32), centre=True)
        s.prediction_columns(0, Gp[:, :120].astype(np.float64), centre=True)
        s.prediction_columns(120, Gp[:, 120:200], centre=True)
    s.end_prediction_panel()
    finish(s, y, v, tuple_set)
    sets = SETS_TUPLE
    X, mean = stored(s, Gp)
    lay = s.prediction_layout()
    assert lay[0] == Np and lay[1] % 16 == 0 and lay[1] * lay[2] >= Np and lay[3] == 64 * RP.CHUNK_BLOCKS
    s1, s2, lasts, betas = run_and_restate(s, X, mean, sets, 12)
    assert len(lasts) == 4
    for g, last in lasts:
        assert np.array_equal(last, g)
        assert np.array_equal(((0.0 + last[0]) + last[1]) + last[2], last[3])
    assert np.abs(lasts[-1][0][3]).max() > 0
    ps = s.prediction_sums()
    assert ps["nKept"] == 4 and np.array_equal(ps["sum"], s1) and np.array_equal(ps["sum2"], s2)
    assert s.prediction_stats() == (4, 4)
    # linearity
    post = s.get_posterior_sums()
    mb = post["sum_beta"] / post["nKept"]
    bmax = np.max(np.abs(np.array(betas + [mb])), axis=0)
    tol = post["nKept"] * RP.bound(X, bmax, sets, mean)
    lin = RP.predict_draw(X, mb, sets, mean)
    assert np.all(np.abs(ps["sum"] / ps["nKept"] - lin) <= tol)
    # the host summary
    pr = s.prediction()
    m = s1 / 4
    assert np.array_equal(pr["mean"], m[3]) and np.array_equal(pr["sd"], np.sqrt(np.maximum(0.0, s2[3] / 4 - m[3] * m[3])))
    assert len(pr["sets"]) == 3 and np.array_equal(pr["sets"][1]["mean"], m[1])


@pytest.mark.parametrize("engine", ["persistent", "u8"])
def test_a_set_over_three_chunks_with_a_partial_last_one(ngp, O, engine):
    """P = 4500: the first set spans the chunks [0, 2048), [2048, 4096) and [4096, 4400), the second starts inside block 68."""
    Pw, Np, sched = 4500, 63, (6, 2, 2)
    kw = ENGINES[engine][0]
    G, y, v = make_codes(O, 200, Pw)
    s = ngp.Sampler(device=0, seed=5, chain=0, **kw)
    s.set_panel(G, centre=True)
    Gp = codes(Np, Pw)
    s.set_prediction_panel(Gp, centre=True)
    add_sets(s, [(0, 4400, "PR"), (4400, 100, "B")], v)
    s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var()); s.set_schedule(*sched)
    sets = [(0, 4400), (4400, 100)]
    assert RP.chunks(0, 4400) == [(0, 2048), (2048, 4096), (4096, 4400)]
    X, mean = stored(s, Gp)
    s1, s2, lasts, _ = run_and_restate(s, X, mean, sets, 6, sched)
    assert len(lasts) == 2 and all(np.array_equal(a, b) for a, b in lasts)
    ps = s.prediction_sums()
    assert np.array_equal(ps["sum"], s1) and np.array_equal(ps["sum2"], s2) and np.abs(s1[0]).max() > 0


def test_centring_uses_the_training_means_and_weights_never_scale(ngp, O):
    """The training rows themselves as the prediction panel give ngp_xbeta(beta): the two sums run over the same stored values in
    different orders, each within ref_predict.bound of the exact sum.  Under residual weights the training tiles are row-scaled, the
    prediction tiles are not: the prediction is the restatement on the unscaled values bit for bit, and ngp_xbeta (which divides the
    scale out again after the fp32 rounding of s x: two relative roundings of 2^-24 per element) agrees to 2^-22 sum |x| |beta|."""
    N = 300
    G, y, v = make_codes(O, N, P)
    sets = [(0, 100), (100, 92), (256, 74)]
    for weighted in (False, True):
        s = ngp.Sampler(device=0, seed=9, chain=0)
        if weighted:
            s.set_residual_weights(np.random.default_rng(3).uniform(0.25, 4.0, size=N))
        s.set_panel(G, centre=True)
        s.set_prediction_panel(G, centre=True)
        add_sets(s, SPEC_R, v)
        s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var()); s.set_schedule(4, 2, 2)
        s.run(4)
        beta = s.get_state()["beta"]
        X = RP.stored_f32(G, s.means())
        last = s.prediction_last()
        assert np.array_equal(last, RP.predict_draw(X, beta, sets))
        xb = s.xbeta(beta)
        B = RP.bound(X, beta, sets)[3]
        if weighted:
            assert np.all(np.abs(last[3] - xb) <= 2.0 ** -22 * (np.abs(X) @ np.abs(beta)) + 2 * B)
        else:
            assert np.all(np.abs(last[3] - xb) <= 2 * B)
        # means of the prediction rows are never used: other rows, the same centring
        s.set_prediction_panel(G[:40] + (G[:40] == 0), centre=True)
        s.set_y(y); s.run(4)
        X2 = RP.stored_f32(G[:40] + (G[:40] == 0), s.means())
        assert np.array_equal(s.prediction_last(), RP.predict_draw(X2, s.get_state()["beta"], sets))


def fused_chains(ngp, O, K, kw, N, shards, share_first):
    G, y, v = make_codes(O, N, P)
    Gp = codes(63)
    chains = []
    for c in range(K):
        s = ngp.Sampler(device=0, seed=1001 + c, chain=c, **kw)
        if c == 0:
            s.set_max_shards(shards if shards else s.shards_for_pass(K))
            s.set_panel(G, centre=True)
            if not share_first:
                s.set_prediction_panel(Gp, centre=True)
        else:
            s.share_panel(chains[0])
        chains.append(s)
    if share_first:                      # the owner sets it after the others took the panel: they see it all the same
        chains[0].set_prediction_panel(Gp, centre=True)
    for c, s in enumerate(chains):
        add_sets(s, SPEC_R, v)
        s.set_y(y + 0.01 * c); s.set_residual_prior(4.0, 1.0); s.set_schedule(20, 4, 2)
    return chains, G, Gp, y, v


@pytest.mark.parametrize("name,K,kw,N,shards", [("phase", 2, dict(), 500, 0), ("phase", 3, dict(mode=1, lag=6), 500, 0), ("phase", 8, dict(), 500, 0),
                                                ("rows", 2, dict(mode=1, lag=6), 700, 6), ("bytes", 2, dict(mode=1, lag=8, storage="u8"), 500, 0)],
                         ids=["phase2", "phase3", "phase8", "rows2", "bytes2"])
def test_fused_chains_share_one_prediction_pass(ngp, O, name, K, kw, N, shards):
    """ngp_run_many over K chains that share the panel: ONE prediction launch per kept iteration serves all of them (the leader
    counts nKept launches and K nKept chains served, the others none), the prediction panel is uploaded once, and every chain's sums
    are bit for bit what the chain accumulates alone."""
    chains, G, Gp, y, v = fused_chains(ngp, O, K, kw, N, shards, share_first=(K == 2))
    R, S, _ = chains[0].layout()
    ngp.Sampler.run_many(chains, 20)
    assert chains[0].prediction_stats() == (8, 8 * K)               # (only a fused call leaves the leader with every chain's share)
    for s in chains[1:]:
        assert s.prediction_stats() == (0, 0) and s.prediction_layout() == chains[0].prediction_layout()
    for c in (0, K - 1):
        alone = ngp.Sampler(device=0, seed=1001 + c, chain=c, **kw)
        alone.set_max_shards(S); alone.set_panel(G, centre=True)
        assert alone.layout()[:2] == (R, S)
        alone.set_prediction_panel(Gp, centre=True)
        add_sets(alone, SPEC_R, v)
        alone.set_y(y + 0.01 * c); alone.set_residual_prior(4.0, 1.0); alone.set_schedule(20, 4, 2)
        alone.run(20)
        assert alone.prediction_stats() == (8, 8)
        assert np.array_equal(alone.get_state()["beta"], chains[c].get_state()["beta"])
        a, f = alone.prediction_sums(), chains[c].prediction_sums()
        assert a["nKept"] == f["nKept"] == 8 and np.array_equal(a["sum"], f["sum"]) and np.array_equal(a["sum2"], f["sum2"])
        assert np.array_equal(alone.prediction_last(), chains[c].prediction_last())
    assert not np.array_equal(chains[0].prediction_sums()["sum"], chains[1].prediction_sums()["sum"])


def small(ngp, O, seed=21, sched=(20, 4, 2), Np=63, spec=SPEC_R):
    G, y, v = make_codes(O, 300, P)
    s = ngp.Sampler(device=0, seed=seed, chain=0)
    s.set_panel(G, centre=True)
    s.set_prediction_panel(codes(Np), centre=True)
    add_sets(s, spec, v)
    s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var()); s.set_schedule(*sched)
    return s, G, y, v


def test_only_kept_iterations_accumulate(ngp, O):
    """Nothing during burn-in or on thinned-out iterations; a sweep whose census fails (ngp_debug_fail_census) is run again and its
    iteration counts once: the sums equal an undisturbed handle's."""
    s, *_ = small(ngp, O)
    s.run(5)                                                   # burn-in 4, thin 2: iteration 6 is the first kept one
    assert s.prediction_stats() == (0, 0) and not s.prediction_sums()["sum"].any() and not s.prediction_last().any()
    s.run(1)
    assert s.prediction_stats() == (1, 1) and s.prediction_sums()["sum"].any()
    one = s.prediction_sums()
    s.run(1)                                                   # iteration 7: thinned out
    assert s.prediction_stats() == (1, 1) and np.array_equal(s.prediction_sums()["sum"], one["sum"])
    s.run(13)
    ref = s.prediction_sums()
    assert ref["nKept"] == 8 and s.prediction_stats() == (8, 8)
    for fail_at in (7, 10, 20):                                # a thinned-out iteration, a kept one inside the queue, the last one
        d, *_ = small(ngp, O)
        d.debug_fail_census(fail_at)
        d.run(20)
        assert d.census()["retries"] == 1
        ps = d.prediction_sums()
        assert ps["nKept"] == 8 and np.array_equal(ps["sum"], ref["sum"]) and np.array_equal(ps["sum2"], ref["sum2"])
        assert d.prediction_stats() == (8, 8)
    s.set_y(np.zeros(300) + 1.0)                               # zeroed wherever sum_beta is
    assert not s.prediction_sums()["sum"].any() and not s.prediction_sums()["sum2"].any()


def test_set_prediction_then_continue_equals_an_uninterrupted_run(ngp, O):
    """The sums travel beside a snapshot: get_state / get_posterior_sums / prediction_sums of a chain half-way, set on a fresh handle."""
    whole, *_ = small(ngp, O, sched=(12, 2, 2), spec=SPEC)
    whole.run(12)
    a, G, y, v = small(ngp, O, sched=(12, 2, 2), spec=SPEC)
    a.run(6)
    st, post, ps = a.get_state(), a.get_posterior_sums(), a.prediction_sums()
    b, *_ = small(ngp, O, sched=(12, 2, 2), spec=SPEC)
    b.set_state(st); b.set_posterior_sums(post)
    b.set_prediction_sums(ps)
    b.run(6)
    w, r = whole.prediction_sums(), b.prediction_sums()
    assert np.array_equal(whole.get_state()["beta"], b.get_state()["beta"])
    assert w["nKept"] == r["nKept"] == 5 and np.array_equal(w["sum"], r["sum"]) and np.array_equal(w["sum2"], r["sum2"])
    with pytest.raises(ngp.NextGPHipError, match="error -1"):
        b._chk(b.L.ngp_set_prediction(b.h, None, None, C.c_int64(3), C.c_int64(63)))


def test_a_new_training_panel_drops_the_prediction_panel(ngp, O):
    s, G, y, v = small(ngp, O)
    s.run(6)
    assert s.prediction_sums()["nKept"] == 1
    s.set_panel(G, centre=True)
    s.nsets = 0                                                # (a new panel is a new model; the Python mirror counts the sets it added)
    with pytest.raises(ngp.NextGPHipError, match="error -2"):
        s.prediction_layout()
    add_sets(s, SPEC_R, v)
    s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var()); s.set_schedule(20, 4, 2)
    s.run(6)                                                   # runs as a handle that never had one
    assert s.prediction_stats() == (0, 0)
    with pytest.raises(ngp.NextGPHipError, match="error -2"):
        s.prediction_sums()


def test_refusals_leave_a_handle_that_still_runs(ngp, O):
    G, y, v = make_codes(O, 300, P)
    Gp = codes(20)
    s = ngp.Sampler(device=0, seed=3, chain=0)
    with pytest.raises(ngp.NextGPHipError, match="error -2"):    # no training panel
        s.begin_prediction_panel(20)
    s.begin_panel(300, P)
    with pytest.raises(ngp.NextGPHipError, match="error -2"):    # the training panel is still open
        s.begin_prediction_panel(20)
    s.panel_columns(0, G, centre=True)
    s.end_panel()
    with pytest.raises(ngp.NextGPHipError, match="error -1"):    # Np < 1
        s.begin_prediction_panel(0)
    with pytest.raises(ngp.NextGPHipError, match="error -2"):    # columns without an open prediction panel
        s.prediction_columns(0, Gp)
    s.begin_prediction_panel(20)
    with pytest.raises(ngp.NextGPHipError, match="error -1"):    # columns outside [0, P)
        s.prediction_columns(P - 10, Gp[:, :11])
    with pytest.raises(ngp.NextGPHipError, match="error -1"):
        s.prediction_columns(-1, Gp[:, :5])
    with pytest.raises(ngp.NextGPHipError, match="error -2"):    # any other call between begin and end
        s.layout()
    with pytest.raises(ngp.NextGPHipError, match="error -2"):
        s.set_y(y)
    s.prediction_columns(0, Gp, centre=True)
    s.end_prediction_panel()
    with pytest.raises(ngp.NextGPHipError, match="error -2"):    # ended already
        s.end_prediction_panel()
    g = ngp.Sampler(device=0, seed=3, chain=0)
    g.set_records(300)
    with pytest.raises(ngp.NextGPHipError, match="error -2"):    # a records-only (GBLUP) handle
        g.begin_prediction_panel(20)
    u = ngp.Sampler(device=0, seed=3, chain=0, storage="u8")
    u.set_panel(G, centre=True)
    u.begin_prediction_panel(20)
    with pytest.raises(ngp.NextGPHipError, match="error -1"):    # byte tiles take codes only
        u.prediction_columns(0, Gp.astype(np.float64))
    u.prediction_columns(0, Gp, centre=True)
    u.end_prediction_panel()
    for m in (s, u):
        add_sets(m, SPEC_R, v)
        m.set_y(y); m.set_residual_prior(4.0, 0.25 * y.var()); m.set_schedule(6, 2, 2)
        m.run(6)
        X, mean = stored(m, Gp)
        assert np.array_equal(m.prediction_last(), RP.predict_draw(X, m.get_state()["beta"], [(0, 100), (100, 92), (256, 74)], mean))
        with pytest.raises(ngp.NextGPHipError, match="error -1"):    # the arrays are [nsets + 1][Np]
            m._chk(m.L.ngp_get_prediction_last(m.h, np.zeros(80).ctypes.data_as(C.POINTER(C.c_double)), C.c_int64(4), C.c_int64(19)))


def test_prediction_file_of_either_width(ngp, O, tmp_path):
    """ngp_load_prediction_file (NGPPNL01, 8 and 2 bits) gives the tiles of the same codes uploaded as columns."""
    G, y, v = make_codes(O, 300, P)
    Gp = codes(63)
    out = []
    for how in ("columns", 8, 2):
        s = ngp.Sampler(device=0, seed=4, chain=0)
        s.set_panel(G, centre=True)
        if how == "columns":
            s.set_prediction_panel(Gp, centre=True)
        else:
            ngp.write_panel_file(str(tmp_path / f"p{how}.ngp"), Gp, bits=how)
            s.load_prediction_file(tmp_path / f"p{how}.ngp", centre=True)
        add_sets(s, SPEC_R, v)
        s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var()); s.set_schedule(4, 2, 2)
        s.run(4)
        out.append(s.prediction_sums())
    assert out[0]["sum"].any()
    for o in out[1:]:
        assert np.array_equal(o["sum"], out[0]["sum"]) and np.array_equal(o["sum2"], out[0]["sum2"])
    ngp.write_panel_file(str(tmp_path / "narrow.ngp"), Gp[:, :100], bits=8)
    with pytest.raises(ngp.NextGPHipError, match="error -1"):
        s.load_prediction_file(tmp_path / "narrow.ngp")
    s.run(0)


# ---- runLMEM(predict=...) ------------------------------------------------------------------------------------------------------------
def test_runlmem_predict_end_to_end(ngp, O, tmp_path):
    """200 x 192 in two SNP terms, the candidates from an array and an .npy file: gebvPredict.txt read back is res["predict"], which is
    the summary of the device's own sums; chains=2 pools the chains' sums; and the *Out files of a run without predict= are byte for
    byte those of the run with it (the prediction panel observes the chain and never touches it)."""
    N, Pm, Np = 200, 192, 50
    G, y, v = make_codes(O, N, Pm)
    Gp = codes(Np, Pm)
    ga, gb = tmp_path / "a.txt", tmp_path / "b.txt"
    np.savetxt(ga, G[:, :100], fmt="%d", delimiter=" ")
    np.savetxt(gb, G[:, 100:], fmt="%d", delimiter=" ")
    np.save(tmp_path / "pB.npy", Gp[:, 100:])
    f = f'y ~ 1 + SNP(M1,"{ga}") + SNP(M2,"{gb}")'
    VCV = {"M1": ngp.BayesPR(9999, v), "M2": ngp.BayesB(0.2, v, estimatePi=True), "e": ngp.Random("I", 0.25 * y.var())}
    pred = {"M1": Gp[:, :100], "M2": str(tmp_path / "pB.npy")}
    ids = [f"cand{i}" for i in range(Np)]
    plain = ngp.runLMEM(f, {"y": y}, 12, 4, 2, outFolder=str(tmp_path / "plain"), VCV=VCV, seed=7)
    res = ngp.runLMEM(f, {"y": y}, 12, 4, 2, outFolder=str(tmp_path / "with"), VCV=VCV, seed=7, predict=pred, predict_ids=ids)
    assert "predict" not in plain and not (tmp_path / "plain" / "gebvPredict.txt").exists()
    names = sorted(p.name for p in (tmp_path / "plain").iterdir())
    assert sorted(p.name for p in (tmp_path / "with").iterdir()) == sorted(names + ["gebvPredict.txt"])
    for nm in names:
        assert (tmp_path / "plain" / nm).read_bytes() == (tmp_path / "with" / nm).read_bytes(), nm
    pr = res["predict"]
    back = ngp.read_prediction_file(tmp_path / "with" / "gebvPredict.txt")
    head = (tmp_path / "with" / "gebvPredict.txt").read_text().splitlines()[0].split("\t")
    assert head == ["ID", "mean", "sd", "mean_M1", "sd_M1", "mean_M2", "sd_M2"]
    assert back["ids"] == pr["ids"] == ids and pr["nKept"] == 4
    assert np.array_equal(back["mean"], pr["mean"]) and np.array_equal(back["sd"], pr["sd"])
    for nm in ("M1", "M2"):
        assert np.array_equal(back["sets"][nm]["mean"], pr["sets"][nm]["mean"]) and np.array_equal(back["sets"][nm]["sd"], pr["sets"][nm]["sd"])
    smp = res["sampler"]
    ps = smp.prediction_sums()
    assert np.array_equal(pr["mean"], ps["sum"][2] / 4) and np.array_equal(pr["sets"]["M1"]["mean"], ps["sum"][0] / 4)
    assert np.array_equal(pr["sd"], np.sqrt(np.maximum(0.0, ps["sum2"][2] / 4 - (ps["sum"][2] / 4) ** 2))) and pr["sd"].max() > 0
    # two chains: pooled over the chains' sums, each chain's own beside it
    two = ngp.runLMEM(f, {"y": y}, 12, 4, 2, outFolder=str(tmp_path / "two"), VCV=VCV, seed=7, chains=2, predict=pred)
    sums = [sc.prediction_sums() for sc in two["samplers"]]
    assert two["predict"]["nKept"] == 8 and two["predict"]["ids"] == [str(i + 1) for i in range(Np)]
    assert np.array_equal(two["predict"]["mean"], (sums[0]["sum"][2] + sums[1]["sum"][2]) / 8)
    for c in range(2):
        assert np.array_equal(two["chains"][c]["predict"]["mean"], sums[c]["sum"][2] / 4)
    assert (tmp_path / "two" / "gebvPredict.txt").exists() and not np.array_equal(sums[0]["sum"], sums[1]["sum"])
    # storage="u8" takes the same sources as codes
    u8 = ngp.runLMEM(f, {"y": y}, 6, 2, 2, outFolder=str(tmp_path / "u8"), VCV=VCV, seed=7, storage="u8", predict=pred)
    assert u8["predict"]["nKept"] == 2 and np.isfinite(u8["predict"]["sd"]).all()
