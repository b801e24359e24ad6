"""Genomic variance per kept draw on the device (include/nextgp_hip.h, "genomic variance"; DESIGN.md section 2, "Genomic variance"):
behind every kept iteration one pass over the training tiles forms var_i (X beta)_i per window, per marker set and in all, q = V / V_g,
r = V_g / (V_g + varE) and the WPPA indicator.  The reference has no such step; what is checked here is the arithmetic DESIGN.md
fixes, restated in tests/ref_genvar.py, bit for bit."""
import numpy as np
import pytest

import ref_genvar as RG
from conftest import add_sets
from test_gpu_compact import make_codes
from test_gpu_predict import ENGINES, P, SCHED, SETS_TUPLE, SPEC_R, add_model, kept

pytestmark = pytest.mark.gpu

# set 0 (columns 0..99): a single column, 60..70 across the edge of block 0, and a window that ends at the set's last column inside
# block 1, which set 1 shares; between them gaps.  Set 1 (100..191): no windows at all.  Set 2 (256..329, Tuple or BayesR): one window.
WINDOWS = [[(0, 1), (60, 70), (90, 100)], [], [(10, 74)]]
THR = 0.05


def build(ngp, O, engine, N=None, seed=1001, chain=0, sched=SCHED, windows=WINDOWS, thr=THR, trace_rows=0, shards=None, y_shift=0.0):
    kw, N0, sh, tuple_set = ENGINES[engine]
    N = N or N0
    G, y, v = make_codes(O, N, P)
    s = ngp.Sampler(device=0, seed=seed, chain=chain, **kw)
    if shards or sh:
        s.set_max_shards(shards or sh)
    s.set_panel(G, centre=True)
    add_model(s, v, tuple_set)
    for k, w in enumerate(windows):
        s.set_variance_windows(k, w)
    s.enable_genomic_variance(True, thr, trace_rows)
    s.set_y(y + y_shift); s.set_residual_prior(4.0, 0.25 * max(y.var(), 0.1)); s.set_schedule(*sched)
    return s, G, y, v


def stored(s, G):
    if s.storage() == 1:
        return G.astype(np.float64), s.means()
    return RG.stored_f32(G, s.means()), None


def run_and_restate(s, G, sets, windows, niter, sched=SCHED, thr=THR, trace_rows=0):
    X, mean = stored(s, G)
    n = sum(len(w) for w in windows) + len(sets) + 1
    S = RG.Sums(n, thr, trace_rows)
    lasts = []
    for it in range(1, niter + 1):
        s.run(1)
        if kept(it, sched):
            st = s.get_state()
            V, _ = RG.draw(X, st["beta"], sets, windows, mean)
            S.add(V, float(st["varE"]))
            lasts.append((V, s.genomic_variance_last()))
    return S, lasts


def same_sums(gs, S):
    return (gs["nKept"] == S.n and all(np.array_equal(gs[k], S.a[i]) for i, k in enumerate(("sumV", "sumV2", "sumQ", "sumQ2", "count", "last")))
            and np.array_equal(gs["ratio"], S.ratio))


@pytest.mark.parametrize("N", [2, 5, 67, 300])
@pytest.mark.parametrize("engine", ["persistent", "perblock", "u8"])
def test_bit_for_bit_against_the_restatement(ngp, O, engine, N):
    """genomic_variance_last() after every kept iteration and all sums after 12 iterations with schedule (12, 4, 2) equal
    tests/ref_genvar.py bit for bit.  N = 67 is a multiple of neither 4 nor 16: padding rows add nothing."""
    s, G, y, v = build(ngp, O, engine, N, trace_rows=3)
    assert s.genomic_variance_layout()[:3] == (8, 4, 3)
    S, lasts = run_and_restate(s, G, SETS_TUPLE, WINDOWS, 12, trace_rows=3)
    assert len(lasts) == 4
    for V, last in lasts:
        assert np.array_equal(last, V)
    assert lasts[-1][0][-1] > 0 and np.isfinite(S.a).all()
    assert same_sums(s.genomic_variance_sums(), S)
    assert s.genomic_variance_stats() == (4, 4)
    assert s.genomic_variance_layout() == (8, 4, 3, 3, 1)             # three rows traced, the fourth draw counted
    tV, tr = s.genomic_variance_trace()
    assert np.array_equal(tV, np.array(S.trV)) and np.array_equal(tr, np.array(S.trR))
    out = s.genomic_variance()
    assert out["names"] == ["set0:win_1", "set0:win_2", "set0:win_3", "set2:win_1", "set0", "set1", "set2", "total"]
    assert np.array_equal(out["wppa"], S.a[4] / 4) and out["meanQ"][-1] == 1.0


def test_bit_for_bit_on_tall_shards(ngp, O):
    """Several shards per streamer workgroup (all-padding shards at the end of the panel included), at that engine's own N."""
    s, G, y, v = build(ngp, O, "tall")
    S, lasts = run_and_restate(s, G, SETS_TUPLE, WINDOWS, 8, sched=SCHED)
    assert len(lasts) == 2 and all(np.array_equal(a, b) for a, b in lasts)
    assert same_sums(s.genomic_variance_sums(), S)


@pytest.mark.parametrize("engine", ["persistent", "u8"])
def test_a_window_longer_than_32_blocks(ngp, O, engine):
    """P = 2200 and one window of 2100 columns: an item of its own, as long as it needs to be."""
    Pw, sched = 2200, (4, 2, 2)
    G, y, v = make_codes(O, 100, Pw)
    s = ngp.Sampler(device=0, seed=5, chain=0, **ENGINES[engine][0])
    s.set_panel(G, centre=True)
    add_sets(s, [(0, 2180, "PR"), (2180, 20, "B")], v)
    s.set_variance_windows(0, [(50, 2150)])
    s.enable_genomic_variance(True, THR)
    s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var()); s.set_schedule(*sched)
    sets, windows = [(0, 2180), (2180, 20)], [[(50, 2150)], []]
    assert RG.items(RG.segments(0, 2180, windows[0])) == [[0], [1], [2]]
    S, lasts = run_and_restate(s, G, sets, windows, 4, sched)
    assert len(lasts) == 1 and np.array_equal(lasts[0][0], lasts[0][1]) and lasts[0][0][0] > 0
    assert same_sums(s.genomic_variance_sums(), S)


@pytest.mark.parametrize("engine,shards", [("persistent", (6, 3)), ("u8", (5, 2))])
def test_layout_independence(ngp, O, engine, shards):
    """The same model and seed at N = 700 on two layouts with different R (set_max_shards; the second byte layout has shards of more
    than 256 rows, which several workgroups serve): on each, every slot of every kept draw and all sums are the bits of the ONE
    restatement, which knows no layout -- no floating-point tree over the shards takes part.  (The sweep itself draws other effects
    on another layout, and the pass runs only behind a sweep, so the two layouts never hold the same draw to compare directly: the
    layout-free restatement is the common term.)"""
    runs = []
    for sh in shards:
        s, G, y, v = build(ngp, O, engine, 700, shards=sh)
        S, lasts = run_and_restate(s, G, SETS_TUPLE, WINDOWS, 8)
        assert len(lasts) == 2 and all(np.array_equal(a, b) for a, b in lasts) and same_sums(s.genomic_variance_sums(), S)
        runs.append((s.layout()[0], s.get_state()["beta"], s.genomic_variance_sums()))
    assert runs[0][0] != runs[1][0] and max(runs[0][0], runs[1][0]) > (256 if engine == "u8" else 128)


def test_zero_genomic_variance_gives_zero_shares(ngp, O):
    """V_g == 0: every q and r is 0 and nothing is non-finite.  A sweep always draws effects, so the state handed over holds zero
    effects AND variance components of 1e-300: the effects of the next draw are of the order 1e-150, their row sums lie below the
    smallest scale (E is clamped at -400) and every V of the draw is exactly 0 -- on the device as in the restatement."""
    G, y, v = make_codes(O, 300, P)
    s = ngp.Sampler(device=0, seed=7, chain=0)
    s.set_panel(G, centre=True)
    add_sets(s, [(0, 100, "PR"), (100, 92, "PR")], v)
    s.set_variance_windows(0, WINDOWS[0])
    s.enable_genomic_variance(True, 0.0, 1)                            # threshold 0: any q > 0 would count
    s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var()); s.set_schedule(1, 0, 1)
    st = s.get_state()
    st["beta"][:] = 0.0; st["varBeta"][:] = 1e-300
    s.set_state(st)
    s.run(1)
    beta = s.get_state()["beta"]
    assert np.abs(beta).max() < 1e-100
    V, E = RG.draw(RG.stored_f32(G, s.means()), beta, [(0, 100), (100, 92)], [WINDOWS[0], []])
    assert not V.any()
    gs = s.genomic_variance_sums()
    assert gs["nKept"] == 1
    for k in ("sumV", "sumV2", "sumQ", "sumQ2", "count", "last", "ratio"):
        assert np.isfinite(gs[k]).all() and not gs[k].any(), k
    tV, tr = s.genomic_variance_trace()
    assert not tV.any() and not tr.any()


def fused(ngp, O, K, other_windows_for=None):
    G, y, v = make_codes(O, 500, P)
    chains = []
    for c in range(K):
        s = ngp.Sampler(device=0, seed=1001 + c, chain=c)
        if c == 0:
            s.set_max_shards(s.shards_for_pass(K))
            s.set_panel(G, centre=True)
        else:
            s.share_panel(chains[0])
        add_sets(s, SPEC_R, v)
        for k, w in enumerate(WINDOWS):
            s.set_variance_windows(k, w if c != other_windows_for else [(0, 5)])
        s.enable_genomic_variance(True, THR, 2)
        s.set_y(y + 0.01 * c); s.set_residual_prior(4.0, 1.0); s.set_schedule(20, 4, 2)
        chains.append(s)
    return chains, G, y, v


def test_fused_chains_share_one_variance_pass(ngp, O):
    """ngp_run_many over three chains that share the panel, sets and windows: ONE pass per kept iteration serves all of them (the
    leader counts nKept launches and 3 nKept chains, the others none) and every chain is bit for bit what it computes alone; a
    fourth chain with other windows launches its own."""
    chains, G, y, v = fused(ngp, O, 4, other_windows_for=3)
    R, S, _ = chains[0].layout()
    ngp.Sampler.run_many(chains, 20)
    assert chains[0].genomic_variance_stats() == (8, 24)
    assert chains[1].genomic_variance_stats() == (0, 0) and chains[2].genomic_variance_stats() == (0, 0)
    assert chains[3].genomic_variance_stats() == (8, 8)
    for c in (0, 2, 3):
        alone = ngp.Sampler(device=0, seed=1001 + c, chain=c)
        alone.set_max_shards(S); alone.set_panel(G, centre=True)
        assert alone.layout()[:2] == (R, S)
        add_sets(alone, SPEC_R, v)
        for k, w in enumerate(WINDOWS):
            alone.set_variance_windows(k, w if c != 3 else [(0, 5)])
        alone.enable_genomic_variance(True, THR, 2)
        alone.set_y(y + 0.01 * c); alone.set_residual_prior(4.0, 1.0); alone.set_schedule(20, 4, 2)
        alone.run(20)
        assert alone.genomic_variance_stats() == (8, 8)
        assert np.array_equal(alone.get_state()["beta"], chains[c].get_state()["beta"])
        a, f = alone.genomic_variance_sums(), chains[c].genomic_variance_sums()
        assert a["nKept"] == f["nKept"] == 8 and all(np.array_equal(a[k], f[k]) for k in a) and a["sumV"][-1] > 0
        ta, tf = alone.genomic_variance_trace(), chains[c].genomic_variance_trace()
        assert np.array_equal(ta[0], tf[0]) and np.array_equal(ta[1], tf[1]) and ta[0].shape == (2, a["sumV"].size)
    assert not np.array_equal(chains[0].genomic_variance_sums()["sumV"], chains[1].genomic_variance_sums()["sumV"])


def test_only_kept_iterations_accumulate(ngp, O):
    """Nothing during burn-in or on thinned-out iterations; a sweep whose census fails (ngp_debug_fail_census) is run again and its
    iteration counts once: the sums equal an undisturbed handle's."""
    sched = (20, 4, 2)
    s, *_ = build(ngp, O, "persistent", sched=sched)
    s.run(5)                                                   # burn-in 4, thin 2: iteration 6 is the first kept one
    z = s.genomic_variance_sums()
    assert s.genomic_variance_stats() == (0, 0) and z["nKept"] == 0 and not z["sumV"].any() and not z["last"].any()
    s.run(1)
    assert s.genomic_variance_stats() == (1, 1) and s.genomic_variance_sums()["sumV"].any()
    one = s.genomic_variance_sums()
    s.run(1)                                                   # iteration 7: thinned out
    assert s.genomic_variance_stats() == (1, 1) and np.array_equal(s.genomic_variance_sums()["sumV"], one["sumV"])
    s.run(13)
    ref = s.genomic_variance_sums()
    assert ref["nKept"] == 8 and s.genomic_variance_stats() == (8, 8)
    d, *_ = build(ngp, O, "persistent", sched=sched)
    d.debug_fail_census(9)                                     # the sweep of iteration 9 ends at its census once; 10 is a kept one
    d.run(20)
    got = d.genomic_variance_sums()
    assert d.genomic_variance_stats() == (8, 8) and got["nKept"] == 8
    assert all(np.array_equal(got[k], ref[k]) for k in ref)


def test_set_y_zeroes_and_set_then_continue(ngp, O):
    """ngp_set_y zeroes the sums; get -> set -> continue equals the uninterrupted run."""
    sched = (20, 4, 2)
    a, G, y, v = build(ngp, O, "persistent", sched=sched)
    a.run(20)
    ref = a.genomic_variance_sums()
    b, *_ = build(ngp, O, "persistent", sched=sched)
    b.run(12)
    mid, state = b.genomic_variance_sums(), b.get_state()
    assert mid["nKept"] == 4
    b.set_y(y)
    z = b.genomic_variance_sums()
    assert z["nKept"] == 0 and not z["sumV"].any() and not z["ratio"].any() and not z["count"].any()
    c, *_ = build(ngp, O, "persistent", sched=sched)
    c.run(12)
    c.set_variance_windows(0, WINDOWS[0])                       # (setting windows zeroes this chain's sums as well)
    assert c.genomic_variance_sums()["nKept"] == 0
    c.set_genomic_variance_sums(mid)
    c.run(8)
    got = c.genomic_variance_sums()
    assert got["nKept"] == 8 and all(np.array_equal(got[k], ref[k]) for k in ref)


def test_refusals(ngp, O):
    E = ngp.NextGPHipError
    G, y, v = make_codes(O, 300, P)
    s = ngp.Sampler(device=0, seed=1, chain=0)
    with pytest.raises(E, match="-3|finished training panel"):
        s.enable_genomic_variance(True, 0.01)
    s.set_panel(G, centre=True)
    add_sets(s, SPEC_R, v)
    for bad in ([(5, 5)], [(10, 20), (15, 30)], [(20, 30), (0, 10)], [(90, 101)], [(-1, 3)]):
        with pytest.raises(E, match="ascending, disjoint, non-empty"):
            s.set_variance_windows(0, bad)
    with pytest.raises(E, match="no marker set 3"):
        s.set_variance_windows(3, [(0, 1)])
    with pytest.raises(E, match="no marker set -1"):
        s.set_variance_windows(-1, [(0, 1)])
    for thr in (-0.1, 1.5, float("nan")):
        with pytest.raises(E, match="threshold"):
            s.enable_genomic_variance(True, thr)
    with pytest.raises(E, match="no genomic variance"):
        s.genomic_variance_sums()
    s.enable_genomic_variance(True, 0.01)
    n = s.genomic_variance_layout()[0]
    assert n == 4
    with pytest.raises(E, match="nslots = 4"):
        s._chk(s.L.ngp_get_genomic_variance(s.h, None, None, None, None, None, None, 5, None, None))
    gs = s.genomic_variance_sums()
    with pytest.raises(E, match="nslots = 4"):
        s.set_genomic_variance_sums({k: (np.zeros(3) if k not in ("ratio", "nKept") else gs[k]) for k in gs})
    # the handle still runs
    s.set_y(y); s.set_residual_prior(4.0, 1.0); s.set_schedule(4, 2, 2); s.run(4)
    assert s.genomic_variance_sums()["nKept"] == 1
    s.enable_genomic_variance(False)
    with pytest.raises(E, match="no genomic variance"):
        s.genomic_variance_sums()
    s.run(2)
    # residual weights: the tiles hold row-scaled values
    w = ngp.Sampler(device=0, seed=1, chain=0)
    w.set_residual_weights(np.random.default_rng(3).uniform(0.25, 4.0, size=300))
    w.set_panel(G, centre=True)
    with pytest.raises(E, match="residual weights"):
        w.enable_genomic_variance(True, 0.01)
    # a single individual
    one = ngp.Sampler(device=0, seed=1, chain=0)
    one.set_panel(G[:1], centre=False)
    with pytest.raises(E, match="two individuals"):
        one.enable_genomic_variance(True, 0.01)
    # a records-only (GBLUP) handle has no marker panel: NGP_ERR_STATE from both calls, and the handle still runs
    g = ngp.Sampler(device=0, seed=3, chain=0)
    g.set_records(300)
    with pytest.raises(E, match="error -2.*records-only"):
        g.enable_genomic_variance(True, 0.01)
    with pytest.raises(E, match="error -2"):
        g.set_variance_windows(0, [(0, 1)])
    g.add_random_set(np.arange(300) % 10, 10, df=4.0, varU0=1.0)
    g.set_y(y); g.set_residual_prior(4.0, 1.0); g.set_schedule(4, 2, 2); g.run(4)
    assert g.get_state()["iter"] == 4 and g.genomic_variance_stats() == (0, 0)


def lmem(ngp, problem, tmp_path, name, **kw):
    G, y, v = problem
    np.save(tmp_path / "a.npy", G[:, :200]); np.save(tmp_path / "b.npy", G[:, 200:])
    f = f'y ~ 1 + SNP(M1,"{tmp_path / "a.npy"}") + SNP(M2,"{tmp_path / "b.npy"}")'
    vc = {"M1": ngp.BayesPR(9999, v), "M2": ngp.BayesPR(9999, v), "e": ngp.Random("I", 0.25 * y.var())}
    out = tmp_path / name
    return ngp.runLMEM(f, {"y": y}, 12, 4, 2, VCV=vc, outFolder=str(out), seed=7, **kw), out


def test_runlmem_windows_end_to_end(ngp, O, tmp_path):
    """runLMEM(windows=...) at N = 300, P = 330: the files and res["variance"] agree with summaryMCMC of the trace files to rtol 1e-12
    (the means are the same sums divided by the same count; the text rows carry every digit); chains=2 pools the chains' sums and
    writes each chain's files under chain<c>/; windows={} with genomicVariance=True gives the set and total slots only."""
    problem = make_codes(O, 300, P)
    wins = {"M1": 64, "M2": [(0, 1), (60, 70), (100, 130)]}
    res, out = lmem(ngp, problem, tmp_path, "one", windows=wins, windowThreshold=0.05)
    var = res["variance"]
    assert var["nKept"] == 4 and var["threshold"] == 0.05 and list(var["sets"]) == ["M1", "M2"]
    w1, w2 = var["sets"]["M1"]["windows"], var["sets"]["M2"]["windows"]
    assert list(w1["first"]) == [1, 65, 129, 193] and list(w1["last"]) == [64, 128, 192, 200]
    assert list(w2["first"]) == [1, 61, 101] and list(w2["last"]) == [1, 70, 130]
    hd = lambda nm: open(out / nm).readline().rstrip("\n").split("\t")
    assert hd("windowVarM1Out") == ["win_1", "win_2", "win_3", "win_4"] and hd("windowVarM2Out") == ["win_1", "win_2", "win_3"]
    assert hd("genVarOut") == ["M1", "M2", "total", "ratio"]
    assert hd("gwasM1.txt") == ["window", "firstSNP", "lastSNP", "meanV", "meanQ", "sdQ", "WPPA"]
    m1, m2, gv = ngp.summaryMCMC("windowVarM1", str(out))[0], ngp.summaryMCMC("windowVarM2", str(out))[0], ngp.summaryMCMC("genVar", str(out))[0]
    assert np.allclose(w1["meanV"], m1, rtol=1e-12, atol=0) and np.allclose(w2["meanV"], m2, rtol=1e-12, atol=0)
    assert np.allclose([var["sets"]["M1"]["meanV"], var["sets"]["M2"]["meanV"], var["total"]["meanV"], var["ratio"]["mean"]], gv, rtol=1e-12, atol=0)
    assert var["total"]["meanV"] > 0 and 0 < var["ratio"]["mean"] < 1 and len(np.loadtxt(out / "genVarOut", skiprows=1)) == 4
    gw = np.loadtxt(out / "gwasM2.txt", skiprows=1)
    assert gw.shape == (3, 7) and np.array_equal(gw[:, 3], w2["meanV"]) and np.array_equal(gw[:, 6], w2["wppa"]) and np.array_equal(gw[:, 1:3], [[1, 1], [61, 70], [101, 130]])
    tV = np.loadtxt(out / "windowVarM2Out", skiprows=1); tG = np.loadtxt(out / "genVarOut", skiprows=1)
    q = tV / tG[:, 2:3]
    assert np.allclose(w2["meanQ"], q.mean(axis=0), rtol=1e-12, atol=0) and np.array_equal(w2["wppa"], (q > 0.05).mean(axis=0))
    # two chains: pooled sums, per-chain files
    res2, out2 = lmem(ngp, problem, tmp_path, "two", windows=wins, windowThreshold=0.05, chains=2)
    v2 = res2["variance"]
    assert v2["nKept"] == 8 and len(res2["chains"]) == 2 and res2["chains"][0]["variance"]["nKept"] == 4
    rows = np.concatenate([np.loadtxt(out2 / f"chain{c}" / "windowVarM1Out", skiprows=1) for c in (0, 1)])
    assert rows.shape == (8, 4) and np.allclose(v2["sets"]["M1"]["windows"]["meanV"], rows.mean(axis=0), rtol=1e-12, atol=0)
    gr = np.concatenate([np.loadtxt(out2 / f"chain{c}" / "genVarOut", skiprows=1) for c in (0, 1)])
    assert np.allclose([v2["total"]["meanV"], v2["ratio"]["mean"]], gr.mean(axis=0)[2:], rtol=1e-12, atol=0)
    assert (out2 / "gwasM1.txt").exists() and not (out2 / "chain0" / "gwasM1.txt").exists()
    assert not np.array_equal(res2["chains"][0]["variance"]["sets"]["M1"]["windows"]["meanV"], res2["chains"][1]["variance"]["sets"]["M1"]["windows"]["meanV"])
    # set and total slots only
    res3, out3 = lmem(ngp, problem, tmp_path, "three", windows={}, genomicVariance=True)
    assert len(res3["variance"]["sets"]["M1"]["windows"]["meanV"]) == 0 and res3["variance"]["total"]["meanV"] > 0
    assert (out3 / "genVarOut").exists() and not (out3 / "windowVarM1Out").exists() and not (out3 / "gwasM1.txt").exists()
    res4, _ = lmem(ngp, problem, tmp_path, "four")
    assert "variance" not in res4
