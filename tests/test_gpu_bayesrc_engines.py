"""BayesRCpi marker sets on the remaining engines of the persistent sweep: K chains per pass (k_sweep_multi_rc, over the phase streamer,
the row-owning streamer and byte tiles) and fp32 panels so tall that a streamer workgroup owns two or three shards (k_sweep_tall_rc).
A fused chain must be, bit for bit, the chain it is alone with the same layout; a tall chain is held to BayesR where one annotation
makes the two coincide, to tests/ref_bayesrc.py lane by lane, to its one-shard sibling, and to the reference-order chain."""
import os

import numpy as np
import pytest

import ref_bayesrc as RB
from conftest import add_sets, make_problem
from test_gpu_bayesrc import CONFIGS, PI4, REF_SPEC, VC4, integer_problem, make_annot, make_codes

pytestmark = pytest.mark.gpu

NITER, SCHED = 20, (20, 4, 2)
VC3, PI3 = [0.0, 0.05, 1.0], [0.7, 0.2, 0.1]
P_RC = 650                      # ten blocks and a tail of ten lanes; the sets meet inside blocks 3 and 6
RC_SETS = [("rc", 0, 230, 3, VC4, PI4), ("B", 230, 200), ("rc", 430, 220, 2, VC3, PI3)]
PLAIN_SETS = [(0, 300, "PR"), (300, 200, "B"), (500, 150, "R")]      # a chain without a BayesRCpi set, on the same panel


def add_rc_model(s, v):
    """[RC A=3 x 4 classes | BayesB | RC A=2 x 3 classes] on 650 columns; returns the ids of the BayesRCpi sets."""
    ids = []
    for k, spec in enumerate(RC_SETS):
        if spec[0] == "rc":
            _, c0, n, A, vc, pi = spec
            ids.append(s.add_marker_set_rc(c0, n, 4.0, v * 0.5, v, vc, pi, make_annot(n, A, seed=60 + k), estPi=True))
        else:
            s.add_marker_set(spec[1], spec[2], 1, 4.0, v * 0.5, [(j, j + 1) for j in range(spec[2])], [v] * spec[2], pi0=0.05, estPi=True)
    return ids


def add_plain_model(s, v):
    add_sets(s, PLAIN_SETS, v)
    return []


def full_state(s, ids):
    st = dict(s.get_state())
    for sid in ids:
        st.update({f"rc{sid}_{k}": x for k, x in s.rc_state(sid).items()})
    st.update({"post_" + k: x for k, x in s.get_posterior_sums().items()})
    return st


def same(a, b, what=""):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), (what, k)


# ---- the panels, made once -------------------------------------------------------------------------------------------------------------
_panels = {}


def panel(O, engine, N):
    """(what set_panel takes, y, v) of the engine's panel with N rows and P_RC columns."""
    key = (engine, N)
    if key not in _panels:
        if engine == "u8":
            from test_gpu_compact import make_codes as codes
            G, y, v = codes(O, N, P_RC)
            _panels[key] = (G, y, v)
        else:
            X, y, _, v = make_problem(O, N, P_RC, seed=6)
            _panels[key] = (X, y, v)
    return _panels[key]


def new_sampler(ngp, engine, lag, c, seed=None):
    kw = {"mode": 1, "lag": lag} if lag else {}
    if engine == "u8":
        kw["storage"] = "u8"
    return ngp.Sampler(device=0, seed=(2001 + 7 * c) if seed is None else seed, chain=c, **kw)


def finish(s, model, y, v, c):
    ids = model(s, v)
    s.set_y(y + 0.01 * c)              # the chains differ in seed and in y
    s.set_residual_prior(4.0, 1.0)
    s.set_schedule(*SCHED)
    return ids


def fused_chains(ngp, O, engine, N, K, lag, shards=None, models=None):
    M, y, v = panel(O, engine, N)
    chains, ids = [], []
    for c in range(K):
        s = new_sampler(ngp, engine, lag, c)
        if c == 0:
            s.set_max_shards(shards if shards else s.shards_for_pass(K))
            s.set_panel(M, centre=True) if engine == "u8" else s.set_panel(M)
        else:
            s.share_panel(chains[0])
        ids.append(finish(s, (models[c] if models else add_rc_model), y, v, c))
        chains.append(s)
    return chains, ids


# a chain alone: its state behind 20 and behind 25 iterations, computed once per (engine, N, lag, S, chain, model) and left unchanged
_alone = {}


def alone_states(ngp, O, engine, N, lag, S, c, model=add_rc_model, layout=None):
    key = (engine, N, lag, S, c, model.__name__)
    if key not in _alone:
        M, y, v = panel(O, engine, N)
        s = new_sampler(ngp, engine, lag, c)
        s.set_max_shards(S)
        s.set_panel(M, centre=True) if engine == "u8" else s.set_panel(M)
        ids = finish(s, model, y, v, c)
        s.run(NITER)
        at20 = full_state(s, ids)
        grid = s.census()["grid"]
        s.run(5)
        _alone[key] = (at20, full_state(s, ids), s.layout()[:2], grid)
    at20, at25, lay, grid = _alone[key]
    if layout is not None:
        assert lay == layout
    return at20, at25, grid


# ---- fused passes ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,lag", [(2, None), (3, 6), (8, None)])
def test_fused_rc_chains_on_the_phase_streamer(ngp, O, K, lag):
    """1. One launch per iteration serves K chains of the mixed model (grid: K samplers, the reducers -- paired from four chains on --
    and S streamers); the first and the last chain are the chains they are alone, full state; a second call continues them."""
    N = 500
    fused, ids = fused_chains(ngp, O, "f32", N, K, lag)
    R, S, _ = fused[0].layout()
    assert R <= 64 and fused[0].streamer()[0] == 1
    ngp.Sampler.run_many(fused, NITER)
    assert fused[0].census()["grid"] == K + (((K + 1) // 2) if K >= 4 else K) * ((S + 31) // 32) + S
    for c in (0, K - 1):
        same(full_state(fused[c], ids[c]), alone_states(ngp, O, "f32", N, lag, S, c, layout=(R, S))[0], c)
    a, b = fused[0].get_state(), fused[K - 1].get_state()
    assert not np.array_equal(a["beta"], b["beta"]) and not np.array_equal(a["delta"], b["delta"])
    assert len(np.unique(a["delta"][:230])) >= 3 and len(set(fused[0].rc_state(ids[0][0])["annotCat"])) == 3
    ngp.Sampler.run_many(fused, 5)
    assert fused[0].get_state()["iter"] == 25
    for c in (0, K - 1):
        same(full_state(fused[c], ids[c]), alone_states(ngp, O, "f32", N, lag, S, c)[1], c)


@pytest.mark.parametrize("lag", [6, 4])
def test_fused_rc_chains_on_the_row_owning_streamer(ngp, O, lag):
    """2. Two chains over shards of 64+ rows (role_streamer_rows_multi)."""
    N, K = 700, 2
    fused, ids = fused_chains(ngp, O, "f32", N, K, lag, shards=6)
    R, S, _ = fused[0].layout()
    assert fused[0].streamer() == (2, 7) and R >= 64 and fused[0].config() == (1, lag)
    ngp.Sampler.run_many(fused, NITER)
    assert fused[0].census()["grid"] == K * (1 + (S + 31) // 32) + S
    for c in range(K):
        same(full_state(fused[c], ids[c]), alone_states(ngp, O, "f32", N, lag, S, c, layout=(R, S))[0], c)
    assert not np.array_equal(fused[0].get_state()["beta"], fused[1].get_state()["beta"])


@pytest.mark.parametrize("K,lag,N,shards,tasks", [(2, 8, 500, 0, 1), (3, 8, 500, 0, 1), (2, 8, 1500, 6, 2), (2, 6, 2900, 6, 4)],
                         ids=["two_chains", "three_chains", "two_tasks", "four_tasks"])
def test_fused_rc_chains_over_compact_storage(ngp, O, K, lag, N, shards, tasks):
    """3. Two or three chains over byte tiles, with one, two and four update tasks per lane."""
    fused, ids = fused_chains(ngp, O, "u8", N, K, lag, shards=shards)
    R, S, _ = fused[0].layout()
    assert fused[0].streamer() == (3, 7) and fused[1].storage() == 1
    nuw = -(-(R // 16) // 7)
    assert {1: 1, 2: 2, 3: 4, 4: 4}[(4 * nuw + 7) // 8] == tasks
    ngp.Sampler.run_many(fused, NITER)
    assert fused[0].census()["grid"] == K * (1 + (S + 31) // 32) + S
    for c in range(K):
        same(full_state(fused[c], ids[c]), alone_states(ngp, O, "u8", N, lag, S, c, layout=(R, S))[0], c)
    assert not np.array_equal(fused[0].get_state()["beta"], fused[1].get_state()["beta"])


def test_rc_chain_and_plain_chain_in_one_pass(ngp, O):
    """4. Chain 0 holds the BayesRCpi model, chain 1 [PR | B | R] without such a set: one launch, whose samplers take the lanes of chain 1
    through eval_rform; each chain the chain alone."""
    N, K = 500, 2
    models = [add_rc_model, add_plain_model]
    fused, ids = fused_chains(ngp, O, "f32", N, K, None, models=models)
    R, S, _ = fused[0].layout()
    ngp.Sampler.run_many(fused, NITER)
    assert fused[0].census()["grid"] == K * (1 + (S + 31) // 32) + S
    for c in range(K):
        same(full_state(fused[c], ids[c]), alone_states(ngp, O, "f32", N, None, S, c, model=models[c], layout=(R, S))[0], c)
    assert len(np.unique(fused[1].get_state()["delta"][500:])) >= 2      # the BayesR lanes of the plain chain move


def test_three_rc_chains_on_row_owning_shards_run_unfused(ngp, O):
    """5. The fused kernel serves two chains on fp32 row-owning shards: three run side by side, each handle's last grid its own, the
    results those of the chains alone."""
    N, K, lag = 700, 3, 6
    chains, ids = fused_chains(ngp, O, "f32", N, K, lag, shards=6)
    R, S, _ = chains[0].layout()
    assert chains[0].streamer() == (2, 7)
    ngp.Sampler.run_many(chains, NITER)
    for c in range(K):
        assert chains[c].census()["grid"] == 1 + (S + 31) // 32 + S
        at20, _, grid = alone_states(ngp, O, "f32", N, lag, S, c, layout=(R, S))
        assert grid == 1 + (S + 31) // 32 + S
        same(full_state(chains[c], ids[c]), at20, c)


def test_runLMEM_two_fused_chains(ngp, O, tmp_path):
    """6. runLMEM(chains=2) with a BayesRCpi prior at 200 x 192: one fused launch per iteration, and every chain's files (annotMOut
    among them) are byte for byte those of the same call alone with chain=c and the layout of the fused run."""
    from nextgp_jl_amd import api
    N, P, A = 200, 192, 3
    X, y, _, v = make_problem(O, N, P, seed=8)
    X = np.rint(X.astype(np.float64) - X.min(axis=0))
    geno = str(tmp_path / "geno.npy")
    np.save(geno, X)
    prior = api.BayesRCπ(PI4, VC4, v, make_annot(P, A, seed=3), estimatePi=True)
    f, VCV, K = f'y ~ 1 + SNP(M, "{geno}")', {"M": prior, "e": api.Random("I", 1.0)}, 2
    out = tmp_path / "two"
    res = api.runLMEM(f, dict(y=y), 30, 10, 2, outFolder=str(out), VCV=VCV, seed=13, chains=K)
    first = res["samplers"][0]
    R, S, _ = first.layout()
    assert res["fused"] is True and first.census()["grid"] == K + K * ((S + 31) // 32) + S
    for c in range(K):
        alone = tmp_path / f"alone{c}"
        r1 = api.runLMEM(f, dict(y=y), 30, 10, 2, outFolder=str(alone), VCV=VCV, seed=13, chain=c, max_shards=S)
        assert r1["sampler"].layout()[:2] == (R, S)
        cdir = out / f"chain{c}"
        names = sorted(p.name for p in alone.iterdir())
        assert "annotMOut" in names and sorted(p.name for p in cdir.iterdir()) == names
        for pth in alone.iterdir():
            assert pth.read_bytes() == (cdir / pth.name).read_bytes(), (c, pth.name)
        assert np.array_equal(r1["sets"]["M"]["annot"], res["chains"][c]["sets"]["M"]["annot"])
    assert (out / "chain0" / "annotMOut").read_bytes() != (out / "chain1" / "annotMOut").read_bytes()


def test_sample_file_of_a_fused_chain(ngp, O, tmp_path):
    """7. A sample file on one chain of a fused run: the last kept record is that chain's end state, annotCat and annotProb included."""
    N, K = 500, 2
    fused, ids = fused_chains(ngp, O, "f32", N, K, None)
    S = fused[0].layout()[1]
    path = str(tmp_path / "chain1.smp")
    fused[1].set_sample_file(path)
    ngp.Sampler.run_many(fused, NITER)
    fused[1].set_sample_file(None)
    assert fused[0].census()["grid"] == K * (1 + (S + 31) // 32) + S
    end = full_state(fused[1], ids[1])
    smp = ngp.read_sample_file(path)
    assert smp["iter"].tolist() == list(range(6, 21, 2))
    for sid in ids[1]:
        assert np.array_equal(smp["annotCat"][sid][-1], end[f"rc{sid}_annotCat"]) and np.array_equal(smp["annotProb"][sid][-1], end[f"rc{sid}_annotProb"])
    assert np.array_equal(smp["delta"][-1], end["delta"]) and np.array_equal(smp["beta"][-1], end["beta"])
    assert np.array_equal(smp["varBeta"][-1], end["varBeta"]) and smp["varE"][-1] == end["varE"]
    assert np.array_equal(smp["class_pi"][-1], np.concatenate([end[f"rc{sid}_piHat"].ravel() for sid in ids[1]]))
    same(end, alone_states(ngp, O, "f32", N, None, S, 1)[0])


# ---- tall shards -----------------------------------------------------------------------------------------------------------------------
def tall_sampler(ngp, X, V, shards, seed=1001):
    s = ngp.Sampler(device=0, seed=seed, chain=0, mode=1, lag=6, streamer=2 * V)
    s.set_max_shards(shards)
    s.set_panel(X)
    return s


TALL_SHAPES = {2: (1500, 8), 3: (1000, 9)}     # V: (N, max shards), the multi-set shapes of test_several_shards_per_workgroup_bit_exact


@pytest.mark.parametrize("V", [2, 3])
def test_tall_panel_takes_a_bayesrc_set(ngp, O, V):
    """8. add_marker_set_rc on a handle whose streamer workgroups own V shards, and the grid of its sweep."""
    N, shards = TALL_SHAPES[V]
    X, y, _, v = make_problem(O, N, P_RC, seed=5)
    s = tall_sampler(ngp, X, V, shards)
    ids = finish(s, add_rc_model, y, v, 0)
    R, S, _ = s.layout()
    assert s.config() == (1, 5 - V) and s.streamer() == (2, 7) and S % V == 0
    s.run(4)
    assert s.census()["grid"] == 1 + (S + 31) // 32 + S // V
    st = full_state(s, ids)
    assert st["iter"] == 4 and np.isfinite(st["beta"]).all() and len(np.unique(st["delta"][:230])) >= 2
    resid = y - st["b"] - s.xbeta(st["beta"])
    assert np.abs(st["ycorr"] - resid).max() <= 1e-10 * max(1.0, np.abs(y).max())


@pytest.mark.parametrize("V", [2, 3])
def test_tall_one_annotation_is_bayesr(ngp, O, V):
    """9. [PR | RC or R | B], the RC set with one all-ones annotation: the full state is that of the chain added with add_marker_set_r
    on the same tall engine (which the blocked oracle holds), bit for bit, 12 iterations."""
    N, shards = TALL_SHAPES[V]
    P, niter = 450, 12
    X, y, _, v = make_problem(O, N, P, seed=5)
    out = []
    for kind in ("rc", "r"):
        s = tall_sampler(ngp, X, V, shards)
        add_sets(s, [(0, 150, "PR")], v)
        if kind == "rc":
            sid = s.add_marker_set_rc(150, 170, 4.0, v * 0.5, v, VC4, PI4, np.ones((170, 1), dtype=np.int32), estPi=True)
        else:
            sid = s.add_marker_set_r(150, 170, 4.0, v * 0.5, v, VC4, PI4, estPi=True)
        add_sets(s, [(320, 130, "B")], v)
        s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var()); s.set_schedule(niter, 4, 2)
        s.run(niter)
        st = full_state(s, [])
        st.update({"pi_" + k: x for k, x in s.get_class_state(sid).items()})
        if kind == "rc":
            rc = s.rc_state(sid)
            assert np.array_equal(rc["annotProb"], np.ones((170, 1))) and np.all(rc["annotCat"] == 1)
            assert np.array_equal(rc["piHat"].ravel(), st["pi_piHat"])
            assert s.census()["grid"] == 1 + (s.layout()[1] + 31) // 32 + s.layout()[1] // V
        out.append(st)
    assert len(np.unique(out[0]["delta"][150:320])) >= 3
    same(out[0], out[1])


TALL_LANES = [(c, V, c0, n) for c in ("3x5", "8x2") for V in (2, 3) for c0, n in ((0, 330), (128, 64), (320, 10))]


@pytest.mark.parametrize("cfg,V,col0,ncol", TALL_LANES, ids=["-".join(map(str, c)) for c in TALL_LANES])
def test_tall_lane_rule_bit_for_bit(ngp, O, cfg, V, col0, ncol):
    """10. One fine-seam call from beta = 0 on an integer panel swept by k_sweep_tall_rc: the assertions of
    test_gpu_bayesrc.test_lane_rule_bit_for_bit -- the first block the set samples against ref_bayesrc.block_chain, varBeta, pi and
    annotProb behind the sweep against ref_bayesrc.behind_sweep at every locus."""
    A, vc, pi = CONFIGS[cfg]
    N, P, seed = 128, 330, 77
    G, y = integer_problem(N, P, seed=len(cfg) + P)
    an = make_annot(ncol, A, seed=ncol + A + col0)
    s = tall_sampler(ngp, G.astype(np.float32), V, {2: 8, 3: 6}[V], seed=seed)
    assert s.config() == (1, 5 - V) and s.layout()[1] % V == 0
    v, df, varE = 0.02, 4.0, 1.7
    sid = s.add_marker_set_rc(col0, ncol, df, v * 0.5, v, vc, pi, an, estPi=True)
    ycorr, beta, vb = y.copy(), np.zeros(ncol), np.full(A, v)
    delta = s.sweep_set(sid, varE, ycorr, beta, vb)
    assert s.census()["grid"] == 1 + (s.layout()[1] + 31) // 32 + s.layout()[1] // V
    rc = s.rc_state(sid)
    X = G.astype(np.float64)[:, col0:col0 + ncol]
    mpm = (X * X).sum(axis=0)
    n0 = min(ncol, 64)
    Gm = X[:, :n0].T @ X[:, :n0]
    iVarE = 1.0 / varE
    logpi = [[O.det_log(p) for p in pi] for _ in range(A)]
    prob0 = an / an.sum(axis=1, keepdims=True)
    tabs = [RB.lane_tables(O, seed, 0, 1, sid, l, mpm[l], 0.0, iVarE, [v] * A, vc, logpi, prob0[l], an[l]) for l in range(n0)]
    fin = RB.block_chain(O, tabs, list(X[:, :n0].T @ y), Gm, iVarE, [0.0] * n0, [0.0] * n0)
    assert np.array_equal(delta[:n0], [f[0] + 1 for f in fin])
    assert np.array_equal(rc["annotCat"][:n0], [f[1] + 1 for f in fin])
    assert np.array_equal(beta[:n0], np.array([f[2] for f in fin]) + 0.0)
    if n0 == 64:
        assert len(set(rc["annotCat"][:n0])) >= 2 and np.count_nonzero(beta[:n0]) >= 1
    assert all(an[l, rc["annotCat"][l] - 1] == 1 for l in range(ncol))
    rvb, rpi, rprob = RB.behind_sweep(O, seed, 0, 1, sid, beta, delta - 1, rc["annotCat"] - 1, an, df, v * 0.5, vc, A, True)
    assert np.array_equal(vb, rvb)
    assert np.array_equal(rc["piHat"], np.array(rpi))
    assert np.array_equal(rc["annotProb"], rprob)


def test_tall_two_shards_equal_the_one_shard_sibling(ngp, O):
    """11. Two shards per workgroup at lag 3 and the row-owning streamer at lag 3 share layout, shard partials and reducer groups: the
    multi-annotation model is the same chain on both, full state, 12 iterations."""
    N, shards, niter = 1500, 8, 12
    X, y, _, v = make_problem(O, N, P_RC, seed=5)
    tall = tall_sampler(ngp, X, 2, shards)
    sib = ngp.Sampler(device=0, seed=1001, chain=0, mode=1, streamer=2, lag=3)
    sib.set_max_shards(shards); sib.set_panel(X)
    assert tall.layout()[:2] == sib.layout()[:2] and tall.near() == sib.near() and tall.config() == sib.config() == (1, 3)
    assert tall.streamer() == sib.streamer() == (2, 7) and (tall.layout()[1] + 31) // 32 <= 8
    states = []
    for s in (tall, sib):
        ids = add_rc_model(s, v)
        s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var()); s.set_schedule(niter, 4, 2)
        s.run(niter)
        states.append(full_state(s, ids))
    S = tall.layout()[1]
    assert tall.census()["grid"] == 1 + (S + 31) // 32 + S // 2 and sib.census()["grid"] == 1 + (S + 31) // 32 + S
    assert len(np.unique(states[0]["delta"][:230])) >= 3
    same(states[0], states[1])


TALL_REF_SEED = 101   # chosen on the CPU with RCRefChain alone: the smallest relative margin of any comparison of its 12 iterations is 3.6e-5


@pytest.mark.parametrize("V", [2, 3])
def test_tall_reference_order_chain(ngp, O, V):
    """12. The REF_SPEC model of test_gpu_bayesrc.py ([RC 100 | BayesB 90 | RC 100 | BayesPR 40], N = 300) on fp32 tiles swept by
    k_sweep_tall_rc against ref_bayesrc.RCRefChain on the same panel in Float64, 12 iterations: every class and every annotation
    identical at every locus and iteration, beta within 1e-9 of the largest effect (the bound test_chain_vs_reference_order_oracle
    holds fp32 chains to).  Seed 101 was chosen with RCRefChain alone, on the CPU: the smallest relative margin of any comparison of
    the run (annotation search, class search, BayesB inclusion) is 3.6e-5, printed and asserted to be at least 1e-6 -- three orders
    above the bound, so rounding cannot flip a comparison."""
    N, P = 300, 330
    X, G, y, v = make_codes(O, N, P)
    ref = RB.RCRefChain(O, X.astype(np.float64), y, TALL_REF_SEED, 0)
    ref.E_df, ref.E_scale = 4.0, 0.25 * y.var()
    s = tall_sampler(ngp, X, V, {2: 8, 3: 9}[V], seed=TALL_REF_SEED)
    assert s.config() == (1, 5 - V) and s.layout()[1] % V == 0
    ids = []
    for k, spec in enumerate(REF_SPEC):
        if spec[0] == "rc":
            _, c0, n, A, vc, pi = spec
            an = make_annot(n, A, seed=40 + k)
            ref.add_set_rc(c0, n, 4.0, v * 0.5, v, vc, pi, an, estPi=True)
            ids.append(s.add_marker_set_rc(c0, n, 4.0, v * 0.5, v, vc, pi, an, estPi=True))
        else:
            if spec[0] == "B":
                args, kw = (spec[1], spec[2], 1, 4.0, v * 0.5, [(j, j + 1) for j in range(spec[2])], [v] * spec[2]), dict(pi0=0.1, estPi=True)
            else:
                args, kw = (spec[1], spec[2], 0, 4.0, v * 0.5, [(0, spec[2])], [v]), {}
            ref.add_set(*args, **kw); s.add_marker_set(*args, **kw)
            ids.append(None)
    s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var())
    for it in range(12):
        ref.run(1)
        s.run(1)
        st = s.get_state()
        rdelta = np.concatenate(ref.delta)
        assert np.array_equal(st["delta"], rdelta), (it, np.nonzero(st["delta"] != rdelta)[0][:8])
        for k, sid in enumerate(ids):
            if sid is not None:
                assert np.array_equal(s.rc_state(sid)["annotCat"], ref.M[k]["annotCat"]), (it, k)
        rbeta = np.concatenate(ref.beta)
        d = np.abs(st["beta"] - rbeta).max() / np.abs(rbeta).max()
        assert d < 1e-9, (it, d)
    S = s.layout()[1]
    assert s.census()["grid"] == 1 + (S + 31) // 32 + S // V
    print("smallest relative margin of a comparison:", ref.min_margin)
    assert ref.min_margin >= 1e-6
