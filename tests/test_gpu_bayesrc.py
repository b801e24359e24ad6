"""BayesRCpi marker sets on the device (annotation-informed BayesR; include/nextgp_hip.h ngp_add_marker_set_rc, DESIGN.md section 2
"BayesRCpi sets") against tests/ref_bayesrc.py, the numpy restatement of src/functions.jl:291-360, and against the existing BayesR
path where the two must coincide."""
import numpy as np
import pytest

import ref_bayesrc as RB
from conftest import make_problem

pytestmark = pytest.mark.gpu

VC4, PI4 = [0.0, 0.01, 0.1, 1.0], [0.85, 0.10, 0.04, 0.01]


def make_codes(O, N, P, seed=5):
    X, y, bt, v = make_problem(O, N, P, seed=seed)
    _, mu = O.generate_panel(N, P)
    G = np.rint(X.astype(np.float64) + mu[None, :]).astype(np.uint8)
    return X, G, y, v


def make_annot(P, A, seed):
    """Loci with one, some and all annotations (never none)."""
    rng = np.random.default_rng(seed)
    an = (rng.random((P, A)) < 0.5).astype(np.int32)
    an[np.arange(P), rng.integers(0, A, P)] = 1
    an[::7, :] = 1                      # all annotations
    an[1::7, :] = 0
    an[1::7, rng.integers(0, A)] = 1    # exactly one
    return an


def sampler(ngp, X, G, engine, seed=31, chain=0, centre=True):
    if engine == "u8":
        s = ngp.Sampler(device=0, seed=seed, chain=chain, mode=1, lag=8, storage="u8")
        s.set_panel(G, centre=centre)
    else:
        s = ngp.Sampler(device=0, seed=seed, chain=chain, mode=1 if engine == "persistent" else 0, lag=6)
        s.set_panel(X)
    return s


# ---- 1. A = 1 is BayesR ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", ["persistent", "per_block", "u8"])
def test_one_annotation_is_bayesr(ngp, O, engine):
    """One all-ones annotation column: beta, delta, ycorr, varBeta, pi and varE are bit for bit those of the same chain added with
    ngp_add_marker_set_r (N = 400, P = 520: eight full blocks and one of 8 lanes; 15 iterations).  Ties the new path -- eval_rcform,
    k_prep's slot tables, k_rc_count / k_rc_draw -- to the path the oracle checks."""
    N, P, niter = 400, 520, 15
    X, G, y, v = make_codes(O, N, P)
    out = []
    for kind in ("rc", "r"):
        s = sampler(ngp, X, G, engine)
        if kind == "rc":
            sid = s.add_marker_set_rc(0, P, 4.0, v * 0.5, v, VC4, PI4, np.ones((P, 1), dtype=np.int32), estPi=True)
        else:
            sid = s.add_marker_set_r(0, P, 4.0, v * 0.5, v, VC4, PI4, estPi=True)
        s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var()); s.set_schedule(niter, 3, 2)
        s.run(niter)
        st = s.get_state()
        st["pi"] = s.get_class_state(sid)
        st["post"] = s.get_posterior_sums()
        if kind == "rc":
            rc = s.rc_state(sid)
            assert np.array_equal(rc["annotProb"], np.ones((P, 1))) and np.all(rc["annotCat"] == 1)
            assert np.array_equal(rc["sum_annot"][:, 0], np.full(P, float(st["post"]["nKept"])))
            assert np.array_equal(rc["piHat"].ravel(), st["pi"]["piHat"])
        out.append(st)
    a, b = out
    assert len(np.unique(a["delta"])) >= 3          # the chain visits zero and non-zero classes
    for k in ("delta", "beta", "ycorr", "varBeta"):
        assert np.array_equal(a[k], b[k]), k
    assert a["varE"] == b["varE"] and a["b"] == b["b"]
    assert np.array_equal(a["pi"]["piHat"], b["pi"]["piHat"]) and np.array_equal(a["pi"]["sum_pi"], b["pi"]["sum_pi"])
    for k in ("sum_beta", "sum_beta2", "sum_delta", "sum_varBeta"):
        assert np.array_equal(a["post"][k], b["post"][k]), k


# ---- 2. the lane's rule, bit for bit ---------------------------------------------------------------------------------------------
CONFIGS = {"2x2": (2, [0.0, 1.0], [0.8, 0.2]), "2x4": (2, VC4, PI4), "3x5": (3, [0.0, 0.001, 0.01, 0.1, 1.0], [0.7, 0.1, 0.1, 0.06, 0.04]),
           "8x2": (8, [0.05, 1.0], [0.9, 0.1])}


def integer_problem(N, P, seed):
    """Genotype counts 0 / 1 / 2, NOT centred, and an integer-valued residual: every x'ycorr and x'x is an integer, exact in fp64 in
    whatever order a kernel adds it (fixed-point sums included), so the numpy side knows r of the first block bit for bit."""
    rng = np.random.default_rng(seed)
    G = rng.binomial(2, rng.uniform(0.1, 0.5, P), size=(N, P)).astype(np.uint8)
    y = rng.integers(-6, 7, N).astype(np.float64)
    return G, y


# every configuration at both widths on the persistent sweep over fp32 tiles; the per-block engine and the byte tiles run the same
# eval_rcform: the single-block panel in every configuration, and the widest configuration at 330 loci.  (col0, ncol): where the set
# lies on the P-column panel.  A sweep from beta = 0 over an integer residual has exact totals only in the FIRST block it samples, so
# the blocks behind the first of the 330-column panel are reached by sets that start there: a whole block in the middle (columns
# 128..191) and the 10-lane tail block (columns 320..329, beside 54 lanes nobody owns).
LANE_CASES = [(c, P, "persistent", 0, P) for c in CONFIGS for P in (64, 330)] + [(c, 64, e, 0, 64) for c in CONFIGS for e in ("per_block", "u8")] + \
             [("3x5", 330, "per_block", 0, 330), ("3x5", 330, "u8", 0, 330)] + \
             [(c, 330, "persistent", c0, n) for c in CONFIGS for c0, n in ((128, 64), (320, 10))] + \
             [("3x5", 330, e, c0, n) for e in ("per_block", "u8") for c0, n in ((192, 64), (320, 10))]


@pytest.mark.parametrize("cfg,P,engine,col0,ncol", LANE_CASES, ids=["-".join(map(str, c)) for c in LANE_CASES])
def test_lane_rule_bit_for_bit(ngp, O, cfg, P, engine, col0, ncol):
    """One fine-seam call from beta = 0 on an integer panel.  Class, annotation and dlt of every lane of the first block the set
    samples against ref_bayesrc.block_chain -- block 0, a middle block or the partial tail block of the panel, by where the set lies
    (behind its first block a sweep's totals depend on the engine's summation order once ycorr holds fractions; whole multi-block
    chains are held to the reference-order ref and, with one annotation, to BayesR); varBeta, pi and annotProb behind the sweep against
    ref_bayesrc.behind_sweep from what the sweep left at EVERY locus of the set.  All bit for bit."""
    A, vc, pi = CONFIGS[cfg]
    N, seed = 128, 77
    G, y = integer_problem(N, P, seed=len(cfg) + P)
    an = make_annot(ncol, A, seed=ncol + A + col0)
    s = sampler(ngp, G.astype(np.float32), G, engine, seed=seed, centre=False)
    v, df, varE = 0.02, 4.0, 1.7
    sid = s.add_marker_set_rc(col0, ncol, df, v * 0.5, v, vc, pi, an, estPi=True)
    ycorr, beta, vb = y.copy(), np.zeros(ncol), np.full(A, v)
    delta = s.sweep_set(sid, varE, ycorr, beta, vb)
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
    assert all(an[l, rc["annotCat"][l] - 1] == 1 for l in range(ncol))       # never an annotation the locus lacks
    rvb, rpi, rprob = RB.behind_sweep(O, seed, 0, 1, sid, beta, delta - 1, rc["annotCat"] - 1, an, df, v * 0.5, vc, A, True)
    assert np.array_equal(vb, rvb)
    assert np.array_equal(rc["piHat"], np.array(rpi))
    assert np.array_equal(rc["annotProb"], rprob)


# ---- 4. the law on the device ------------------------------------------------------------------------------------------------------
def test_annotation_and_class_frequencies_follow_the_exact_law(ngp, O):
    """128 x 64 panel of mutually orthogonal zero-sum columns (a Hadamard matrix without its ones column) in fp32, every fine-seam
    call from beta = 0 and the same residual: the right-hand side of every locus is known in advance and does not depend on the other
    loci.  Replicates by the call's iteration key.  The (annotation, class) of every locus and replicate goes through the randomised
    probability integral transform of its exact joint law (ref_bayesrc.locus_law); the bound is the KS condition of tests/pivots.py."""
    from scipy import stats
    import pivot_models as PM
    H = np.array([[1.0]])
    while H.shape[0] < 128:
        H = np.block([[H, H], [H, -H]])
    X = np.asfortranarray(H[:, 1:65], dtype=np.float32)
    A, vc, pi = 3, [0.0, 0.05, 1.0], [0.6, 0.3, 0.1]
    P, K = 64, 3
    an = make_annot(P, A, seed=4)
    rng = np.random.default_rng(12)
    y = X.astype(np.float64) @ (rng.normal(size=P) * 0.12) + rng.normal(size=128) * 0.3
    s = ngp.Sampler(device=0, seed=PM.SEED, chain=0)
    s.set_panel(X)
    v, varE = 0.02, 0.4
    sid = s.add_marker_set_rc(0, P, 4.0, v * 0.5, v, vc, pi, an, estPi=False)
    prob0 = an / an.sum(axis=1, keepdims=True)
    rhs = (X.astype(np.float64).T @ y) / varE
    laws = [RB.locus_law(rhs[l], 128.0 / varE, [v] * A, vc, [pi] * A, prob0[l]) for l in range(P)]
    us, cnt = [], np.zeros((A, K))
    for rep in range(120):
        s.set_rc_state(sid, dict(annotProb=prob0, piHat=np.tile(pi, (A, 1))))
        ycorr, beta, vb = y.copy(), np.zeros(P), np.full(A, v)
        delta = s.sweep_set(sid, varE, ycorr, beta, vb)
        cat = s.rc_state(sid)["annotCat"]
        for l in range(P):
            pa, pc = laws[l]
            joint = (pa[:, None] * pc).ravel()
            F = np.concatenate([[0.0], np.cumsum(joint)])
            i = (cat[l] - 1) * K + (delta[l] - 1)
            assert joint[i] > 0.0, (l, i)
            us.append(F[i] + rng.uniform() * (F[i + 1] - F[i]))
            cnt[cat[l] - 1, delta[l] - 1] += 1
    p = float(stats.kstest(us, "uniform").pvalue)
    print("annotation x class counts", cnt.tolist(), "KS p", p)
    assert p > PM.KS_MIN, p
    assert (cnt.sum(axis=1) > 0).all() and (cnt.sum(axis=0) > 0).all()


# ---- 5. state ------------------------------------------------------------------------------------------------------------------------
def rc_model(ngp, O, engine="persistent", seed=5, chain=0):
    N, P = 300, 200
    X, G, y, v = make_codes(O, N, P)
    s = sampler(ngp, X, G, engine, seed=seed, chain=chain)
    an = make_annot(120, 3, seed=9)
    s.add_marker_set(0, 80, 0, 4.0, v * 0.5, [(0, 80)], [v])
    sid = s.add_marker_set_rc(80, 120, 4.0, v * 0.5, v, VC4, PI4, an, estPi=True)
    s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var())
    return s, sid


def full_state(s, sid):
    st = s.get_state()
    st.update({"rc_" + k: v for k, v in s.rc_state(sid).items()})
    st.update(s.get_posterior_sums())
    return st


def same(a, b):
    for k in a:
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k


def test_snapshot_resume_get_set_state_and_sample_file(ngp, O, tmp_path):
    s, sid = rc_model(ngp, O)
    s.set_schedule(12, 2, 2)
    s.run(6)
    snap = str(tmp_path / "rc.snap")
    s.save_snapshot(snap)
    mid, mid_rc, mid_post = s.get_state(), s.rc_state(sid), s.get_posterior_sums()
    s.set_sample_file(str(tmp_path / "rc.smp"))
    s.run(6)
    s.set_sample_file(None)
    end = full_state(s, sid)
    assert end["varBeta"].shape == (1 + 3,) and end["rc_sum_annot"].sum() == 120 * end["nKept"]
    assert s.posterior_len() == 3 * 200 + 4 + 2 * 2 + 3 * 4 + 3 * 120 + 3
    # the sample file: the last kept record is the end state
    smp = ngp.read_sample_file(str(tmp_path / "rc.smp"))
    assert smp["iter"].tolist() == [8, 10, 12] and smp["sets"][sid]["rcA"] == 3 and smp["sets"][sid]["rcK"] == 4
    assert np.array_equal(smp["annotCat"][sid][-1], end["rc_annotCat"]) and np.array_equal(smp["annotProb"][sid][-1], end["rc_annotProb"])
    assert np.array_equal(smp["delta"][-1], end["delta"]) and np.array_equal(smp["beta"][-1], end["beta"])
    assert np.array_equal(smp["varBeta"][-1], end["varBeta"]) and np.array_equal(smp["class_pi"][-1], end["rc_piHat"].ravel())
    # resumed from the snapshot: bit for bit the uninterrupted chain
    t, tid = rc_model(ngp, O)
    t.set_schedule(12, 2, 2)
    t.load_snapshot(snap)
    t.run(6)
    same(end, full_state(t, tid))
    # ... and from get / set state
    u, uid = rc_model(ngp, O)
    u.set_schedule(12, 2, 2)
    u.set_state(mid); u.set_rc_state(uid, mid_rc); u.set_posterior_sums(mid_post)
    u.run(6)
    same(end, full_state(u, uid))
    # a model without the set refuses the snapshot (its signature holds method, slots and annotations)
    N, P = 300, 200
    X, G, y, v = make_codes(O, N, P)
    z = sampler(ngp, X, G, "persistent", seed=5)
    z.add_marker_set(0, 80, 0, 4.0, v * 0.5, [(0, 80)], [v])
    z.add_marker_set_r(80, 120, 4.0, v * 0.5, v, VC4, PI4, estPi=True)
    z.set_y(y)
    with pytest.raises(Exception):
        z.load_snapshot(snap)
    # ... and so does the same model over OTHER annotations of the same shape: the signature digests the masks (a loaded annotProb
    # is positive exactly where the mask it was saved under has a bit)
    q = sampler(ngp, X, G, "persistent", seed=5)
    q.add_marker_set(0, 80, 0, 4.0, v * 0.5, [(0, 80)], [v])
    q.add_marker_set_rc(80, 120, 4.0, v * 0.5, v, VC4, PI4, make_annot(120, 3, seed=10), estPi=True)
    q.set_y(y)
    with pytest.raises(Exception):
        q.load_snapshot(snap)


def test_two_chains_side_by_side_and_pooled_sums(ngp, O):
    alone = []
    for c in (0, 1):
        s, sid = rc_model(ngp, O, chain=c)
        s.set_schedule(8, 2, 2)
        s.run(8)
        alone.append(full_state(s, sid))
    pair = [rc_model(ngp, O, chain=c) for c in (0, 1)]
    for s, _ in pair:
        s.set_schedule(8, 2, 2)
    type(pair[0][0]).run_many([p[0] for p in pair], 8)
    for (s, sid), ref in zip(pair, alone):
        same(ref, full_state(s, sid))
    type(pair[0][0]).allreduce_posterior([p[0] for p in pair])
    for s, sid in pair:
        assert np.array_equal(s.rc_state(sid)["sum_annot"], alone[0]["rc_sum_annot"] + alone[1]["rc_sum_annot"])
        assert np.array_equal(s.rc_state(sid)["sum_pi"], alone[0]["rc_sum_pi"] + alone[1]["rc_sum_pi"])


def test_refusals_leave_a_handle_that_still_runs(ngp, O):
    N, P = 300, 200
    X, G, y, v = make_codes(O, N, P)
    s = sampler(ngp, X, G, "persistent")
    an = make_annot(P, 2, seed=1)
    bad = an.copy(); bad[17, :] = 0
    with pytest.raises(Exception, match="no annotation"):
        s.add_marker_set_rc(0, P, 4.0, v * 0.5, v, VC4, PI4, bad)
    two = an.copy(); two[3, 0] = 2
    with pytest.raises(Exception, match="0 or 1"):
        s.add_marker_set_rc(0, P, 4.0, v * 0.5, v, VC4, PI4, two)
    with pytest.raises(Exception, match="A \\* K <= 16"):
        s.add_marker_set_rc(0, P, 4.0, v * 0.5, v, [0.0, 0.001, 0.01, 0.1, 1.0], [0.2] * 5, make_annot(P, 4, seed=2))
    sid = s.add_marker_set_rc(0, P, 4.0, v * 0.5, v, VC4, PI4, an)
    assert sid == 0
    with pytest.raises(Exception, match="BayesRCpi"):          # time stamps and timing modes live in a kernel without the set's rule
        s.debug_stamps(True)
    with pytest.raises(Exception, match="BayesRCpi"):
        s.debug_set_mode(2)
    s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var())
    s.run(3)
    st = s.get_state()
    assert st["iter"] == 3 and np.isfinite(st["beta"]).all() and st["varBeta"].shape == (2,)


# ---- 3. reference order ----------------------------------------------------------------------------------------------------------
REF_SEED = 101   # chosen on the CPU with RCRefChain: the smallest relative margin of any comparison of its 12 iterations is 3.6e-5
REF_SPEC = [("rc", 0, 100, 3, VC4, PI4), ("B", 100, 90), ("rc", 190, 100, 2, [0.0, 0.05, 1.0], [0.7, 0.2, 0.1]), ("PR", 290, 40)]


def reference_order_model(O, seed, device=None):
    """[RC 100 | BayesB 90 | RC 100 | BayesPR 40] on N = 300 byte genotypes: the reference-order chain on g - mean in Float64 (device
    None), or the same model on a handle."""
    N, P = 300, 330
    X, G, y, v = make_codes(O, N, P)
    if device is None:
        mu = G.sum(axis=0, dtype=np.int64).astype(np.float64) / float(N)
        m = RB.RCRefChain(O, G.astype(np.float64) - mu[None, :], y, seed, 0)
        m.E_df, m.E_scale = 4.0, 0.25 * y.var()
    else:
        m = device
        m.set_panel(G, centre=True)
    ids = []
    for k, spec in enumerate(REF_SPEC):
        if spec[0] == "rc":
            _, c0, n, A, vc, pi = spec
            an = make_annot(n, A, seed=40 + k)
            ids.append(m.add_set_rc(c0, n, 4.0, v * 0.5, v, vc, pi, an, estPi=True) if device is None
                       else m.add_marker_set_rc(c0, n, 4.0, v * 0.5, v, vc, pi, an, estPi=True))
        elif spec[0] == "B":
            args = (spec[1], spec[2], 1, 4.0, v * 0.5, [(j, j + 1) for j in range(spec[2])], [v] * spec[2])
            (m.add_set if device is None else m.add_marker_set)(*args, pi0=0.1, estPi=True)
            ids.append(None)
        else:
            args = (spec[1], spec[2], 0, 4.0, v * 0.5, [(0, spec[2])], [v])
            (m.add_set if device is None else m.add_marker_set)(*args)
            ids.append(None)
    if device is not None:
        m.set_y(y); m.set_residual_prior(4.0, 0.25 * y.var())
    return m, ids


def test_reference_order_chain(ngp, O):
    """Compact storage, RC lanes beside BayesB and BayesPR lanes in one block and two RC sets in one model, 12 iterations against the
    reference-order chain: every class and every annotation identical at every locus and iteration, beta within the bound
    tests/test_gpu_compact.py holds the compact chain to against the reference's Float64 arithmetic (1e-11 of the largest effect).
    The seed was chosen with the ref so that no comparison of the run (annotation search, class search, BayesB inclusion) has a
    relative margin below 1e-9 -- the smallest of the run is printed and asserted; rounding differences of ~1e-13 cannot flip one."""
    ref, _ = reference_order_model(O, REF_SEED)
    s = ngp.Sampler(device=0, seed=REF_SEED, chain=0, mode=1, lag=8, storage="u8")
    s, ids = reference_order_model(O, REF_SEED, device=s)
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
        assert d < 1e-11, (it, d)
    print("smallest relative margin of a comparison:", ref.min_margin)
    assert ref.min_margin >= 1e-9
    for k, sid in enumerate(ids):
        if sid is not None:
            rc = s.rc_state(sid)
            assert np.allclose(rc["piHat"], ref.M[k]["piHat"], rtol=1e-9, atol=0) and np.allclose(rc["annotProb"], ref.M[k]["annotProb"], rtol=1e-9, atol=0)
    assert np.allclose(st["varBeta"], np.concatenate(ref.varBeta), rtol=1e-9, atol=0) and abs(st["varE"] - ref.varE) < 1e-10 * ref.varE


# ---- 6. runLMEM end to end ---------------------------------------------------------------------------------------------------------
def test_runLMEM_end_to_end(ngp, O, tmp_path):
    """200 x 192 with a BayesRCπ prior: the four files with their pinned headers read back, and res[...] their column means."""
    import os
    from nextgp_jl_amd import api
    N, P, A = 200, 192, 3
    X, y, _, v = make_problem(O, N, P, seed=8)
    X = np.rint(X.astype(np.float64) - X.min(axis=0))
    geno = str(tmp_path / "geno.npy")
    np.save(geno, X)
    an = make_annot(P, A, seed=3)
    prior = api.BayesRCπ(PI4, VC4, v, an, estimatePi=True)
    out = str(tmp_path / "out")
    nChain, nBurn, nThin = 30, 10, 2
    res = api.runLMEM(f'y ~ 1 + SNP(M, "{geno}")', dict(y=y), nChain, nBurn, nThin, outFolder=out, VCV={"M": prior, "e": api.Random("I", 1.0)}, seed=13)
    head = lambda n: open(os.path.join(out, n)).readline().rstrip("\n").split("\t")
    assert head("piMOut") == [f"pi{i + 1}" for i in range(A * 4)] and head("varMOut") == [f"reg_{a + 1}" for a in range(A)]
    assert head("annotMOut") == [f"M{j + 1}" for j in range(P)] and head("deltaMOut") == [f"M{j + 1}" for j in range(P)]
    rows = lambda n: np.loadtxt(os.path.join(out, n), delimiter="\t", skiprows=1, ndmin=2)
    cat, dl, pim, vm = rows("annotMOut"), rows("deltaMOut"), rows("piMOut"), rows("varMOut")
    nk = (nChain - nBurn) // nThin
    assert cat.shape == (nk, P) and dl.shape == (nk, P) and pim.shape == (nk, A * 4) and vm.shape == (nk, A)
    assert set(np.unique(cat)) <= {1.0, 2.0, 3.0} and all(an[j, int(c) - 1] == 1 for row in cat for j, c in enumerate(row))
    assert set(np.unique(dl)) <= {1.0, 2.0, 3.0, 4.0} and np.allclose(pim.reshape(nk, A, 4).sum(axis=2), 1.0, rtol=1e-12)
    M = res["sets"]["M"]
    assert np.allclose(M["pi"].ravel(), pim.mean(axis=0), rtol=1e-12) and np.allclose(M["var"], vm.mean(axis=0), rtol=1e-12)
    member = np.stack([(cat == a + 1).mean(axis=0) for a in range(A)], axis=1)
    assert np.allclose(M["annot"], member, atol=1e-12) and np.allclose(M["annot"].sum(axis=1), 1.0)
    assert np.allclose(api.summaryMCMC("annotM", outFolder=out)[0], cat.mean(axis=0))
    res2 = api.runLMEM(f'y ~ 1 + SNP(M, "{geno}")', dict(y=y), nChain, nBurn, nThin, outFolder=str(tmp_path / "two"),
                       VCV={"M": prior, "e": api.Random("I", 1.0)}, seed=13, chains=2)
    assert len(res2["chains"]) == 2 and res2["sets"]["M"]["annot"].shape == (P, A)      # (side by side: no fused kernel carries the rule)
    assert np.allclose(res2["sets"]["M"]["annot"].sum(axis=1), 1.0) and os.path.exists(os.path.join(str(tmp_path / "two"), "chain1", "annotMOut"))
    with pytest.raises(NotImplementedError, match="362-419"):
        api.BayesRCplus(PI4, VC4, v, an)
