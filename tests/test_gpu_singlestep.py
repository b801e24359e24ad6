"""Single-step GBLUP on the device: the corner block D = G_w^-1 - A22^-1 (ngp_grm_single_step), the hybrid random-effect set
(ngp_add_random_set_hybrid: a CSR S plus a dense block on the last levels) and runLMEM's Random("H", v) route.  Yardsticks:
tests/ref_singlestep.py (hybrid_step: the device's documented order, bit for bit; h_inverse: the dense H^-1 in numpy) and the two
existing engines (ngp_add_random_set_dense on the embedded K, ngp_add_random_set on a K both can take).  Nothing here times anything."""
import os

import numpy as np
import pytest

import ref_gblup as RG
import ref_pedigree as RP
import ref_random as RR
import ref_singlestep as RS

pytestmark = pytest.mark.gpu

P_GENO = 400      # columns of every genotype matrix here: G has full rank (plus the ridge) for n_g <= 130
_cache = {}


def _api():
    from nextgp_jl_amd import api
    return api


def _build(s, M, method=1):
    s.grm_begin(M.shape[0], method)
    s.grm_columns(M)
    s.grm_end()
    return s.grm_get()


def _problem(ngp, O, hd, nd, seed=0):
    """A pedigree of q = hd + nd animals, nd of them genotyped; S = A^-1 renumbered (genotyped last), D = G_w^-1 - A22^-1 in numpy."""
    key = (hd, nd, seed)
    if key not in _cache:
        api = _api()
        q = hd + nd
        rng = np.random.default_rng(100 + 7 * hd + nd + seed)
        if q > 2:
            s_, d_ = RP.random_pedigree(q, max(2, q // 6), seed=3 + seed)
            gpos = rng.permutation(q)[:nd]
        else:                                                           # (1, 1): a founder and its genotyped offspring
            s_, d_, gpos = np.array([0, 1], dtype=np.int32), np.zeros(2, dtype=np.int32), np.array([1])
        F, Ainv = ngp.pedigree_ainv(s_, d_)
        perm = api.single_step_order(q, gpos)
        S = api.permute_csr(Ainv, perm)
        A22 = ngp.pedigree_a22(s_, d_, F, gpos)
        G, _ = RG.make_g(RG.hw_genotypes(O, nd, P_GENO, seed=11 + nd), 1) if nd > 1 else (np.array([[1.3]]), None)
        D = np.linalg.inv(0.95 * G + 0.05 * A22) - np.linalg.inv(A22)
        D = (D + D.T) / 2.0
        _cache[key] = dict(q=q, S=S, rows=RP.csr_rows(*S), D=D, A22=A22, gpos=gpos, perm=perm, sire=s_, dam=d_, F=F, Ainv=Ainv)
    return _cache[key]


# ---- 1. the corner block ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ng", [65, 130])
def test_grm_single_step(ngp, O, ng):
    s_, d_ = RP.random_pedigree(300, 20)
    F, _ = ngp.pedigree_ainv(s_, d_)
    gpos = np.random.default_rng(ng).permutation(300)[:ng]
    A22 = ngp.pedigree_a22(s_, d_, F, gpos)
    M = RG.hw_genotypes(O, ng, P_GENO, seed=ng)
    w = 0.05
    s = ngp.Sampler(device=0)
    G = _build(s, M)
    s.grm_single_step(A22, w)
    D = s.grm_get()
    Gw = (1.0 - w) * G + w * A22
    res = np.abs((D + np.linalg.inv(A22)) @ Gw - np.eye(ng)).max()
    print(f"single-step corner n_g={ng}: max |(D + inv(A22)) G_w - I| = {res:.3e}; cond(G_w) {np.linalg.cond(Gw):.3e}, cond(A22) {np.linalg.cond(A22):.3e}")
    assert res < 1e-8
    assert np.array_equal(D, D.T)
    with pytest.raises(ngp.NextGPHipError, match="error -2"):          # the matrix is D now, not a G to blend or invert
        s.grm_single_step(A22, w)
    with pytest.raises(ngp.NextGPHipError, match="error -2"):          # ... and no inverse of a G for the dense engine
        s.set_records(ng); s.add_random_set_dense(None, ng)
    s.close()


def test_grm_single_step_refusals_leave_a_usable_handle(ngp, O):
    ng = 65
    s_, d_ = RP.random_pedigree(300, 20)
    F, _ = ngp.pedigree_ainv(s_, d_)
    A22 = ngp.pedigree_a22(s_, d_, F, np.arange(200, 200 + ng))
    M = RG.hw_genotypes(O, ng, P_GENO, seed=4)
    s = ngp.Sampler(device=0)
    with pytest.raises(ngp.NextGPHipError, match="error -2"):          # nothing begun
        s.grm_N = ng; s.grm_single_step(A22, 0.05)
    s.grm_begin(ng, 1)
    s.grm_columns(M)
    with pytest.raises(ngp.NextGPHipError, match="error -2"):          # before ngp_grm_end
        s.grm_single_step(A22, 0.05)
    s.grm_end()
    asym = A22.copy(); asym[3, 40] += 1e-9
    nonfinite = A22.copy(); nonfinite[5, 5] = np.inf
    notpd = A22.copy(); notpd[10, 10] = -1.0
    for bad, w in ((asym, 0.05), (nonfinite, 0.05), (notpd, 0.05), (A22, 1.0), (A22, -0.01), (A22, float("nan"))):
        with pytest.raises(ngp.NextGPHipError, match="error -1"):
            s.grm_single_step(bad, w)
        with pytest.raises(ngp.NextGPHipError, match="error -2"):      # the matrix is dropped
            s.grm_get()
        G = _build(s, M)                                                # the handle builds on
    s.grm_single_step(A22, 0.0)                                         # w = 0 is in range: D = inv(G) - inv(A22)
    D = s.grm_get()
    assert np.abs((D + np.linalg.inv(A22)) @ G - np.eye(ng)).max() < 1e-8
    s.close()


# ---- 2. fine seam, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("hd,nd", [(0, 64), (1, 1), (5, 63), (70, 65), (300, 130)])
def test_hybrid_fine_seam_bit_exact(ngp, O, hd, nd, weighted):
    """Three consecutive steps (old and new values mix) under the serial and the scheduled head engine against the restatement."""
    pr = _problem(ngp, O, hd, nd)
    q, nrec = pr["q"], 90
    rng = np.random.default_rng(4 + q)
    level = rng.integers(0, q, size=nrec)
    w = rng.uniform(0.3, 3.0, nrec) if weighted else None
    rs = np.sqrt(w) if weighted else None
    y0, u0 = rng.normal(size=nrec) * 3.0, rng.normal(size=q)
    out = {}
    for mode in ((1, 2) if hd > 0 else (0,)):
        s = ngp.Sampler(device=0, seed=77, chain=2)
        if weighted:
            s.set_residual_weights(w)
        s.set_records(nrec)
        s.add_random_set(rng.integers(0, 5, size=nrec), 5)             # a first set: the hybrid one's keys carry set id 1
        rid = s.add_random_set_hybrid(level, q, pr["S"], nd, D=pr["D"], df=4.0, scale=0.4, varU0=0.8)
        assert rid == 1
        if hd > 0:
            s.set_random_schedule(rid, mode)
            info = s.get_random_schedule(rid)
            assert info["engine"] == mode and info["depths"] >= 1 and info["launches"] >= 1
        else:
            with pytest.raises(ngp.NextGPHipError, match="head rows"):
                s.set_random_schedule(rid, 2)
            assert s.get_random_schedule(rid)["engine"] == 0
        ycorr, u, varU, calls = y0.copy(), u0.copy(), 0.8, []
        for _ in range(3):
            varU = s.sample_random_set(rid, 1.3, ycorr, u, varU)
            calls.append((ycorr.copy(), u.copy(), varU))
        out[mode] = calls
        s.close()
    modes = list(out)
    for a, b in zip(out[modes[0]], out[modes[-1]]):                     # the bits are the same under both engines
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    zpz = RR.zpz_of(level, q, w)
    ycorr, u, varU = y0, u0, 0.8
    for it in range(3):
        yt_in = ycorr * rs if weighted else ycorr
        yt, u, varU = RS.hybrid_step(O, 77, 2, it + 1, 1, yt_in, None if rs is None else list(rs), level, q, pr["rows"], nd, pr["D"], zpz, u, varU,
                                     1.3, 4.0, 0.4)
        ycorr = yt / rs if weighted else yt
        got = out[modes[0]][it]
        assert np.array_equal(got[1], u), it
        assert got[2] == varU, it
        assert np.array_equal(got[0], ycorr), it


def test_corner_block_taken_from_the_builder_is_the_host_one(ngp, O):
    """D == None takes the handle's own corner block (S_tt added on the device); a host copy of the same D (S_tt added on the host) gives
    the same bits, and the builder is empty afterwards."""
    pr = _problem(ngp, O, 70, 65)
    q, nd, nrec = pr["q"], 65, 80
    rng = np.random.default_rng(9)
    level = rng.integers(0, q, size=nrec)
    M = RG.hw_genotypes(O, nd, P_GENO, seed=8)
    a = ngp.Sampler(device=0, seed=3, chain=0)
    a.set_records(nrec)
    _build(a, M)
    a.grm_single_step(pr["A22"], 0.05)
    D = a.grm_get()
    with pytest.raises(ngp.NextGPHipError, match="error -1"):          # another size than nd: refused, the block stays
        a.add_random_set_hybrid(level, q, pr["S"], nd - 1)
    ra = a.add_random_set_hybrid(level, q, pr["S"], nd, df=4.0, scale=0.4, varU0=0.8)
    with pytest.raises(ngp.NextGPHipError, match="error -2"):          # consumed
        a.grm_get()
    b = ngp.Sampler(device=0, seed=3, chain=0)
    b.set_records(nrec)
    with pytest.raises(ngp.NextGPHipError, match="error -2"):          # no corner block on this handle
        b.add_random_set_hybrid(level, q, pr["S"], nd)
    rb = b.add_random_set_hybrid(level, q, pr["S"], nd, D=D, df=4.0, scale=0.4, varU0=0.8)
    y0, u0 = rng.normal(size=nrec), rng.normal(size=q)
    res = []
    for s, rid in ((a, ra), (b, rb)):
        yc, u, v = y0.copy(), u0.copy(), 0.8
        for _ in range(2):
            v = s.sample_random_set(rid, 1.3, yc, u, v)
        res.append((yc, u, v))
        s.close()
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]) and res[0][2] == res[1][2]


# ---- 3. two identities -----------------------------------------------------------------------------------------------------------
def test_no_head_and_empty_S_is_the_dense_engine_bit_for_bit(ngp, O):
    nd, nrec = 130, 100
    T = np.linalg.inv(RG.make_g(RG.hw_genotypes(O, nd, P_GENO, seed=6), 1)[0])     # (positive definite: the block alone is K here)
    T = (T + T.T) / 2.0
    rng = np.random.default_rng(12)
    level = rng.integers(0, nd, size=nrec)
    empty = (np.zeros(nd + 1, dtype=np.int64), np.zeros(0, dtype=np.int32), np.zeros(0))
    y0, u0 = rng.normal(size=nrec), rng.normal(size=nd)
    res = []
    for hybrid in (True, False):
        s = ngp.Sampler(device=0, seed=21, chain=1)
        s.set_records(nrec)
        rid = (s.add_random_set_hybrid(level, nd, empty, nd, D=T, df=4.0, scale=0.4, varU0=0.8) if hybrid
               else s.add_random_set_dense(level, nd, K=T, df=4.0, scale=0.4, varU0=0.8))
        yc, u, v, calls = y0.copy(), u0.copy(), 0.8, []
        for _ in range(3):
            v = s.sample_random_set(rid, 1.3, yc, u, v)
            calls.append((yc.copy(), u.copy(), v))
        res.append(calls)
        s.close()
    for a, b in zip(*res):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_zero_block_of_one_level_against_the_csr_engine(ngp, O):
    """K = a pedigree's A^-1 with a founder placed last, D = [[0]]: the same K as ngp_add_random_set's, the last row walked by the other
    engine -- the same chain to 1e-9 relative, not to the bit."""
    api = _api()
    s_, d_ = RP.random_pedigree(200, 30, seed=5)
    _, Ainv = ngp.pedigree_ainv(s_, d_)
    K = api.permute_csr(Ainv, api.single_step_order(200, [4]))          # animal 4 is a founder
    nrec = 120
    rng = np.random.default_rng(3)
    level = rng.integers(0, 200, size=nrec)
    y0 = rng.normal(size=nrec) * 2.0
    res = []
    for hybrid in (True, False):
        s = ngp.Sampler(device=0, seed=9, chain=0)
        s.set_records(nrec)
        rid = (s.add_random_set_hybrid(level, 200, K, 1, D=np.zeros((1, 1)), df=4.0, scale=0.4, varU0=0.8) if hybrid
               else s.add_random_set(level, 200, K=K, df=4.0, scale=0.4, varU0=0.8))
        yc, u, v = y0.copy(), np.zeros(200), 0.8
        for _ in range(3):
            v = s.sample_random_set(rid, 1.3, yc, u, v)
        res.append((yc, u, v))
        s.close()
    (ya, ua, va), (yb, ub, vb) = res
    print(f"zero block: rel err u {np.abs(ua - ub).max() / np.abs(ub).max():.2e} varU {abs(va - vb) / vb:.2e}")
    assert np.abs(ua - ub).max() <= 1e-9 * np.abs(ub).max()
    assert abs(va - vb) <= 1e-9 * vb
    assert np.abs(ya - yb).max() <= 1e-9 * np.abs(y0).max()


# ---- 4. against the dense engine on the embedded K -------------------------------------------------------------------------------
def test_hybrid_against_dense_engine(ngp, O):
    """The same level order and the same draw keys, hence the same chain: 10 steps at (70, 65)."""
    pr = _problem(ngp, O, 70, 65)
    q, nd, nrec = pr["q"], 65, 150
    K = RS.embed(pr["rows"], q, nd, pr["D"])
    rng = np.random.default_rng(8)
    level = rng.integers(0, q, size=nrec)
    y0 = rng.normal(size=nrec) * 2.0
    res = []
    for hybrid in (True, False):
        s = ngp.Sampler(device=0, seed=5, chain=1)
        s.set_records(nrec)
        rid = (s.add_random_set_hybrid(level, q, pr["S"], nd, D=pr["D"], varU0=0.8) if hybrid else s.add_random_set_dense(level, q, K=K, varU0=0.8))
        yc, u, v = y0.copy(), np.zeros(q), 0.8
        for _ in range(10):
            v = s.sample_random_set(rid, 1.3, yc, u, v)
        res.append((yc, u, v))
        s.close()
    (ya, ua, va), (yb, ub, vb) = res
    print(f"hybrid vs dense, 10 steps: rel err u {np.abs(ua - ub).max() / np.abs(ub).max():.2e} varU {abs(va - vb) / vb:.2e}")
    assert np.abs(ua - ub).max() <= 1e-9 * np.abs(ub).max()
    assert abs(va - vb) <= 1e-9 * vb
    assert np.abs(ya - yb).max() <= 1e-9 * np.abs(y0).max()


# ---- 5. whole chains through runLMEM ---------------------------------------------------------------------------------------------
def _ped300():
    s_, d_ = RP.random_pedigree(300, 40, seed=7)
    names = [f"A{i + 1}" for i in range(300)]
    rows = [(names[i], names[s_[i] - 1] if s_[i] else "0", names[d_[i] - 1] if d_[i] else "0") for i in range(300)]
    return rows, names


def _run_case(O, name):
    rng = np.random.default_rng(17)
    if name == "pblup14":
        rows = list(RP.PBLUP_PED)
        ids = ["QGG12", "QGG5", "QGG9", "QGG14", "QGG3"]
        rec = [r[0] for r in RP.PBLUP_DATA]
        y = np.array([r[5] for r in RP.PBLUP_DATA])
        v, ve = 150.0, 350.0
    else:
        rows, names = _ped300()
        ids = [names[i] for i in rng.permutation(300)[:65]]
        rec = [names[i] for i in rng.integers(60, 300, size=200)]
        y = 10.0 + rng.normal(size=200) * 2.0
        v, ve = 2.0, 2.0
    M = RG.hw_genotypes(O, len(ids), P_GENO, seed=31 + len(ids))
    return rows, ids, rec, y, v, ve, M


@pytest.mark.parametrize("case", ["pblup14", "ped300", "ped300_snp"])
def test_runLMEM_single_step(ngp, O, tmp_path, case):
    api = _api()
    snp = case.endswith("_snp")
    rows, ids, rec, y, v, ve, M = _run_case(O, case.replace("_snp", ""))
    N, w = len(y), 0.05
    data = dict(ID=np.array(rec), BW=y)
    VCV = {"ID": api.Random("H", v), "e": api.Random("I", ve)}
    formula = "BW ~ 1 + PED(ID)"
    Pm, vm = 64, 0.05
    if snp:
        Xm = RG.hw_genotypes(O, N, Pm, seed=5).astype(np.float64)
        np.save(str(tmp_path / "x.npy"), Xm)
        formula += ' + SNP(M1, "%s")' % str(tmp_path / "x.npy")
        VCV["M1"] = api.BayesPR(9999, vm)
    out = str(tmp_path / "out")
    nIt, nBurn, nThin = 30, 10, 2
    res = api.runLMEM(formula, data, nIt, nBurn, nThin, outFolder=out, VCV=VCV, userPedData=rows, seed=1,
                      singleStep={"ID": {"geno": M, "ids": ids, "w": w}})
    kept = (nIt - nBurn) // nThin
    table, Ainv = api.makePed(rows)
    n = len(table["origID"])
    gpos = np.array([table["pos"][a] for a in ids])
    perm = api.single_step_order(n, gpos)
    levels = [table["origID"][o] for o in perm]
    assert levels[n - len(ids):] == ids                                 # the genotyped animals last, in ids order
    with open(os.path.join(out, "uIDOut")) as f:
        lines = f.read().rstrip("\n").split("\n")
    assert lines[0].split("\t") == levels and len(lines) == 1 + kept    # the header names the renumbered animals
    with open(os.path.join(out, "varUIDOut")) as f:
        assert f.readline().rstrip("\n") == "ID"
    rr = res["random"]["ID"]
    assert rr["levels"] == levels and len(rr["u"]) == n
    assert np.allclose(api.summaryMCMC("uID", outFolder=out)[0], rr["u"], rtol=1e-12, atol=1e-12)
    assert np.allclose(api.summaryMCMC("varUID", outFolder=out)[0, 0], rr["varU"], rtol=1e-12)
    # the same model through the dense engine over numpy's H^-1, renumbered
    A = api.makeA(table["Sire"], table["Dam"])
    G = api.makeG(M, 1)
    Hi = RS.h_inverse(A, G, gpos, w)[np.ix_(perm, perm)]
    inv = np.empty(n, dtype=np.int64); inv[perm] = np.arange(n)
    level = inv[np.array([table["pos"][a] for a in rec])]
    s = ngp.Sampler(device=0, seed=1, chain=0)
    if snp:
        s.set_panel(np.asfortranarray(Xm), centre=True)
    else:
        s.set_records(N)
    s.set_residual_prior(4.0, ve * 2.0 / 4.0)
    s.set_intercept(True)
    s.add_random_set_dense(level, n, K=Hi, df=4.0, scale=v * 2.0 / 4.0, varU0=v)
    if snp:
        s.add_marker_set(0, Pm, 0, 4.0, vm * 2.0 / 4.0, [(0, Pm)], [vm])
    s.set_y(y); s.set_schedule(nIt, nBurn, nThin); s.run(nIt)
    hand, ps = s.get_random(0), s.get_posterior_sums()
    eu = np.abs(hand["sum_u"] / kept - rr["u"]).max() / np.abs(rr["u"]).max()
    ev = abs(hand["sum_varU"] / kept - rr["varU"]) / rr["varU"]
    ee = abs(ps["sum_varE"] / kept - res["varE"]) / res["varE"]
    print(f"runLMEM single-step {case}: rel err of the posterior means against the dense engine over numpy's H^-1: u {eu:.2e} varU {ev:.2e} varE {ee:.2e}")
    assert ps["nKept"] == kept == res["nKept"]
    assert eu <= 1e-9 and ev <= 1e-9 and ee <= 1e-9
    if snp:
        assert sorted(res["sets"]) == ["M1"] and os.path.exists(os.path.join(out, "betaM1Out"))
        eb = np.abs(ps["sum_beta"][:Pm] / kept - res["sets"]["M1"]["beta"]).max() / np.abs(res["sets"]["M1"]["beta"]).max()
        assert eb <= 1e-9
    s.close()


# ---- 6. snapshots and shared blocks ----------------------------------------------------------------------------------------------
def _chain(ngp, pr, level, y, D, chain=0, src=None, nd=65):
    s = ngp.Sampler(device=0, seed=13, chain=chain)
    s.set_records(len(y))
    s.add_random_set_hybrid(level, pr["q"], pr["S"], nd, D=D if src is None else (src, 0), df=4.0, scale=0.5, varU0=1.0)
    s.set_y(y); s.set_residual_prior(4.0, 1.0); s.set_schedule(8, 2, 2)
    return s


def _state(s):
    r = s.get_random(0)
    return r["u"], r["sum_u"], r["varU"], r["sum_varU"], s.get_state()["ycorr"], s.get_state()["varE"]


def _same(a, b):
    for x, z in zip(a, b):
        assert np.array_equal(x, z)


def test_snapshot_resume_and_signature(ngp, O, tmp_path):
    pr = _problem(ngp, O, 70, 65)
    rng = np.random.default_rng(2)
    level = rng.integers(0, pr["q"], size=160)
    y = rng.normal(size=160) * 2.0 + 3.0
    a = _chain(ngp, pr, level, y, pr["D"]); a.run(8)
    assert np.abs(_state(a)[0]).max() > 0
    b = _chain(ngp, pr, level, y, pr["D"]); b.run(3)
    b.save_snapshot(str(tmp_path / "snap"))
    c = _chain(ngp, pr, level, y, pr["D"])
    c.load_snapshot(str(tmp_path / "snap")); c.run(5)
    _same(_state(a), _state(c))
    D2 = pr["D"].copy(); D2[40, 17] += 1e-3; D2[17, 40] += 1e-3          # ONE entry pair of the block
    d = _chain(ngp, pr, level, y, D2)
    with pytest.raises(ngp.NextGPHipError, match="random-effect sets differ"):
        d.load_snapshot(str(tmp_path / "snap"))
    for s in (a, b, c, d):
        s.close()


def test_chains_share_one_block(ngp, O):
    pr = _problem(ngp, O, 70, 65)
    nd = 65
    rng = np.random.default_rng(6)
    level = rng.integers(0, pr["q"], size=160)
    ys = [rng.normal(size=160) * 2.0 + 3.0 for _ in range(2)]
    M = RG.hw_genotypes(O, nd, P_GENO, seed=8)
    first = ngp.Sampler(device=0, seed=13, chain=0)
    first.set_records(160)
    _build(first, M)
    first.grm_single_step(pr["A22"], 0.05)
    D = first.grm_get()
    first.add_random_set_hybrid(level, pr["q"], pr["S"], nd, df=4.0, scale=0.5, varU0=1.0)   # takes the builder's block: the builder is empty
    first.set_y(ys[0]); first.set_residual_prior(4.0, 1.0); first.set_schedule(8, 2, 2)
    with pytest.raises(ngp.NextGPHipError, match="error -2"):
        first.grm_get()
    second = _chain(ngp, pr, level, ys[1], None, chain=1, src=first)    # by reference, accepted after the owner's builder is empty
    dense = ngp.Sampler(device=0, seed=13, chain=2)
    dense.set_records(160)
    with pytest.raises(ngp.NextGPHipError, match="not a dense set"):    # the block of a hybrid set is no K of a dense one
        dense.add_random_set_dense(level % nd, nd, K=(first, 0))
    dense.close()
    ngp.Sampler.run_many([first, second], 8)
    for c, s in enumerate((first, second)):
        alone = _chain(ngp, pr, level, ys[c], D, chain=c); alone.run(8)
        _same(_state(s), _state(alone))
        alone.close()
    first.close()                                                       # the block lives on with the set that refers to it
    second.run(1)
    second.close()


def test_runLMEM_two_chains(ngp, O, tmp_path):
    api = _api()
    rows, ids, rec, y, v, ve, M = _run_case(O, "pblup14")
    kw = dict(VCV={"ID": api.Random("H", v), "e": api.Random("I", ve)}, userPedData=rows, seed=1, singleStep={"ID": {"geno": M, "ids": ids}})
    two = api.runLMEM("BW ~ 1 + PED(ID)", dict(ID=np.array(rec), BW=y), 12, 2, 2, outFolder=str(tmp_path / "two"), chains=2, **kw)
    for c in (0, 1):
        assert os.path.exists(os.path.join(str(tmp_path / "two"), f"chain{c}", "uIDOut"))
        one = api.runLMEM("BW ~ 1 + PED(ID)", dict(ID=np.array(rec), BW=y), 12, 2, 2, outFolder=str(tmp_path / f"one{c}"), chain=c, **kw)
        assert np.array_equal(one["random"]["ID"]["u"], two["chains"][c]["random"]["ID"]["u"])
        assert one["random"]["ID"]["varU"] == two["chains"][c]["random"]["ID"]["varU"]
