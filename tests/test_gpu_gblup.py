"""GBLUP on the device: the relationship matrix (ngp_grm_*), its inverse, dense random-effect sets (ngp_add_random_set_dense), handles
without a genotype panel (ngp_set_records) and runLMEM's GBLUP route.  Yardsticks: tests/ref_gblup.py (make_g: the reference's order
of operations in numpy; dense_step_blocked: the device's documented order, bit for bit) and ref_random.RandomRefChain (the reference's
order, to 1e-9 relative)."""
import os

import numpy as np
import pytest

import ref_gblup as RG
import ref_random as RR
from conftest import add_sets, make_problem

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53


def _build(s, M, method, split=None):
    N, P = M.shape
    s.grm_begin(N, method)
    edges = [0, P] if split is None else split
    for a, b in zip(edges[:-1], edges[1:]):
        s.grm_columns(M[:, a:b])
    s.grm_end()
    return s.grm_get()


def _spd_K(q, seed=9):
    rng = np.random.default_rng(seed)
    A = rng.normal(size=(q, min(q, 400)))
    K = np.linalg.inv(A @ A.T + q * np.eye(q))
    return (K + K.T) / 2.0


def _grm_K(O, N, P, method=1, seed=5):
    G, _ = RG.make_g(RG.hw_genotypes(O, N, P, seed=seed), method)
    K = np.linalg.inv(G)
    return (K + K.T) / 2.0


# ---- 4. G against the restatement -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("N,P", [(300, 2000), (257, 4100)])
def test_grm_against_restatement(ngp, O, N, P, method):
    M8 = RG.hw_genotypes(O, N, P, seed=77 + N)
    Gref, scale = RG.make_g(M8, method)
    bound = (2 * P + 2 * N + 8) * EPS * scale
    s = ngp.Sampler(device=0)
    got = {}
    for name, M in (("f64", M8.astype(np.float64)), ("f32", M8.astype(np.float32)), ("u8", M8)):
        G = _build(s, M, method)
        err = np.abs(G - Gref)
        print(f"grm N={N} P={P} method={method} {name}: max err / bound = {(err / bound).max():.3e}")
        assert np.all(err <= bound), name
        assert np.array_equal(G, G.T), name
        got[name] = G
    assert np.array_equal(got["f64"], got["f32"]) and np.array_equal(got["f64"], got["u8"])
    by64 = _build(s, M8, method, split=list(range(0, P, 64)) + [P])
    two = _build(s, M8, method, split=[0, 1984, P])
    assert np.array_equal(by64, got["u8"]) and np.array_equal(two, got["u8"])
    s.close()


def test_grm_ragged_calls_and_leading_dimension(ngp, O):
    """Two corners of the column kernels: a call whose column count is not a multiple of four followed by another call (its tail is
    padded with zero columns, whose products add + 0.0: the contract promises split-independence for multiples of 64 only, the
    error bound holds for any split), and ld > N (the first N rows of a taller matrix, no copy)."""
    N, P = 257, 1000
    M8 = RG.hw_genotypes(O, N, P, seed=21)
    s = ngp.Sampler(device=0)
    whole = _build(s, M8, 1)
    for method in (1, 2):
        Gref, scale = RG.make_g(M8, method)
        bound = (2 * P + 2 * N + 8) * EPS * scale
        G = _build(s, M8, method, split=[0, 61, 63, 322, P])
        print(f"ragged split, method {method}: max err / bound = {(np.abs(G - Gref) / bound).max():.3e}; equal to one call: {np.array_equal(G, whole)}")
        assert np.all(np.abs(G - Gref) <= bound) and np.array_equal(G, G.T)
    for dt in (np.uint8, np.float32, np.float64):
        big = np.asfortranarray(np.vstack([M8, np.full((43, P), 7, dtype=np.uint8)]).astype(dt))   # rows beyond N must not be read as genotypes
        view = big[:N]
        assert view.strides[1] == (N + 43) * big.itemsize
        assert np.array_equal(_build(s, view, 1, split=[0, 640, P]), whole), dt
    s.close()


def test_grm_method2_refuses_a_monomorphic_column(ngp, O):
    N, P = 300, 200
    M = RG.hw_genotypes(O, N, P, seed=3)
    bad = M.copy(); bad[:, 130] = 0
    s = ngp.Sampler(device=0)
    s.grm_begin(N, 2)
    s.grm_columns(bad[:, :128])
    with pytest.raises(ngp.NextGPHipError, match=r"error -1: .*column 130 "):
        s.grm_columns(bad[:, 128:])
    s.grm_begin(N, 2)
    with pytest.raises(ngp.NextGPHipError, match=r"error -1: .*column 130 "):   # ... and inside one call
        s.grm_columns(bad)
    G1 = _build(s, bad, 1)                                              # method 1 takes it as the zero column it becomes
    assert np.all(np.abs(G1 - RG.make_g(bad, 1)[0]) <= (2 * P + 2 * N + 8) * EPS * RG.make_g(bad, 1)[1])
    G2 = _build(s, M, 2)                                                # the handle builds on
    assert np.all(np.abs(G2 - RG.make_g(M, 2)[0]) <= (2 * P + 2 * N + 8) * EPS * RG.make_g(M, 2)[1])
    s.close()


# ---- 5. inverse -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,P", [(300, 150), (300, 2000), (1200, 5000)])
def test_grm_inverse(ngp, O, N, P):
    M = RG.hw_genotypes(O, N, P, seed=N + P)
    s = ngp.Sampler(device=0)
    G = _build(s, M, 1)
    s.grm_invert()
    K = s.grm_get()
    cond = np.linalg.cond(G, 2)
    res = np.abs(K @ G - np.eye(N)).max()
    print(f"inverse N={N} P={P}: cond {cond:.3e}, max|KG - I| {res:.3e}, bound {8 * N * EPS * cond:.3e}")
    assert res <= 8 * N * EPS * cond
    assert np.array_equal(K, K.T)
    with pytest.raises(ngp.NextGPHipError, match="error -2"):          # inverted already
        s.grm_invert()
    s.close()


def test_grm_refusals_leave_a_usable_handle(ngp, O):
    N = 128
    s = ngp.Sampler(device=0)
    with pytest.raises(ngp.NextGPHipError, match="error -2"):          # nothing begun
        s.grm_invert()
    s.grm_begin(N, 1)
    s.grm_columns(np.full((N, 64), 2, dtype=np.uint8))                  # every column monomorphic: sum 2pq = 0
    with pytest.raises(ngp.NextGPHipError, match="error -2"):          # invert before end
        s.grm_invert()
    with pytest.raises(ngp.NextGPHipError, match="error -1"):
        s.grm_end()
    M = RG.hw_genotypes(O, N, 500, seed=2)
    G = _build(s, M, 1)
    s.grm_invert()
    assert np.abs(s.grm_get() @ G - np.eye(N)).max() < 1e-8
    s.close()


# ---- 6. dense engine, fine seam, bit for bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("incidence", ["identity", "levels"])
@pytest.mark.parametrize("q", [23, 64, 65, 200, 1100, 2500])
def test_dense_fine_seam_bit_exact(ngp, O, q, incidence, weighted):
    rng = np.random.default_rng(4 + q)
    N = q if incidence == "identity" else 300
    level = None if incidence == "identity" else rng.integers(0, q - 2, size=N)      # two levels without records
    w = rng.uniform(0.3, 3.0, N) if weighted else None
    K = _spd_K(q)
    s = ngp.Sampler(device=0, seed=77, chain=2)
    if weighted:
        s.set_residual_weights(w)
    if incidence == "identity":
        s.set_records(N)                                                # no genotype panel at all
    else:
        s.set_panel(make_problem(O, N, 128, seed=2)[0])
    s.add_random_set(rng.integers(0, 5, size=N), 5)                     # a first set: the dense one's keys carry set id 1
    rid = s.add_random_set_dense(level, q, K=K, df=4.0, scale=0.4, varU0=0.8)
    assert rid == 1
    ycorr = rng.normal(size=N) * 3.0
    u = rng.normal(size=q)
    rs = np.sqrt(w) if weighted else None
    zpz = RR.zpz_of(np.arange(N) if level is None else level, q, w)
    varU = 0.8
    for it in (1, 2):                                                   # the set's own call counter is the iteration of its draws
        yt_in = ycorr * rs if weighted else ycorr
        yt, u_ref, v_ref = RG.dense_step_blocked(O, 77, 2, it, rid, yt_in, rs, level, q, K, zpz, u, varU, 1.3, 4.0, 0.4)
        y_ref = yt / rs if weighted else yt
        varU = s.sample_random_set(rid, 1.3, ycorr, u, varU)           # ycorr, u updated in place
        assert np.array_equal(u, u_ref), it
        assert varU == v_ref, it
        assert np.array_equal(ycorr, y_ref), it
    s.close()


# ---- 7. dense engine against the CSR engine ------------------------------------------------------------------------------------
def test_dense_against_csr_engine(ngp, O):
    N, P, q = 300, 128, 200
    X, y, _, v = make_problem(O, N, P, seed=2)
    rng = np.random.default_rng(8)
    level = rng.integers(0, q, size=N)
    K = _grm_K(O, q, 1500)
    hs = []
    for dense in (True, False):
        s = ngp.Sampler(device=0, seed=5, chain=1)
        s.set_panel(X)
        rid = s.add_random_set_dense(level, q, K=K, varU0=0.8) if dense else s.add_random_set(level, q, K=K, varU0=0.8)
        add_sets(s, [(0, P, "B")], v)
        s.set_y(y)
        hs.append((s, rid))
    out = []
    for s, rid in hs:
        yc, u = y - y.mean(), np.zeros(q)
        vu = s.sample_random_set(rid, 1.3, yc, u, 0.8)
        out.append((yc, u, vu))
    (ya, ua, va), (yb, ub, vb) = out
    assert np.abs(ua - ub).max() <= 1e-9 * np.abs(ub).max()
    assert abs(va - vb) <= 1e-9 * vb
    assert np.abs(ya - yb).max() <= 1e-9 * np.abs(y).max()
    res = []
    for s, rid in hs:                                                   # the same numbers next: a BayesB set on common values
        yc, beta, vb_, pi = ya.copy(), np.zeros(P), np.full(P, v), np.array([0.95, 0.05])
        delta = s.sweep_set(0, 1.3, yc, beta, vb_, pi)
        res.append((delta, beta))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    # ... and in a chain: after one iteration through ngp_run both handles agree to rounding, delta exactly
    for s, _ in hs:
        s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var()); s.run(1)
    a, b = hs[0][0].get_state(), hs[1][0].get_state()
    assert np.array_equal(a["delta"], b["delta"])
    assert np.abs(a["beta"] - b["beta"]).max() <= 1e-9 * max(1e-6, np.abs(b["beta"]).max())
    for s, _ in hs:
        s.close()


# ---- 8. whole chains -----------------------------------------------------------------------------------------------------------
def _chain_problem(O, N=300, P=128, qh=12, seed=3):
    X, y, _, v = make_problem(O, N, P, seed=seed)
    rng = np.random.default_rng(seed + 50)
    herd = rng.integers(0, qh, size=N)
    y = y + (rng.normal(size=qh) * 2.0 * np.sqrt(y.var()))[herd]
    return X, y, v, herd, qh, _grm_K(O, N, 1500, seed=seed)


def _model(ngp, X, y, v, herd, qh, K, seed=31, chain=1, markers=True, k_src=None):
    s = ngp.Sampler(device=0, seed=seed, chain=chain)
    if markers:
        s.set_panel(X)
    else:
        s.set_records(len(y))
    s.add_random_set_dense(None, len(y), K=K if k_src is None else k_src, df=4.0, scale=0.5, varU0=1.0)
    s.add_random_set(herd, qh, df=4.0, scale=1.0, varU0=2.0)
    if markers:
        add_sets(s, [(0, X.shape[1], "B")], v)
    s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var()); s.set_schedule(4, 0, 1)
    return s


def _rand_state(s):
    return [s.get_random(r) for r in range(2)], s.get_state(), s.get_posterior_sums()


def _same_chain(a, b):
    (ra, sa, pa), (rb, sb, pb) = a, b
    for x, z in zip(ra, rb):
        assert np.array_equal(x["u"], z["u"]) and np.array_equal(x["sum_u"], z["sum_u"])
        assert x["varU"] == z["varU"] and x["sum_varU"] == z["sum_varU"]
    for k in ("ycorr", "beta", "delta", "varBeta"):
        assert np.array_equal(sa[k], sb[k]), k
    assert sa["varE"] == sb["varE"] and sa["b"] == sb["b"] and sa["iter"] == sb["iter"]
    assert pa["sum_varE"] == pb["sum_varE"] and pa["nKept"] == pb["nKept"] and np.array_equal(pa["sum_beta"], pb["sum_beta"])


@pytest.mark.parametrize("markers", [True, False], ids=["with_marker_set", "records_only"])
def test_chain_vs_reference_order(ngp, O, markers):
    X, y, v, herd, qh, K = _chain_problem(O)
    N = len(y)
    s = _model(ngp, X, y, v, herd, qh, K, markers=markers)
    ref = RR.RandomRefChain(O, X.astype(np.float64) if markers else np.zeros((N, 1)), y, seed=31, chain=1)
    ref.add_marker_set, ref.add_marker_set_r = ref.add_set, ref.add_set_r
    ref.add_random(np.arange(N), N, K, df=4.0, scale=0.5, v=1.0)
    ref.add_random(herd, qh, None, df=4.0, scale=1.0, v=2.0)
    if markers:
        add_sets(ref, [(0, X.shape[1], "B")], v)
    ref.E_df, ref.E_scale = 4.0, 0.25 * y.var()
    tol = lambda a, b: np.abs(np.asarray(a) - np.asarray(b)).max() <= 1e-9 * max(1e-6, np.abs(np.asarray(b)).max())
    for it in range(4):
        s.run(1); ref.run(1)
        a = s.get_state()
        if markers:
            b = ref.state()
            assert np.array_equal(a["delta"], b["delta"]), it
            assert tol(a["beta"], b["beta"]) and tol(a["varBeta"], b["varBeta"]), it
        assert tol(a["ycorr"], ref.ycorr), it
        for r in range(2):
            g = s.get_random(r)
            assert tol(g["u"], ref.u[r]), (it, r)
            assert abs(g["varU"] - ref.varU[r]) <= 1e-9 * ref.varU[r], (it, r)
        assert abs(a["varE"] - ref.varE) <= 1e-9 * ref.varE and abs(a["b"] - ref.b[0]) <= 1e-9 * max(1e-6, abs(ref.b[0]))
    s.close()


@pytest.mark.parametrize("markers", [True, False], ids=["with_marker_set", "records_only"])
def test_chain_repeats_resumes_and_splits(ngp, O, markers, tmp_path):
    X, y, v, herd, qh, K = _chain_problem(O)
    a = _model(ngp, X, y, v, herd, qh, K, markers=markers); a.run(4)
    b = _model(ngp, X, y, v, herd, qh, K, markers=markers); b.run(4)          # run to run
    _same_chain(_rand_state(a), _rand_state(b))
    c = _model(ngp, X, y, v, herd, qh, K, markers=markers); c.run(2); c.run(2)  # ngp_run(4) == ngp_run(2) twice
    _same_chain(_rand_state(a), _rand_state(c))
    d = _model(ngp, X, y, v, herd, qh, K, markers=markers); d.run(2)
    d.save_snapshot(str(tmp_path / "snap"))
    e = _model(ngp, X, y, v, herd, qh, K, markers=markers)
    e.load_snapshot(str(tmp_path / "snap")); e.run(2)                        # snapshot at iteration 2 + resume
    _same_chain(_rand_state(a), _rand_state(e))
    K2 = K.copy(); K2[150, 97] += 1e-3; K2[97, 150] += 1e-3              # another K: ONE entry pair, away from row 0 and the diagonal
    f = _model(ngp, X, y, v, herd, qh, K2, markers=markers)
    with pytest.raises(ngp.NextGPHipError, match="random-effect sets differ"):
        f.load_snapshot(str(tmp_path / "snap"))
    if not markers:
        with pytest.raises(ngp.NextGPHipError, match="ngp_set_records"):
            a.add_marker_set(0, 64, 0, 4.0, 0.5 * v, [(0, 64)], [v])
        g = ngp.Sampler(device=0); g.set_records(len(y)); g.set_y(y)
        with pytest.raises(ngp.NextGPHipError, match="no random-effect set"):
            g.run(1)
        g.close()
    for s in (a, b, c, d, e, f):
        s.close()


def test_sample_file_of_a_records_only_chain(ngp, O, tmp_path):
    X, y, v, herd, qh, K = _chain_problem(O)
    a = _model(ngp, X, y, v, herd, qh, K, markers=False)
    a.set_sample_file(str(tmp_path / "s.ngpsmp")); a.run(4); a.set_sample_file(None)
    S = ngp.read_sample_file(str(tmp_path / "s.ngpsmp"))
    assert S["u"][0].shape == (4, len(y)) and S["u"][1].shape == (4, qh) and S["varU"].shape == (4, 2)
    assert np.array_equal(S["u"][0][-1], a.get_random(0)["u"]) and S["varU"][-1, 0] == a.get_random(0)["varU"]
    assert a.posterior_len() == 3 * 64 + 0 + 0 + (len(y) + qh + 2) + 3   # the inert block's 64 columns, no variance component, no set
    a.close()


# ---- 9. one K, several chains --------------------------------------------------------------------------------------------------
def test_shared_dense_K(ngp, O):
    import torch
    q = 2048
    K = _spd_K(q, seed=2)
    rng = np.random.default_rng(1)
    ys = [rng.normal(size=q) * 2.0 + 5.0 for _ in range(3)]

    def chain(c, src=None):
        s = ngp.Sampler(device=0, seed=11, chain=c)
        s.set_records(q)
        s.add_random_set_dense(None, q, K=K if src is None else (src, 0), df=4.0, scale=0.5, varU0=1.0)
        s.set_y(ys[c]); s.set_residual_prior(4.0, 1.0); s.set_schedule(6, 2, 2)
        return s

    first = chain(0)
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    chains = [first, chain(1, first), chain(2, first)]
    torch.cuda.synchronize()
    grown = free0 - torch.cuda.mem_get_info()[0]
    print(f"two sharers: device memory grew by {grown / 2 ** 20:.1f} MiB, one K is {q * q * 8 / 2 ** 20:.1f} MiB")
    assert grown < q * q * 8
    ngp.Sampler.run_many(chains, 6)
    for c in range(3):
        alone = chain(c); alone.run(6)
        g, h = chains[c].get_random(0), alone.get_random(0)
        assert np.array_equal(g["u"], h["u"]) and np.array_equal(g["sum_u"], h["sum_u"]) and g["varU"] == h["varU"]
        assert np.array_equal(chains[c].get_state()["ycorr"], alone.get_state()["ycorr"])
        alone.close()
    first.close()                                                       # the matrix lives on with the sets that refer to it
    chains[1].run(1)
    for s in chains[1:]:
        s.close()


# ---- 10. runLMEM ---------------------------------------------------------------------------------------------------------------
def _sim(O, N=300, P=2000, seed=12):
    """300 x 2,000 Hardy-Weinberg genotypes, every marker with a normal effect, h2 = 0.5."""
    M = RG.hw_genotypes(O, N, P, seed=seed)
    rng = np.random.default_rng(seed)
    Xc = M.astype(np.float64) - M.mean(axis=0)
    g = Xc @ rng.normal(size=P)
    g = g / g.std()
    y = 10.0 + g + rng.normal(size=N)
    return M, y, g


def test_runLMEM_gblup(ngp, O, tmp_path):
    """Files, headers, means, and the chain built by hand through the C ABI.  Accuracy: corr(posterior mean of u, simulated g) after
    2,000 iterations (burn-in 400, every 4th kept).  Yardstick: the reference-order restatement (ref_random.RandomRefChain, Z = I over
    K = inv(ref_gblup.make_g(M))) on the same data with the same schedule gives 0.7491 on the CPU (seed 1, chain 0); seeds 2, 3, 4 give
    0.7483, 0.7519, 0.7485 -- a seed-to-seed spread of 0.004, far below the 0.05 the comparison allows."""
    from nextgp_jl_amd import api
    M, y, g = _sim(O)
    N = len(y)
    v = ve = 0.5 * y.var()
    VCV = {"M1": api.Random("G", v), "e": api.Random("I", ve)}
    out = str(tmp_path / "one")
    res = api.runLMEM("y ~ 1 + SNP(M1, X)".replace("X", '"%s"' % _npy(tmp_path, "g.npy", M)), dict(y=y), 2000, 400, 4, outFolder=out, VCV=VCV, seed=1)
    kept = (2000 - 400) // 4
    for name, hdr in (("uM1", [f"Ind{i + 1}" for i in range(N)]), ("varUM1", ["M1"]), ("varE", ["e"]), ("b", ["(Intercept)"])):
        with open(os.path.join(out, name + "Out")) as f:
            lines = f.read().rstrip("\n").split("\n")
        assert lines[0].split("\t") == hdr, name
        assert len(lines) == 1 + kept, name
    assert not [f for f in os.listdir(out) if f.startswith(("beta", "delta", "var")) and not f.startswith(("varU", "varE"))]
    rr = res["random"]["M1"]
    assert np.allclose(api.summaryMCMC("uM1", outFolder=out)[0], rr["u"], rtol=1e-12, atol=1e-12)
    assert np.allclose(api.summaryMCMC("varUM1", outFolder=out)[0, 0], rr["varU"], rtol=1e-12)
    assert np.allclose(api.summaryMCMC("varE", outFolder=out)[0, 0], res["varE"], rtol=1e-12)
    # the same chain by hand
    s = ngp.Sampler(device=0, seed=1, chain=0)
    s.set_records(N)
    s.set_residual_prior(4.0, ve * 2.0 / 4.0)
    _build(s, M, 1, split=[0, 640, 2000]); s.grm_invert()
    s.add_random_set_dense(None, N, df=4.0, scale=v * 2.0 / 4.0, varU0=v)
    s.set_y(y); s.set_schedule(2000, 400, 4); s.run(2000)
    hand = s.get_random(0)
    assert np.array_equal(hand["sum_u"] / kept, rr["u"]) and hand["sum_varU"] / kept == rr["varU"]
    s.close()
    corr = np.corrcoef(rr["u"], g)[0, 1]
    print(f"runLMEM GBLUP: corr(posterior mean u, simulated g) = {corr:.4f} (reference order on the CPU: 0.7491)")
    assert abs(corr - 0.7491) <= 0.05


def _npy(tmp_path, name, M):
    p = str(tmp_path / name)
    np.save(p, M)
    return p


def test_runLMEM_mixed_model_and_chains(ngp, O, tmp_path):
    from nextgp_jl_amd import api
    M, y, g = _sim(O, N=300, P=640)
    M2 = RG.hw_genotypes(O, 300, 256, seed=99)
    v = 0.5 * y.var()
    f = 'y ~ 1 + SNP(M1, "%s") + SNP(M2, "%s")' % (_npy(tmp_path, "g1.npy", M), _npy(tmp_path, "g2.npy", M2))
    VCV = {"M1": api.Random("G", v, type=2), "M2": api.BayesC(0.1, 0.01), "e": api.Random("I", v)}
    out = str(tmp_path / "mixed")
    res = api.runLMEM(f, dict(y=y), 40, 10, 2, outFolder=out, VCV=VCV, chains=2, storage="u8")
    for c in (0, 1):
        folder = os.path.join(out, f"chain{c}")
        for name in ("uM1", "varUM1", "betaM2", "varM2", "piM2", "varE", "b"):
            assert os.path.exists(os.path.join(folder, name + "Out")), (c, name)
        assert not os.path.exists(os.path.join(folder, "betaM1Out"))
    assert res["random"]["M1"]["u"].shape == (300,) and res["sets"]["M2"]["beta"].shape == (256,)
    assert np.corrcoef(res["random"]["M1"]["u"], g)[0, 1] > 0.5
    one = api.runLMEM('y ~ 1 + SNP(M1, "%s")' % _npy(tmp_path, "g1.npy", M), dict(y=y), 40, 10, 2, outFolder=str(tmp_path / "two"),
                      VCV={"M1": api.Random("G", v), "e": api.Random("I", v)}, chains=2)
    assert os.path.exists(os.path.join(str(tmp_path / "two"), "chain1", "uM1Out")) and len(one["chains"]) == 2
    G = api.makeG(M, method=2)
    assert np.all(np.abs(G - RG.make_g(M, 2)[0]) <= (2 * 640 + 2 * 300 + 8) * EPS * RG.make_g(M, 2)[1])
