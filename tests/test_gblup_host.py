"""GBLUP without a device: the numpy restatements of tests/ref_gblup.py against closed forms and against the reference's order
(ref_random.RandomRefChain), and the prior routing of the host mirror."""
import numpy as np
import pytest

import ref_gblup as RG
import ref_random as RR


@pytest.mark.parametrize("method", [1, 2])
def test_make_g_closed_forms(O, method):
    N, P = 200, 1500
    M = RG.hw_genotypes(O, N, P)
    G, _ = RG.make_g(M, method)
    assert np.array_equal(G, G.T)                                       # symmetric (A A' is, entry by entry, in one dot order)
    G0 = G - 0.001 * np.eye(N)
    scale = np.abs(G0).max()
    assert np.abs(G0.sum(axis=1)).max() <= 1e-12 * N * scale            # centred columns: rows of Xc Xc' sum to 0 before the ridge
    Gn, _ = RG.make_g(M, method, ridge=0.0)
    assert np.allclose(np.diag(G) - np.diag(Gn), 0.001, rtol=0, atol=1e-15)   # the ridge is there, on the diagonal only
    assert np.array_equal(G - np.diag(np.diag(G)), Gn - np.diag(np.diag(Gn)))
    if method == 2:
        # Hardy-Weinberg genotypes: E[(x - 2p)^2 / (2pq)] = 1, so the diagonal averages 1 (+ the ridge) up to sampling: N P terms of
        # variance O(1 / (2pq)) <= 11 at p >= 0.05 -- a standard error below 0.01
        assert abs(np.diag(G).mean() - 1.001) < 0.05


def test_indexed_draws_are_one_stream_per_index(O):
    """dense_step_blocked takes the q normals of a step in one call: entry l must be the first draw of stream index0 + l."""
    a = O.draws(5, 1, 3, RR.KIND_U_NORMAL, (2 << 40), 1, 70, 0.0, 0.0, indexed=True)
    b = np.array([RR.draw(O, 5, 1, 3, RR.KIND_U_NORMAL, (2 << 40) | l, 1) for l in range(70)])
    assert np.array_equal(a, b)


@pytest.mark.parametrize("N,P,method", [(200, 1500, 1), (200, 1500, 2), (300, 150, 1)])
def test_blocked_dense_step_vs_reference_order(O, N, P, method):
    """The device's documented order (blocks of 64 levels, split dot products, u'Ku from dlo) against the reference's order on a
    GRM-derived K: the same Markov chain, other summation orders."""
    M = RG.hw_genotypes(O, N, P, seed=11 + P)
    G, _ = RG.make_g(M, method)
    K = np.linalg.inv(G)
    K = (K + K.T) / 2.0
    q = N
    rng = np.random.default_rng(3)
    y = rng.normal(size=N) * 2.0
    seed, chain, varE, df, v = 41, 2, 1.7, 4.0, 0.9
    scale = v * (df - 2.0) / df
    ref = RR.RandomRefChain(O, np.zeros((N, 1)), y, seed=seed, chain=chain)
    ref.ycorr = y.copy()
    ref.add_random(np.arange(N), q, K, df=df, scale=scale, v=v)
    yt, u, varU = y.copy(), np.zeros(q), v
    zpz = np.ones(q)
    for it in range(1, 7):
        ref.iter = it
        ref.sampleZ(0, varE)
        yt, u, varU = RG.dense_step_blocked(O, seed, chain, it, 0, yt, None, None, q, K, zpz, u, varU, varE, df, scale)
        assert np.abs(u - ref.u[0]).max() <= 1e-9 * max(1e-6, np.abs(ref.u[0]).max()), it
        assert abs(varU - ref.varU[0]) <= 1e-9 * ref.varU[0], it
        assert np.abs(yt - ref.ycorr).max() <= 1e-9 * np.abs(y).max(), it


def test_blocked_dense_step_equals_csr_restatement_to_rounding(O):
    """... and against the CSR engine's restatement (ref_random.random_step_blocked) with a general level coding and weights."""
    N, q = 300, 70
    rng = np.random.default_rng(5)
    A = rng.normal(size=(q, q))
    K = np.linalg.inv(A @ A.T + q * np.eye(q)); K = (K + K.T) / 2.0
    level = rng.integers(0, q - 2, size=N)
    w = rng.uniform(0.3, 3.0, N)
    rs = np.sqrt(w)
    zpz = RR.zpz_of(level, q, w)
    y = rng.normal(size=N)
    u0 = rng.normal(size=q)
    a = RR.random_step_blocked(O, 7, 0, 1, 1, y * rs, list(rs), level, q, K, zpz, u0, 0.8, 1.3, 4.0, 0.4)
    b = RG.dense_step_blocked(O, 7, 0, 1, 1, y * rs, rs, level, q, K, zpz, u0, 0.8, 1.3, 4.0, 0.4)
    assert np.abs(np.array(a[1]) - b[1]).max() <= 1e-9 * np.abs(b[1]).max()
    assert abs(a[2] - b[2]) <= 1e-9 * b[2]
    assert np.abs(np.array(a[0]) - b[0]).max() <= 1e-9 * np.abs(y).max()


def test_library_exports_the_gblup_calls(ngp):
    import ctypes as C
    import __graft_entry__ as g
    g.build()
    lib = ngp.load()
    for name in ("ngp_grm_begin", "ngp_grm_columns_f64", "ngp_grm_columns_f32", "ngp_grm_columns_u8", "ngp_grm_end", "ngp_grm_get", "ngp_grm_invert",
                 "ngp_add_random_set_dense", "ngp_set_records"):
        assert name in ngp.SYMBOLS and hasattr(lib, name), name
    lib.ngp_set_records.restype = C.c_int32
    assert lib.ngp_set_records(None, C.c_int64(10)) == -1          # a null handle is an argument error, not a crash
    lib.ngp_grm_invert.restype = C.c_int32
    assert lib.ngp_grm_invert(None) == -1


def test_gblup_prior_routing_without_a_device(ngp):
    from nextgp_jl_amd import api
    p = api.parse_formula('y ~ 1 + (1|herd) + SNP(M1, "g1.txt") + SNP(M2, "g2.txt")', random_effects=True)
    assert p.order == [("1|", "herd"), ("snp", "M1"), ("snp", "M2")]
    snps = p[2]
    VCV = {"M1": api.Random("G", 0.3, type=2), "M2": api.BayesC(0.1, 0.01)}
    assert api.gblup_terms(snps, VCV) == ["M1"] and VCV["M1"].type == 2
    assert api.gblup_terms(snps, {"M2": api.BayesC(0.1, 0.01)}) == []
    with pytest.raises(NotImplementedError, match="functions.jl:75-89"):        # a tuple key with a GBLUP member
        api.gblup_terms(snps, {"M1": api.Random("G", 0.3), ("M1", "M2"): api.BayesPR(9999, np.eye(2))})
    pm = api.parse_formula('y ~ 1 + SNP(M1, "g1.txt", "map.txt")')
    with pytest.raises(NotImplementedError, match="prepMatVec.jl:126"):         # a map file on a GBLUP term
        api.gblup_terms(pm[2], {"M1": api.Random("G", 0.3)})
    with pytest.raises(NotImplementedError, match="mme.jl:140-147"):            # summary statistics for it
        api.gblup_terms(snps, VCV, {"M1": (np.zeros(3), np.ones(3))})
    with pytest.raises(NotImplementedError, match="structure"):                 # Random("I") under a SNP name is not a model of the reference
        api.gblup_terms(snps, {"M1": api.Random("I", 0.3)})
