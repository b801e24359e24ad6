"""SNP effects and candidate prediction from an APY set (k_apy_kw_tail, k_apy_kw_core; DESIGN.md section 2, "APY random-effect sets")
against plain numpy float64 on the device's own pieces: W = K_APY X by the factored form, Wn = d (Xn - P Xc), Wc = Kc0 Xc - P' Wn.
Bounds by ref_apy's one rule: the factored expressions on absolute values (never the assembled |K|: Kcc can cancel where the factored form
does not) times gamma(longest sum + 2) times RA.TOL; the sums over the draws add test_gpu_backsolve's terms.  Nothing is tuned."""
import ctypes as C

import numpy as np
import pytest

import ref_apy as RA
import test_gpu_backsolve as TB

pytestmark = pytest.mark.gpu


def _chain(ngp, Z, nc, method, dtype, T, chain=0, k_src=None, run=True):
    """test_gpu_backsolve._chain over an APY set (the same calls in the same order: with nc = N the same chain)."""
    N = Z.shape[0]
    y = np.random.default_rng(77).normal(size=N) + 0.3 * (Z[:, 0] - Z[:, 0].mean())
    s = ngp.Sampler(device=0, seed=5, chain=chain)
    s.set_records(N); s.set_residual_prior(4.0, 0.5)
    if k_src is None:
        s.grm_begin_apy(N, nc, method); s.grm_columns(np.asfortranarray(Z.astype(dtype))); s.grm_end(); s.grm_apy()
    s.add_random_set_apy(None, N, nc, K=None if k_src is None else (k_src, 0), df=4.0, scale=0.5, varU0=1.0)
    s.set_y(y); s.set_schedule(2 + T, 2, 1); s.enable_backsolve(0, T)
    if run:
        s.run(2 + T)
    return s


def _kx(pc, X):
    """(K_APY X, the same expressions on absolute values) from the pieces."""
    P, d, K0 = pc["P"], pc["d"][:, None], pc["Kc0"]
    nc = K0.shape[0]
    Wn, aWn = d * (X[nc:] - P @ X[:nc]), d * (np.abs(X[nc:]) + np.abs(P) @ np.abs(X[:nc]))
    return np.vstack([K0 @ X[:nc] - P.T @ Wn, Wn]), np.vstack([np.abs(K0) @ np.abs(X[:nc]) + np.abs(P).T @ aWn, aWn])


def _sums(A, dj, W, aW, n):
    """sum_t m and sum_t m^2 of m = dj (A W) with their tolerances (n: the longest sum), as test_gpu_backsolve._ref forms them."""
    m, b = dj[:, None] * (A @ W), RA.TOL * RA.gamma(n + 2) * dj[:, None] * (np.abs(A) @ aW)
    T = W.shape[1]
    return (m.sum(axis=1), (m ** 2).sum(axis=1), b.sum(axis=1) + T * TB.EPS * np.abs(m).sum(axis=1),
            ((2.0 * np.abs(m) + b) * b).sum(axis=1) + (T + 1) * TB.EPS * (m ** 2).sum(axis=1))


def _weights(Z, method):
    mu = Z.mean(axis=0)
    tp = mu * (1.0 - mu / 2.0)
    return mu, np.full(Z.shape[1], 1.0 / tp.sum()) if method == 1 else 1.0 / (Z.shape[1] * tp)


def _check(r, Z, pc, U, method, what="beta"):
    Z, nc = Z.astype(np.float64), pc["Kc0"].shape[0]
    mu, dj = _weights(Z, method)
    s1, s2, tol1, tol2 = _sums((Z - mu).T, dj, *_kx(pc, U), max(Z.shape[0], nc, Z.shape[0] - nc))
    e1, e2 = np.abs(r["sum"] - s1), np.abs(r["sumsq"] - s2)
    print(f"{what} sum: worst error / bound {np.max(e1 / tol1):.3g}; sumsq: {np.max(e2 / tol2):.3g}")
    assert r["n"] == U.shape[1] and np.all(e1 <= tol1) and np.all(e2 <= tol2)


# every tile partial; nn = 3 < 4 (the nnpad edge); two core tiles, two row tiles, a second 16-draw group; a second 64-draw group and column tile
@pytest.mark.parametrize("N,nc,P,T", [(37, 5, 9, 1), (67, 64, 10, 3), (150, 70, 40, 17), (150, 70, 70, 65)])
@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("kind", ["f64", "u8"])
def test_backsolve_parity(ngp, kind, method, N, nc, P, T):
    Z = TB._genotypes(N, P, seed=N + P)
    s = _chain(ngp, Z, nc, method, TB.DTYPES[kind], T)
    r = s.backsolve(0, np.asfortranarray(Z.astype(TB.DTYPES[kind])), splits=[P // 3 + 1])
    assert s.backsolve_draws(0).shape == (N, T)
    _check(r, Z, s.grm_get_apy(rset=0), s.backsolve_draws(0), method)
    s.close()


def test_all_core_is_the_dense_back_solve(ngp):
    """nc = N: the chain over Kc0 is k_bs_kw's over K and the tail is not launched -- the dense set's bits."""
    Z = TB._genotypes(70, 40, seed=2)
    a, (b, _) = _chain(ngp, Z, 70, 1, np.uint8, 3), TB._chain(ngp, Z, 1, np.uint8, 3)
    ra, rb = a.backsolve(0, Z.astype(np.uint8)), b.backsolve(0, Z.astype(np.uint8))
    assert np.array_equal(a.backsolve_draws(0), b.backsolve_draws(0)) and np.array_equal(ra["sum"], rb["sum"]) and np.array_equal(ra["sumsq"], rb["sumsq"])
    a.close(); b.close()


@pytest.mark.parametrize("N,nc,Nc,T", [(150, 70, 5, 3), (150, 70, 70, 17)])
@pytest.mark.parametrize("method", [1, 2])
def test_prediction_parity(ngp, method, N, nc, Nc, T):
    """sum, sumsq of m = C W; s = gcc - diag(C K_APY C'); gcc = sum_j d_j (z_cj - mu_j)^2 -- C the device's own block (gblup_cross)."""
    Z, Zc = TB._genotypes(N, 70, seed=N + Nc), TB._genotypes(Nc + 2, 70, seed=Nc)[2:]
    s = _chain(ngp, Z, nc, method, np.uint8, T)
    r = s.gblup_predict(0, Z.astype(np.uint8), Zc.astype(np.uint8), splits=[64])
    Cm, pc, n = s.gblup_cross(), s.grm_get_apy(rset=0), max(N, nc, N - nc, 70)
    s1, s2, tol1, tol2 = _sums(Cm, np.ones(Nc), *_kx(pc, s.backsolve_draws(0)), n)
    mu, dj = _weights(Z.astype(np.float64), method)
    gcc = ((Zc - mu) ** 2) @ dj
    V, aV = _kx(pc, Cm.T)
    sref, bs = gcc - np.sum(Cm * V.T, axis=1), RA.TOL * RA.gamma(n + 2) * (gcc + np.sum(np.abs(Cm) * aV.T, axis=1))
    for name, got, want, tol in (("sum", r["sum"], s1, tol1), ("sumsq", r["sumsq"], s2, tol2), ("s", r["s"], sref, bs),
                                 ("gcc", r["gcc"], gcc, RA.TOL * RA.gamma(72) * gcc)):
        print(f"prediction {name}: worst error / bound {np.max(np.abs(got - want) / tol):.3g}")
        assert np.all(np.abs(got - want) <= tol), name
    assert r["n"] == T
    s.close()


def test_shared_form_pools(ngp):
    """The second handle takes the first one's form by reference: the builder's method and column weights travel with the form."""
    N, nc, P, T = 150, 70, 40, 17
    Z = TB._genotypes(N, P, seed=3)
    a = _chain(ngp, Z, nc, 1, np.uint8, T, run=False)
    b = _chain(ngp, Z, nc, 1, np.uint8, T, chain=1, k_src=a, run=False)
    ngp.Sampler.run_many([a, b], 2 + T)
    ra, rb = a.backsolve(0, Z.astype(np.uint8)), b.backsolve(0, Z.astype(np.float32), method=1)
    Ua, Ub = a.backsolve_draws(0), b.backsolve_draws(0)
    assert not np.array_equal(Ua, Ub)
    _check(ngp.pool_backsolve([ra, rb]), Z, b.grm_get_apy(rset=0), np.concatenate([Ua, Ub], axis=1), 1)
    b.close(); a.close()


def test_an_open_back_solve_refuses_a_prediction(ngp):
    Z = TB._genotypes(37, 9, seed=1)
    s = _chain(ngp, Z, 5, 1, np.float64, 2)
    s._chk(s.L.ngp_backsolve_begin(s.h, C.c_int32(0)))
    assert s.L.ngp_gpred_begin(s.h, C.c_int32(0), C.c_int64(3)) == -2   # NGP_ERR_STATE
    _check(s.backsolve(0, Z), Z, s.grm_get_apy(rset=0), s.backsolve_draws(0), 1)   # ... and the handle still works
    s.close()
