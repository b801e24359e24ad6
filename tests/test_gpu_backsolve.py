"""SNP effects from GBLUP on the device (ngp_backsolve_*; DESIGN.md section 2, "SNP effects from GBLUP") against plain numpy float64:
beta_ref = d o ((Z - mu)' (K U)) with K from ngp_grm_get, U from ngp_backsolve_get_draws and Z the test's own integer array.
The per-entry bound is derived, not tuned: |beta - beta_ref| <= 8 (N + q) 2^-53 d_j sum_i |z_ij - mu_j| sum_k |K_ik| |u_kt| (two chained
dot products of N and q terms, the centring by mu_j cw_t inside the same absolute sums, a factor 8 for the constants).  The sums over
the draws add their own rounding: T 2^-53 sum_t |beta_ref| (and the same for the squares)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -53
DTYPES = {"f64": np.float64, "f32": np.float32, "u8": np.uint8}


def _genotypes(N, P, seed):
    rng = np.random.default_rng(seed)
    Z = rng.binomial(2, rng.uniform(0.1, 0.9, size=P), size=(N, P))
    Z[0], Z[1] = 0, 1   # every column polymorphic (method 2 refuses a monomorphic one)
    return Z


def _chain(ngp, Z, method, dtype, T, chain=0, k_src=None, enable=True, extra=None):
    """A records-only GBLUP chain, burn 2, keep T: (sampler, K or None for a sharer)."""
    N = Z.shape[0]
    y = np.random.default_rng(77).normal(size=N) + 0.3 * (Z[:, 0] - Z[:, 0].mean())
    s = ngp.Sampler(device=0, seed=5, chain=chain)
    s.set_records(N)
    s.set_residual_prior(4.0, 0.5)
    K = None
    if k_src is None:
        s.grm_begin(N, method); s.grm_columns(np.asfortranarray(Z.astype(dtype))); s.grm_end(); s.grm_invert()
        K = s.grm_get()
    s.add_random_set_dense(None, N, K=None if k_src is None else (k_src, 0), df=4.0, scale=0.5, varU0=1.0)
    if extra:
        extra(s, K)
    s.set_y(y); s.set_schedule(2 + T, 2, 1)
    if enable:
        s.enable_backsolve(0, T)
        s.run(2 + T)
    return s, K


def _ref(Z, K, U, method):
    """(sum, sumsq) over the draws with their tolerances, from beta_ref and the bound of the module's docstring."""
    Z = Z.astype(np.float64)
    N, P = Z.shape
    mu = Z.mean(axis=0)
    tp = mu * (1.0 - mu / 2.0)
    d = np.full(P, 1.0 / tp.sum()) if method == 1 else 1.0 / (P * tp)
    beta = d[:, None] * ((Z - mu).T @ (K @ U))
    b = 8.0 * (N + K.shape[0]) * EPS * d[:, None] * (np.abs(Z - mu).T @ (np.abs(K) @ np.abs(U)))
    T = U.shape[1]
    tol1 = b.sum(axis=1) + T * EPS * np.abs(beta).sum(axis=1)
    tol2 = ((2.0 * np.abs(beta) + b) * b).sum(axis=1) + (T + 1) * EPS * (beta ** 2).sum(axis=1)
    return beta.sum(axis=1), (beta ** 2).sum(axis=1), tol1, tol2


def _check(r, Z, K, U, method):
    s1, s2, tol1, tol2 = _ref(Z, K, U, method)
    e1, e2 = np.abs(r["sum"] - s1), np.abs(r["sumsq"] - s2)
    print(f"sum: worst error / bound {np.max(e1 / tol1):.3g}; sumsq: {np.max(e2 / tol2):.3g}")
    assert r["n"] == U.shape[1]
    assert np.all(e1 <= tol1) and np.all(e2 <= tol2)


# the smallest shapes that cross each boundary: a partial 64-row tile; a second column tile; a second 16-draw group; a second 64-draw
# group with a chunk boundary inside the call (the staging buffer is shrunk to 64 columns)
@pytest.mark.parametrize("N,P,T", [(37, 5, 1), (64, 70, 3), (130, 70, 17), (130, 129, 65)])
@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("kind", ["f64", "f32", "u8"])
def test_parity(ngp, kind, method, N, P, T):
    Z = _genotypes(N, P, seed=N + P)
    s, K = _chain(ngp, Z, method, DTYPES[kind], T)
    U = s.backsolve_draws(0)
    assert U.shape == (N, T)
    if P > 64:
        s.debug_set_staging_bytes(64 * N)
    r = s.backsolve(0, np.asfortranarray(Z.astype(DTYPES[kind])), splits=[P // 3 + 1])   # two calls of unequal size
    _check(r, Z, K, U, method)
    s.close()


def test_repeats_and_pools(ngp):
    N, P, T = 130, 70, 17
    Z = _genotypes(N, P, seed=3)
    a, K = _chain(ngp, Z, 1, np.uint8, T, enable=False)
    b, _ = _chain(ngp, Z, 1, np.uint8, T, chain=1, k_src=a, enable=False)
    for s in (a, b):
        s.enable_backsolve(0, T)
    ngp.Sampler.run_many([a, b], 2 + T)
    ra, ra2, rb = a.backsolve(0, Z.astype(np.uint8)), a.backsolve(0, Z.astype(np.uint8), splits=[9]), b.backsolve(0, Z.astype(np.float32))
    for k in ("sum", "sumsq"):
        assert np.array_equal(ra[k], ra2[k]), k   # the same bits, however the columns were split
    Ua, Ub = a.backsolve_draws(0), b.backsolve_draws(0)
    assert not np.array_equal(Ua, Ub)
    _check(ngp.pool_backsolve([ra, rb]), Z, K, np.concatenate([Ua, Ub], axis=1), 1)
    for s in (b, a):
        s.close()


def test_refusals_leave_a_usable_handle(ngp):
    N, P, T = 37, 5, 2
    Z = _genotypes(N, P, seed=1)

    def more(s, K):
        s.add_random_set((np.arange(N) % 4).astype(np.int32), 4, df=4.0, scale=1.0, varU0=1.0)   # set 1: CSR
        s.add_random_set_dense(None, N, K=(K + K.T) / 2 + np.eye(N), df=4.0, scale=0.5, varU0=1.0)   # set 2: the caller's K
        lv4 = (np.arange(N) % 4).astype(np.int32)
        s.add_random_set_hybrid(lv4, 4, np.eye(4), 1, D=np.eye(1), df=4.0, scale=1.0, varU0=1.0)     # set 3: hybrid (single-step)
        s.add_random_set_tuple(np.stack([lv4, lv4[::-1]]), 4, varU0=np.eye(2))                       # set 4: correlated (Tuple)

    s, K = _chain(ngp, Z, 1, np.float64, T, enable=False, extra=more)
    for rset in (1, 2, 3, 4, 7):                                      # ... and a set that does not exist
        with pytest.raises(ngp.NextGPHipError, match="error -1:"):
            s.enable_backsolve(rset, T)
    for bad in (0, 64 * 65535 + 1):
        with pytest.raises(ngp.NextGPHipError, match="error -1:"):
            s.enable_backsolve(0, bad)
    with pytest.raises(ngp.NextGPHipError, match="error -2:"):        # nothing enabled
        s.backsolve(0, Z)
    s.enable_backsolve(0, T)
    with pytest.raises(ngp.NextGPHipError, match="error -2:"):        # no kept draw yet
        s.backsolve(0, Z)
    s.run(2 + T)
    with pytest.raises(ngp.NextGPHipError, match="error -2:"):        # the run has started
        s.enable_backsolve(0, T)
    import ctypes as C
    s._chk(s.L.ngp_backsolve_begin(s.h, C.c_int32(0)))
    short = np.asfortranarray(Z[:N - 1].astype(np.float64))
    assert s.L.ngp_backsolve_columns_f64(s.h, short.ctypes.data_as(C.POINTER(C.c_double)), C.c_int64(P), C.c_int64(N - 1)) == -1   # N of the columns != q
    with pytest.raises(ngp.NextGPHipError, match="error -2:"):        # not all of the GRM's columns
        s._chk(s.L.ngp_backsolve_end(s.h, C.c_int32(0), None, None, None))
    with pytest.raises(ngp.NextGPHipError, match="error -1:"):        # more than the GRM's columns
        s.backsolve(0, np.concatenate([Z, Z], axis=1))
    with pytest.raises(ValueError, match="method"):                    # the set's matrix was built by method 1
        s.backsolve(0, Z, method=2)
    _check(s.backsolve(0, Z, method=1), Z, K, s.backsolve_draws(0), 1)   # ... and the handle still works
    s.set_y(np.zeros(N) + np.arange(N) % 3); s.enable_backsolve(0, 1)
    with pytest.raises(ngp.NextGPHipError, match="error -2:.*kept draws"):   # a kept draw beyond max_draws: an error, not a silent drop
        s.run(2 + T)
    s.close()


def test_runLMEM_snp_effects(ngp, tmp_path):
    from nextgp_jl_amd import api
    N, P = 60, 40
    Z = _genotypes(N, P, seed=8).astype(np.uint8)
    y = 10.0 + (Z[:, :4] - Z[:, :4].mean(axis=0)).sum(axis=1) + np.random.default_rng(4).normal(size=N)
    path = str(tmp_path / "g.npy")
    np.save(path, Z)
    VCV = {"M1": api.Random("G", 0.5 * y.var()), "e": api.Random("I", 0.5 * y.var())}
    out = str(tmp_path / "out")
    res = api.runLMEM(f'y ~ 1 + SNP(M1, "{path}")', dict(y=y), 30, 10, 2, outFolder=out, VCV=VCV, seed=3, snpEffects=True)
    snp = res["random"]["M1"]["snp"]
    with open(os.path.join(out, "snpEffectsM1.txt")) as f:
        lines = f.read().rstrip("\n").split("\n")
    assert lines[0].split("\t") == ["snp", "mean", "sd", "mean/sd"] and len(lines) == 1 + P and lines[1].split("\t")[0] == "M1"
    assert snp["n"] == 10 and np.all(snp["sd"] > 0)
    # linearity: the mean of the back-solved draws is the back-solve of the posterior-mean u
    s = ngp.Sampler(device=0)
    s.grm_begin(N, 1); s.grm_columns(Z); s.grm_end(); s.grm_invert()
    K = s.grm_get()
    s.close()
    ubar = np.asarray(res["random"]["M1"]["u"], dtype=np.float64)[:, None]
    m, _, tol, _ = _ref(Z, K, ubar, 1)
    # (the bound is linear in |u|: the mean of the draws' bounds is the bound at mean_t |u_t|; the division by n adds one rounding)
    uabs = np.abs(np.loadtxt(os.path.join(out, "uM1Out"), skiprows=1)).mean(axis=0)[:, None]
    _, _, tol, _ = _ref(Z, K, uabs, 1)
    assert np.all(np.abs(snp["mean"] - m) <= tol + 4 * EPS * np.abs(m))
    with pytest.raises(NotImplementedError, match="betaM1Out"):
        api.runLMEM(f'y ~ 1 + SNP(M1, "{path}")', dict(y=y), 30, 10, 2, outFolder=str(tmp_path / "o2"), VCV={"M1": api.BayesPR(P, 0.01), "e": VCV["e"]},
                    snpEffects=["M1"])
