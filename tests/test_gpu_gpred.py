"""GBLUP prediction of new individuals on the device (ngp_gpred_*; DESIGN.md section 2, "GBLUP prediction").  Shapes: N = 70 records (a
second 64-record tile), Nc = 1 / 65 candidates (a second 64-candidate tile), P = 134 columns as calls of 64 + 70 (a chunk boundary and
a tail that is no multiple of four) and as one call, T = 3 / 70 stored draws (a second 64-draw group), both GRM methods, f64 and u8
input (f32 once, on equal values).  The parity bounds are derived, not tuned: with A_ci = sum_j d_j |z_cj - mu_j| |z_ij - mu_j| and
B_it = sum_k |K_ik| |u_kt|, |m - m_ref| <= 8 (P + 2 N) 2^-53 sum_i A_ci B_it -- a chain of P products behind C, two chains of N behind
W and m, the centring (mu_j carries one rounding, which z - mu_j magnifies by at most N) inside the same absolute sums, and the factor
8 of the back-solve's bound for the constants."""
import ctypes as C
import os

import numpy as np
import pytest

from ref_gpred import EPS, L, reference

gpu = pytest.mark.gpu   # (the two host tests at the end run everywhere)
N, P = 70, 134
DTYPES = {"f64": np.float64, "f32": np.float32, "u8": np.uint8}
_cache = {}


def _genotypes(n, seed):
    rng = np.random.default_rng(seed)
    Z = rng.binomial(2, rng.uniform(0.1, 0.9, size=P), size=(n, P))
    Z[0], Z[1 % n] = 0, 1   # (records: every column polymorphic)
    return Z


def _fit(ngp, method, kind, T, extra=None):
    """A records-only GBLUP chain (burn 2, keep T) with its draw store, once per (method, kind, T): sampler, Z, G, K, U."""
    key = (method, kind, T, extra is not None)
    if key not in _cache:
        Z = _genotypes(N, 11)
        y = np.random.default_rng(77).normal(size=N) + 0.3 * (Z[:, 0] - Z[:, 0].mean())
        s = ngp.Sampler(device=0, seed=5)
        s.set_records(N)
        s.set_residual_prior(4.0, 0.5)
        s.grm_begin(N, method); s.grm_columns(np.asfortranarray(Z.astype(DTYPES[kind]))); s.grm_end()
        G = s.grm_get()
        s.grm_invert()
        K = s.grm_get()
        s.add_random_set_dense(None, N, df=4.0, scale=0.5, varU0=1.0)
        if extra:
            extra(s, K)
        s.set_y(y); s.set_schedule(2 + T, 2, 1); s.enable_backsolve(0, T); s.run(2 + T)
        _cache[key] = dict(s=s, Z=Z, G=G, K=K, U=s.backsolve_draws(0))
    return _cache[key]


def _typed(A, kind):
    return np.asfortranarray(A.astype(DTYPES[kind]))


def parity_bounds(ref, n, p, T):
    """The module's bound for C, gcc, s, sum and sumsq of n records, p columns and T draws, from the absolute sums of ref_gpred.reference
    (tests/test_gpu_gblup_edges.py imports it for its own shapes)."""
    c = 8.0 * (p + 2 * n) * EPS
    bm = c * (ref["A"] @ ref["B"])                                   # per (candidate, draw)
    return dict(C=c * ref["A"], gcc=c * ref["gcc"], s=c * (ref["gcc"] + ref["AKA"]),
                sum=bm.sum(axis=1) + T * EPS * np.abs(ref["m"]).sum(axis=1),
                sumsq=((2 * np.abs(ref["m"]) + bm) * bm).sum(axis=1) + (T + 1) * EPS * (ref["m"] ** 2).sum(axis=1))


@gpu
@pytest.mark.parametrize("kind,method,Nc", [(k, m, c) for k in ("f64", "u8") for m in (1, 2) for c in (1, 65)] + [("f32", 1, 65)])
def test_rows_of_G_bit_for_bit(ngp, kind, method, Nc):
    """Candidates with the genotypes of records get those records' rows of makeG's G: the same bits off the diagonal, and the diagonal
    without its ridge; 64 + 70 columns and one call of 134 give the same bits everywhere.  Their s_c has the closed form
    0.001 - 1e-6 K_rr (from C_c. = G_r. - 0.001 e_r' and K G = I).  Tolerance: 4 ulp (4 x 2^-52) of gcc_c + Q_c,
    Q_c = sum_ik |C_ci| |K_ik| |C_ck| -- what cancels in s_c.  Where the 4 comes from, in ulp of Q_c (at these shapes Q_c >= 300 gcc_c:
    every |K_ik| holds the 1 / (0.001 N) = 14.3 of the ones direction, which C annihilates only in the signed sum):
    (1) V_ic = sum_k K_ik C_ck and sum_i C_ci V_ic are chains of N terms of either sign.  Every rounding is relative to a partial
        sum, and a partial sum of n such terms is of the order of sqrt(n) of them where the absolute sum is n; n roundings of either
        sign add up like sqrt(n).  Together sqrt(n) 2^-53 (absolute sum / sqrt(n)): half an ulp of the absolute sum per chain, one
        ulp of Q_c for the two.  (All roundings aligned would give 2 N 2^-53 Q_c; the issue asks for the few ulp, not for that.)
    (2) gcc_c is a chain of P positive terms in another association than C_cr: sqrt(P) 2^-53 gcc_c, 6 ulp of gcc_c, 0.02 ulp of Q_c.
    (3) K is the inverse rocSOLVER's Cholesky computed, K = inv(G + E) with E_rr of the order N 2^-53 G_rr (backward stability of
        potrf / potri).  To first order C_c. K C_c.' moves by E_rr (K C_c.' is e_r up to the ridge): 35 ulp of gcc_c, 0.12 ulp of Q_c;
        the 1e-6 K_rr of the closed form moves by 1e-6 of K's own error.
    The sum is 1.2 ulp; 4 leaves a factor of three for the constants of (1)."""
    f = _fit(ngp, method, "u8", 3)
    rows = np.array([5]) if Nc == 1 else (np.arange(Nc) * 3 + 2) % N
    Zt, Zc = _typed(f["Z"], kind), _typed(f["Z"][rows], kind)
    a = f["s"].gblup_predict(0, Zt, Zc, splits=[64]); Ca = f["s"].gblup_cross()
    b = f["s"].gblup_predict(0, Zt, Zc, splits=[]); Cb = f["s"].gblup_cross()
    assert np.array_equal(Ca, Cb) and all(np.array_equal(a[k], b[k]) for k in ("sum", "sumsq", "s", "gcc")) and a["n"] == b["n"] == 3
    G = ngp.makeG(f["Z"].astype(np.uint8), method)
    assert np.array_equal(G, f["G"])
    diag = np.zeros_like(Ca, dtype=bool); diag[np.arange(Nc), rows] = True
    assert np.array_equal(Ca[~diag], G[rows][~diag])
    assert np.array_equal(Ca[diag] + 0.001, G[rows, rows])
    K = f["K"]
    Q = ((np.abs(Ca) @ np.abs(K)) * np.abs(Ca)).sum(axis=1)
    assert np.all(Q >= 300.0 * a["gcc"])   # (what the derivation of the 4 ulp rests on)
    tol = 4.0 * 2.0 ** -52 * (a["gcc"] + Q)
    err = np.abs(a["s"] - (0.001 - 1e-6 * K[rows, rows]))
    print(f"s closed form: worst error / tolerance {np.max(err / tol):.3g} (s about {a['s'].mean():.3g})")
    assert np.all(err <= tol)


@gpu
@pytest.mark.parametrize("T", [3, 70])
@pytest.mark.parametrize("Nc", [1, 65])
@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("kind", ["f64", "u8"])
def test_parity_and_the_two_device_paths(ngp, kind, method, Nc, T):
    """C, sum, sumsq, s and gcc against the longdouble reference inside the module's bound; then sum_t m_ct against
    sum_j (z_cj - mu_j) sum_beta[j] of the back-solve on the same draws, inside the sum of both bounds (the back-solve's:
    8 (N + q) 2^-53 d_j sum_i |z_ij - mu_j| B_it per entry, T 2^-53 |beta| for its sums)."""
    f = _fit(ngp, method, kind, T)
    Zc = _genotypes(Nc, 100 + Nc)
    r = f["s"].gblup_predict(0, _typed(f["Z"], kind), _typed(Zc, kind), splits=[64])
    Cd = f["s"].gblup_cross()
    ref = reference(f["Z"], Zc, f["K"], f["U"], method)
    tol = parity_bounds(ref, N, P, T)
    got = dict(C=Cd, gcc=r["gcc"], s=r["s"], sum=r["sum"], sumsq=r["sumsq"])
    frac = {k: float(np.max(np.abs(got[k].astype(L) - ref[k]) / tol[k])) for k in tol}
    print("worst error / bound:", {k: f"{v:.3g}" for k, v in frac.items()})
    assert r["n"] == T and all(v <= 1.0 for v in frac.values()), frac
    bs = f["s"].backsolve(0, _typed(f["Z"], kind))
    via_beta = ref["Xc"] @ bs["sum"].astype(L)
    tol2 = tol["sum"] + (8.0 * 2 * N + T) * EPS * ref["beta_abs"]
    assert np.all(np.abs(r["sum"].astype(L) - via_beta) <= tol2)
    assert np.allclose(r["mean"], r["sum"] / T) and np.all(r["sd"] ** 2 >= np.maximum(r["s"], 0) * r["sum_varU"] / T * (1 - 1e-12))


@gpu
def test_runLMEM_predicts_gblup_candidates(ngp, tmp_path):
    Z, Zc = _genotypes(N, 11).astype(np.uint8), _genotypes(7, 21).astype(np.uint8)
    y = 10.0 + (Z[:, :4] - Z[:, :4].mean(axis=0)).sum(axis=1) + np.random.default_rng(4).normal(size=N)
    path = str(tmp_path / "g.npy")
    np.save(path, Z)
    VCV = {"M1": ngp.Random("G", 0.5 * y.var()), "e": ngp.Random("I", 0.5 * y.var())}
    out = str(tmp_path / "out")
    res = ngp.runLMEM(f'y ~ 1 + SNP(M1, "{path}")', dict(y=y), 30, 10, 2, outFolder=out, VCV=VCV, seed=3, chains=2, predict={"M1": Zc},
                      predict_ids=[f"c{i}" for i in range(7)])
    pr = res["predict"]
    assert pr["ids"][0] == "c0" and set(pr["sets"]["M1"]) >= {"mean", "sd", "s"} and pr["nKept"] == 20
    parts = [r["predict"]["sets"]["M1"] for r in res["chains"]]
    pooled = pr["sets"]["M1"]
    for k in ("sum", "sumsq"):
        assert np.array_equal(pooled[k], parts[0][k] + parts[1][k]), k
    assert pooled["n"] == 20 and pooled["sum_varU"] == parts[0]["sum_varU"] + parts[1]["sum_varU"]
    assert np.array_equal(pr["mean"], pooled["sum"] / 20) and np.array_equal(pr["sd"], pooled["sd"])
    assert np.all(pooled["s"] > 0) and np.all(pooled["sd"] ** 2 >= pooled["s"] * pooled["sum_varU"] / 20 * (1 - 1e-12))
    with open(os.path.join(out, "gebvPredict.txt")) as fh:
        lines = fh.read().rstrip("\n").split("\n")
    assert lines[0].split("\t") == ["ID", "mean", "sd", "mean_M1", "sd_M1"] and len(lines) == 8
    assert float(lines[1].split("\t")[3]) == pooled["mean"][0]


def _others(s, K):
    lv4 = (np.arange(N) % 4).astype(np.int32)
    s.add_random_set(lv4, 4, df=4.0, scale=1.0, varU0=1.0)                                       # set 1: CSR
    s.add_random_set_dense(None, N, K=(K + K.T) / 2 + np.eye(N), df=4.0, scale=0.5, varU0=1.0)   # set 2: the caller's K
    s.add_random_set_hybrid(lv4, 4, np.eye(4), 1, D=np.eye(1), df=4.0, scale=1.0, varU0=1.0)     # set 3: hybrid (single-step)
    s.add_random_set_tuple(np.stack([lv4, lv4[::-1]]), 4, varU0=np.eye(2))                       # set 4: correlated (Tuple)


def _cols(s, Zt, Zc, ldt=None, ldc=None, ncol=None):
    p = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    return s.L.ngp_gpred_columns_f64(s.h, p(Zt), C.c_int64(ldt or Zt.shape[0]), p(Zc), C.c_int64(ldc or Zc.shape[0]), C.c_int64(ncol or Zt.shape[1]))


REFUSALS = {
    "csr": (-1, lambda s, Zt, Zc: s.L.ngp_gpred_begin(s.h, C.c_int32(1), C.c_int64(3))),
    "caller_K": (-1, lambda s, Zt, Zc: s.L.ngp_gpred_begin(s.h, C.c_int32(2), C.c_int64(3))),
    "hybrid": (-1, lambda s, Zt, Zc: s.L.ngp_gpred_begin(s.h, C.c_int32(3), C.c_int64(3))),
    "tuple": (-1, lambda s, Zt, Zc: s.L.ngp_gpred_begin(s.h, C.c_int32(4), C.c_int64(3))),
    "no_candidate": (-1, lambda s, Zt, Zc: s.L.ngp_gpred_begin(s.h, C.c_int32(0), C.c_int64(0))),
    "second_begin": (-2, lambda s, Zt, Zc: s.L.ngp_gpred_begin(s.h, C.c_int32(0), C.c_int64(3)) or s.L.ngp_gpred_begin(s.h, C.c_int32(0), C.c_int64(3))),
    "ld_small": (-1, lambda s, Zt, Zc: s.L.ngp_gpred_begin(s.h, C.c_int32(0), C.c_int64(3)) or _cols(s, Zt, Zc, ldt=N - 1)),
    "non_finite": (-1, lambda s, Zt, Zc: s.L.ngp_gpred_begin(s.h, C.c_int32(0), C.c_int64(3)) or _cols(s, Zt, np.asfortranarray(Zc * np.where(np.arange(P) == 9, np.nan, 1.0)))),
    "too_many": (-1, lambda s, Zt, Zc: s.L.ngp_gpred_begin(s.h, C.c_int32(0), C.c_int64(3)) or _cols(s, Zt[:, :128], Zc[:, :128]) or _cols(s, Zt[:, :64], Zc[:, :64])),
    "end_early": (-2, lambda s, Zt, Zc: s.L.ngp_gpred_begin(s.h, C.c_int32(0), C.c_int64(3)) or _cols(s, Zt[:, :64], Zc[:, :64])
                  or s.L.ngp_gpred_end(s.h, C.c_int32(0), None, None, None, None, None)),
    "backsolve_open": (-2, lambda s, Zt, Zc: s.L.ngp_backsolve_begin(s.h, C.c_int32(0)) or s.L.ngp_gpred_begin(s.h, C.c_int32(0), C.c_int64(3))),
    "cross_ld_small": (-1, lambda s, Zt, Zc: s.L.ngp_gpred_get_cross(s.h, np.empty((3, N)).ctypes.data_as(C.POINTER(C.c_double)), C.c_int64(N - 1))),
}


@gpu
@pytest.mark.parametrize("case", list(REFUSALS))
def test_refusals_leave_a_usable_handle(ngp, case):
    f = _fit(ngp, 1, "f64", 3, extra=_others)
    s, Zt, Zc = f["s"], _typed(f["Z"], "f64"), _typed(_genotypes(3, 9), "f64")
    want, call = REFUSALS[case]
    ok = s.gblup_predict(0, Zt, Zc)
    assert call(s, Zt, Zc) == want
    s.L.ngp_gpred_abort(s.h)
    if case == "backsolve_open":
        s.backsolve(0, Zt)   # (closes it)
    again = s.gblup_predict(0, Zt, Zc)
    assert all(np.array_equal(ok[k], again[k]) for k in ("sum", "sumsq", "s", "gcc"))


def test_candidate_bed_is_imputed_at_the_records_means(ngp, tmp_path):
    """Host only: a candidate fileset is decoded by decode_bed under the run's policy, a missing call at the RECORDS' column mean (rounded
    under "round", refused under "error"); other SNP IDs than the records' fileset are refused."""
    api = __import__(ngp.__name__ + ".api", fromlist=["api"])
    rng = np.random.default_rng(0)
    Z, Zc = rng.integers(0, 3, size=(20, 9)), rng.integers(0, 3, size=(5, 9))
    miss = np.zeros(Zc.shape, dtype=bool); miss[1, 2] = miss[4, 0] = True
    bed, gblup = ngp.write_plink(str(tmp_path / "c"), Zc, missing=miss), {"M1": dict(M=Z.astype(np.float64))}
    want = Zc.astype(np.float64); want[miss] = np.broadcast_to(Z.mean(axis=0), Zc.shape)[miss]
    src = lambda policy, **kw: api._gblup_prediction_sources({"M1": bed}, None, [], gblup, None, 1, policy, 5, None, **kw)
    got = src("mean")
    assert np.array_equal(got["M"]["M1"], want) and got["ids"] == ["1", "2", "3", "4", "5"]
    assert np.array_equal(src("round")["M"]["M1"], np.floor(want + 0.5)) and src("round")["M"]["M1"].dtype == np.uint8
    with pytest.raises(ValueError, match="missing calls"):
        src("error")
    other = api._genotype_source(ngp.write_plink(str(tmp_path / "t"), Z, snp=[f"rs{j}" for j in range(9)]), None, 1, "mean")
    with pytest.raises(ValueError, match="SNP IDs"):
        src("mean", bed_sets={"M1": other})


def test_runLMEM_refuses_single_step_prediction(ngp, tmp_path):
    """Host only: predict= naming a Random("H", v) term is refused with its reason before any device work."""
    import ref_pedigree as RP
    D = RP.PBLUP_DATA
    data = dict(ID=np.array([r[0] for r in D]), BW=np.array([r[5] for r in D]))
    geno = np.random.default_rng(1).integers(0, 3, size=(3, 40)).astype(np.uint8)
    with pytest.raises(NotImplementedError, match="single-step"):
        ngp.runLMEM("BW ~ 1 + PED(ID)", data, 6, 2, 2, outFolder=str(tmp_path / "o"), userPedData=RP.PBLUP_PED, VCV={"ID": ngp.Random("H", 150.0)},
                    singleStep={"ID": {"geno": geno, "ids": ["QGG5", "QGG9", "QGG12"], "w": 0.05}}, predict={"ID": geno})
