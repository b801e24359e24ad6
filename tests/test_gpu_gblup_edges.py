"""GBLUP back-solve and candidate prediction at padded leading dimensions, chunk seams inside a call, tile edges and real-valued
dosages ("SNP effects from GBLUP" and "GBLUP prediction"), and ngp_grm_single_step at ld > N.  No tolerance here is
new: every comparison is np.array_equal against the one-call contiguous default-staging run of the same handle, or a bound imported
from test_gpu_gpred.py (parity_bounds) / test_gpu_backsolve.py (_ref, _check) with the case's own N, P and T.

What each section would catch, from the code (csrc/ngp_api.hip, ngp_gpred.h, ngp_backsolve.h, ngp_grm_stats.h):
A  gpred_columns_t: the copy length `(nc - 1) * ldt + N` (and its ldc twin) taken as `nc * N` leaves the tail of a padded chunk
   unstaged; the host offset `Mt + c0 * ldt` taken as `c0 * N` stages the wrong columns from the second chunk on; `g.bytes_t < need_t`
   not regrowing when ld grows between calls is a short device buffer.  k_gp_colstats: `i < Nc` -> `i < ldc`, or grm_col_stats'
   `i < N` -> `i < ld`, sees NaN / inf in the padding and the call is refused (255 moves mu_j).  k_gp_cross: `pa[j * ldc]` / `pb[j * ldt]`
   addressed with the row count, `on = j < nc` -> `j < cpad` (the 5-column last chunk then reads the columns 5 .. 7 the 64-column chunk
   before it left in the staging buffer, with that chunk's mu), and the chain's start `acc = Ct[...]`, `gc = gcc[c0 + l]` replaced
   by zeros at a chunk all change bits against the one-chunk run.
B  k_gp_cross: `cpad = (nc + 3) / 4 * 4` -> `nc / 4 * 4` drops the last 3, 1, 1, 3 columns of P = 3, 33, 197, 71; `nk` taken as
   NGP_GP_KT / 4 on the last tile multiplies stale LDS rows at P = 3, 33, 71, 197; the prefetch guard `j0 + NGP_GP_KT < cpad` moved
   one tile early (`j0 + 2 * NGP_GP_KT < cpad`) repeats the tile before the last at P = 64, 71, 197 (moved late, `<=`, it is harmless:
   `on` predicates every load of the request off); `wave_gcc` without `w == 0` adds gcc four times; `i0 = 64 * blockIdx.y` and the
   third tile of either grid axis at 129 x 130; N = 9 leaves the record groups g = 1 .. 3 to `onB` alone.
C  `double x = (double)z - m` on a float taken through an integer or a half conversion, or a float column addressed as doubles,
   changes nothing on 0 / 1 / 2 and every value of a dosage; f32 against f64 on equal values must agree to the bit.
D  backsolve_columns_t: `(nc - 1) * ld + N` -> `nc * N`, `M + c0 * ld` -> `c0 * N`, `B.stage_bytes < need`; k_bs_colstats through
   grm_col_stats `i < N`; k_bs_cols: `src + jA * ld`, bs_load16's `i + 15 < N` (row tile 128 .. 143 of N = 130 ends in the padding) and
   the dword path of bytes, whose alignment changes column by column at ld = 173.
E  ngp_grm_single_step: the symmetry scan `A22[i * ld + j]` and hipMemcpy2D's source pitch `ld * sizeof(double)` taken with N.
Not every predicate can show in an output: rows of the records beyond N feed accumulators that are never stored, candidates beyond Nc
columns of C that nothing reads back, and `on` guards a tail column twice (at the request and at the LDS write) -- a single mutation
of those is harmless, and no case here claims to see it.  Measured on an MI355X: 120 cases in 2.9 s, no case above 0.3 s; the worst
fractions of the bounds are 0.011 (C, at 9 x 1 x 3), 0.0093 (gcc), 1.4e-4 (s), 2.5e-4 (sum), 2.7e-4 (sumsq)."""
import ctypes as C

import numpy as np
import pytest

import ref_gblup as RG
import ref_pedigree as RP
from layout_helpers import PAD, assert_poisoned, assert_short, leading_dimension, padded, short_buffer
from ref_gpred import L, reference
from test_gpu_backsolve import _check as bs_check
from test_gpu_gpred import parity_bounds

gpu = pytest.mark.gpu   # (the host test of the helpers at the end runs everywhere)
DTYPES = {"f64": np.float64, "f32": np.float32, "u8": np.uint8}
CT = {"f64": C.c_double, "f32": C.c_float, "u8": C.c_uint8}
KEYS = ("sum", "sumsq", "s", "gcc", "C")
_fits, _base = {}, {}


def _counts(n, P, seed):
    rng = np.random.default_rng(seed)
    Z = rng.binomial(2, rng.uniform(0.1, 0.9, size=P), size=(n, P))
    Z[0], Z[1 % n] = 0, 1   # (records: every column polymorphic, as method 2 requires)
    return Z


def _dosages(n, P, seed):
    """Counts plus uniform noise, clipped to [0, 2] and rounded to float32: what both input types hold."""
    D = np.clip(_counts(n, P, seed) + np.random.default_rng(seed + 1000).uniform(-0.45, 0.45, size=(n, P)), 0.0, 2.0).astype(np.float32)
    assert np.mean(D != np.rint(D)) > 0.5 and np.all(D.max(axis=0) > D.min(axis=0))
    return D


def _typed(A, kind):
    out = np.asfortranarray(A.astype(DTYPES[kind]))
    assert np.array_equal(out.astype(np.float64), np.asarray(A, dtype=np.float64))   # (every type holds equal numbers)
    return out


def _fit(ngp, N, P, T, method, dosage=False):
    """A records-only GBLUP chain (burn 2, keep T) with its draw store, fitted once per case from the f64 input: sampler, Z, Zc maker, K, U."""
    key = (N, P, T, method, dosage)
    if key not in _fits:
        Z = (_dosages if dosage else _counts)(N, P, 11 + N + P)
        y = np.random.default_rng(77).normal(size=N) + 0.3 * (Z[:, 0] - Z[:, 0].mean())
        s = ngp.Sampler(device=0, seed=5)
        s.set_records(N)
        s.set_residual_prior(4.0, 0.5)
        s.grm_begin(N, method); s.grm_columns(np.asfortranarray(Z.astype(np.float64))); s.grm_end(); s.grm_invert()
        K = s.grm_get()
        s.add_random_set_dense(None, N, df=4.0, scale=0.5, varU0=1.0)
        s.set_y(y); s.set_schedule(2 + T, 2, 1); s.enable_backsolve(0, T); s.run(2 + T)
        U = s.backsolve_draws(0)
        assert U.shape == (N, T)
        _fits[key] = dict(s=s, Z=Z, K=K, U=U)
    return _fits[key]


def _candidates(Nc, P, dosage=False):
    return (_dosages if dosage else _counts)(Nc, P, 100 + Nc + P)


# ---- the C entry points, with an explicit leading dimension ------------------------------------------------------------------------
def _ptr(a):
    return a.ctypes.data_as(C.POINTER(CT[{1: "u8", 4: "f32", 8: "f64"}[a.itemsize]]))


def _sfx(a):
    return {np.dtype(np.uint8): "u8", np.dtype(np.float32): "f32", np.dtype(np.float64): "f64"}[a.dtype]


def _predict(s, N, Nc, calls, staging=0):
    """ngp_gpred_begin, one ngp_gpred_columns_* per (train, ldt, cand, ldc, ncol) of `calls` (arrays or flat short buffers of one type),
    ngp_gpred_end and ngp_gpred_get_cross; `staging` bytes per chunk for the calls (0: the 256 MiB), the default again afterwards."""
    s.debug_set_staging_bytes(staging)
    try:
        s._chk(s.L.ngp_gpred_begin(s.h, C.c_int32(0), C.c_int64(Nc)))
        try:
            for Zt, ldt, Zc, ldc, ncol in calls:
                assert Zt.dtype == Zc.dtype
                s._chk(getattr(s.L, "ngp_gpred_columns_" + _sfx(Zt))(s.h, _ptr(Zt), C.c_int64(ldt), _ptr(Zc), C.c_int64(ldc), C.c_int64(ncol)))
            out = {k: np.empty(Nc) for k in ("sum", "sumsq", "s", "gcc")}
            n = C.c_int64()
            s._chk(s.L.ngp_gpred_end(s.h, C.c_int32(0), *(out[k].ctypes.data_as(C.POINTER(C.c_double)) for k in ("sum", "sumsq", "s", "gcc")), C.byref(n)))
        except Exception:
            s.L.ngp_gpred_abort(s.h)
            raise
        out["C"] = np.empty((Nc, N))
        s._chk(s.L.ngp_gpred_get_cross(s.h, out["C"].ctypes.data_as(C.POINTER(C.c_double)), C.c_int64(N)))
        out["n"] = n.value
        return out
    finally:
        s.debug_set_staging_bytes(0)


def _whole(Zt, Zc):
    return [(Zt, leading_dimension(Zt), Zc, leading_dimension(Zc), Zt.shape[1])]


def _split(Zt, Zc, cut, Zt2=None, Zc2=None):
    """Two calls, columns [0, cut) of (Zt, Zc) and [cut, P) of (Zt2, Zc2) (default: the same arrays)."""
    Zt2, Zc2 = Zt if Zt2 is None else Zt2, Zc if Zc2 is None else Zc2
    a, b = (Zt[:, :cut], Zc[:, :cut]), (Zt2[:, cut:], Zc2[:, cut:])
    return [(t, leading_dimension(t), c, leading_dimension(c), t.shape[1]) for t, c in (a, b)]


def _same(got, want, keys=KEYS):
    for k in keys:
        assert np.array_equal(got[k], want[k]), f"{k}: {int(np.sum(got[k] != want[k]))} of {want[k].size} entries differ from the one-call contiguous run"
    assert got["n"] == want["n"]


# ---- A. prediction: layout and chunking do not show in the bits --------------------------------------------------------------------
AN, ANC, AP, AT = 70, 65, 197, 3


def _layout_case(ngp, kind, method):
    f = _fit(ngp, AN, AP, AT, method)
    Zt, Zc = _typed(f["Z"], kind), _typed(_candidates(ANC, AP), kind)
    key = (kind, method)
    if key not in _base:
        _base[key] = _predict(f["s"], AN, ANC, _whole(Zt, Zc))
        assert _base[key]["n"] == AT and np.all(np.isfinite(_base[key]["C"])) and np.all(_base[key]["gcc"] > 0)
    return f["s"], Zt, Zc, _base[key]


def _chunk64(*arrays):
    """Staging bytes under which a gpred / back-solve call takes its columns 64 at a time: 64 columns of the arrays' leading dimensions."""
    return 64 * sum(leading_dimension(a) for a in arrays) * arrays[0].itemsize


LAYOUTS = ["seam", "seam_and_calls", "padded", "padded_chunks", "short", "short_chunks", "mixed", "mixed_reverse"]


@gpu
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("kind", ["f64", "f32", "u8"])
def test_prediction_layouts_bit_for_bit(ngp, kind, method, layout):
    """N = 70, Nc = 65, P = 197: sum, sumsq, s, gcc and C of every layout equal the one-call contiguous default-staging run.
    seam: 64 columns per chunk, one call (chunks of 64, 64, 64, 5); seam_and_calls: the same chunks in calls of 128 + 69; padded:
    ldt = N + 43, ldc = Nc + 43 over NaN / inf / 255, through Sampler.gblup_predict (the view's leading dimension must arrive);
    padded_chunks: the same in calls of 64 + 133, 64 columns per chunk; short / short_chunks: buffers that end with the last column's
    N / Nc elements; mixed / mixed_reverse: calls of 128 + 69, one contiguous and one padded (the staging buffers grow, or are reused
    oversized)."""
    s, Zt, Zc, base = _layout_case(ngp, kind, method)
    if layout == "seam":
        got = _predict(s, AN, ANC, _whole(Zt, Zc), staging=_chunk64(Zt, Zc))
    elif layout == "seam_and_calls":
        got = _predict(s, AN, ANC, _split(Zt, Zc, 128), staging=_chunk64(Zt, Zc))
    elif layout in ("padded", "padded_chunks"):
        Pt, Pc = padded(Zt), padded(Zc)
        assert assert_poisoned(Pt) == AN + PAD and assert_poisoned(Pc) == ANC + PAD
        cuts = [64] if layout == "padded_chunks" else []
        for V in (Pt, Pc):   # what the wrapper hands over: the view itself with the parent's leading dimension, not a copy
            for a, b in zip([0] + cuts, cuts + [AP]):
                A, _, sfx, ld = ngp._lib._columns(V[:, a:b])
                assert A.ctypes.data == V[:, a:b].ctypes.data and ld == V.shape[0] + PAD and sfx == kind
        s.debug_set_staging_bytes(_chunk64(Pt, Pc) if cuts else 0)
        try:
            got = s.gblup_predict(0, Pt, Pc, splits=cuts)
            got["C"] = s.gblup_cross()
        finally:
            s.debug_set_staging_bytes(0)
    elif layout in ("short", "short_chunks"):
        ft, fc = short_buffer(Zt, AN + PAD), short_buffer(Zc, ANC + PAD)
        assert_short(ft, Zt, AN + PAD); assert_short(fc, Zc, ANC + PAD)
        got = _predict(s, AN, ANC, [(ft, AN + PAD, fc, ANC + PAD, AP)], staging=64 * (AN + ANC + 2 * PAD) * Zt.itemsize if layout == "short_chunks" else 0)
    else:
        Pt, Pc = padded(Zt), padded(Zc)
        assert_poisoned(Pt); assert_poisoned(Pc)
        calls = _split(Zt, Zc, 128, Pt, Pc) if layout == "mixed" else _split(Pt, Pc, 128, Zt, Zc)
        assert sorted((c[1], c[3]) for c in calls) == [(AN, ANC), (AN + PAD, ANC + PAD)]
        got = _predict(s, AN, ANC, calls)
    _same(got, base)


@gpu
def test_prediction_candidates_at_ld_2_to_19(ngp):
    """u8, method 1: the candidates alone padded, ldc = 2^19 over untouched zero pages (the records contiguous): 197 x 512 KiB of host
    memory in one strided copy, and `j * ldc` in the kernels far past what 32-bit element offsets of a padded N would show."""
    s, Zt, Zc, base = _layout_case(ngp, "u8", 1)
    big = np.zeros((2 ** 19, AP), dtype=np.uint8, order="F")
    big[:ANC] = Zc
    view = big[:ANC]
    assert leading_dimension(view) == 2 ** 19 and np.array_equal(view, Zc)
    _same(_predict(s, AN, ANC, _whole(Zt, view)), base)


# ---- B. prediction: tile edges against the longdouble reference ---------------------------------------------------------------------
SHAPES = [(9, 1, 3), (64, 64, 64), (64, 64, 32), (65, 128, 33), (129, 130, 71), (70, 65, 197)]   # N, Nc, P
EDGES = ([(sh, k, m, 3) for i, sh in enumerate(SHAPES) for k in ("f64", "u8") + (("f32",) if i in (0, 3, 4) else ()) for m in (1, 2)]
         + [((129, 130, 71), "f64", 1, 70)])


def _parity(got, Zt, Zc, f, method, T):
    """C, gcc, s, sum and sumsq inside test_gpu_gpred.parity_bounds of the longdouble reference formed from the values as stored."""
    N, P = Zt.shape
    ref = reference(Zt, Zc, f["K"], f["U"], method)
    tol = parity_bounds(ref, N, P, T)
    frac = {k: float(np.max(np.abs(got[k].astype(L) - ref[k]) / tol[k])) for k in tol}
    print("worst error / bound:", {k: f"{v:.3g}" for k, v in frac.items()})
    assert got["n"] == T and all(v <= 1.0 for v in frac.values()), frac


@gpu
@pytest.mark.parametrize("shape,kind,method,T", EDGES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_prediction_tile_edges(ngp, shape, kind, method, T):
    """9 x 1 x 3: fewer than four columns, one record group partly on and three off; 64 x 64 x 64 and x 32: exact tiles everywhere, no
    partial LDS tile (the prefetch guard on the last step), exactly one tile; 65 x 128 x 33: one column past a tile (nk = 1), exact
    candidate tiles, one record past; 129 x 130 x 71: a third tile on both grid axes, P = 3 mod 4 (T = 70 once: a second 64-draw group);
    70 x 65 x 197: the layout case, P = 1 mod 4."""
    N, Nc, P = shape
    f = _fit(ngp, N, P, T, method)
    Zt, Zc = _typed(f["Z"], kind), _typed(_candidates(Nc, P), kind)
    _parity(_predict(f["s"], N, Nc, _whole(Zt, Zc)), Zt, Zc, f, method, T)


# ---- C. real-valued dosages ---------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("shape", [(65, 128, 33), (129, 130, 71)], ids=lambda v: "x".join(map(str, v)))
def test_prediction_dosages(ngp, shape, method):
    """Dosages in f32 and in f64 holding the same numbers: each inside the bound of the reference formed from the values as stored, and
    C, gcc, s (and the sums) of the two types equal to the bit -- the kernels' first operation is (double)z in either type."""
    N, Nc, P = shape
    f = _fit(ngp, N, P, 3, method, dosage=True)
    Dc = _candidates(Nc, P, dosage=True)
    got = {}
    for kind in ("f32", "f64"):
        Zt, Zc = _typed(f["Z"], kind), _typed(Dc, kind)
        assert Zt.dtype == DTYPES[kind] and np.any(Zt != np.rint(Zt))
        got[kind] = _predict(f["s"], N, Nc, _whole(Zt, Zc))
        _parity(got[kind], Zt, Zc, f, method, 3)
    _same(got["f32"], got["f64"])


# ---- D. back-solve: the same holes --------------------------------------------------------------------------------------------------
BN, BP, BT = 130, 129, 17
BS_LAYOUTS = ["padded", "short", "three_chunks", "chunks_and_calls", "mixed"]


def _backsolve(s, calls, P, staging=0):
    """ngp_backsolve_begin, one ngp_backsolve_columns_* per (buffer, ncol, ld), ngp_backsolve_end."""
    s.debug_set_staging_bytes(staging)
    try:
        s._chk(s.L.ngp_backsolve_begin(s.h, C.c_int32(0)))
        for M, ncol, ld in calls:
            s._chk(getattr(s.L, "ngp_backsolve_columns_" + _sfx(M))(s.h, _ptr(M), C.c_int64(ncol), C.c_int64(ld)))
        s1, s2, n = np.empty(P), np.empty(P), C.c_int64()
        s._chk(s.L.ngp_backsolve_end(s.h, C.c_int32(0), s1.ctypes.data_as(C.POINTER(C.c_double)), s2.ctypes.data_as(C.POINTER(C.c_double)), C.byref(n)))
        return dict(sum=s1, sumsq=s2, n=n.value)
    finally:
        s.debug_set_staging_bytes(0)


def _padded_for_the_wrapper(ngp, Z):
    """padded(Z), checked on the host: poison below the rows, and Sampler.backsolve's _columns hands the view over as it is."""
    big = padded(Z)
    N = Z.shape[0]
    assert assert_poisoned(big) == N + PAD and big.strides[1] // big.itemsize == N + PAD
    A, _, _, ld = ngp._lib._columns(big[:, 0:big.shape[1]])
    assert A.ctypes.data == big.ctypes.data and ld == N + PAD
    return big


@gpu
@pytest.mark.parametrize("layout", BS_LAYOUTS)
@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("kind", ["f64", "f32", "u8"])
def test_backsolve_layouts_bit_for_bit(ngp, kind, method, layout):
    """N = 130, P = 129, T = 17: sum and sumsq of every layout equal Sampler.backsolve's one call at the default staging.  padded:
    ld = N + 43 over NaN / inf / 255, through the wrapper; short: the buffer ends with the last column's N elements; three_chunks: 64
    columns per chunk, one call (64, 64, 1); chunks_and_calls: the same staging, calls of 64 + 65; mixed: 64 contiguous columns, then 65
    padded ones, and the reverse."""
    f = _fit(ngp, BN, BP, BT, method)
    s, Z = f["s"], _typed(f["Z"], kind)
    key = ("bs", kind, method)
    if key not in _base:
        _base[key] = s.backsolve(0, Z)
        assert _base[key]["n"] == BT and np.all(np.isfinite(_base[key]["sum"])) and np.all(_base[key]["sumsq"] > 0)
    base, keys = _base[key], ("sum", "sumsq")
    if layout == "padded":
        _same(s.backsolve(0, _padded_for_the_wrapper(ngp, Z)), base, keys)
    elif layout == "short":
        flat = short_buffer(Z, BN + PAD)
        assert_short(flat, Z, BN + PAD)
        _same(_backsolve(s, [(flat, BP, BN + PAD)], BP), base, keys)
    elif layout == "three_chunks":
        _same(_backsolve(s, [(Z, BP, BN)], BP, staging=_chunk64(Z)), base, keys)
    elif layout == "chunks_and_calls":
        _same(_backsolve(s, [(Z[:, :64], 64, BN), (Z[:, 64:], 65, BN)], BP, staging=_chunk64(Z)), base, keys)
    else:
        big = _padded_for_the_wrapper(ngp, Z)
        _same(_backsolve(s, [(Z[:, :64], 64, BN), (big[:, 64:], 65, BN + PAD)], BP), base, keys)
        _same(_backsolve(s, [(big[:, :64], 64, BN + PAD), (Z[:, 64:], 65, BN)], BP), base, keys)


@gpu
@pytest.mark.parametrize("method", [1, 2])
@pytest.mark.parametrize("kind", ["f64", "f32"])
def test_backsolve_padded_dosages(ngp, kind, method):
    """Dosages at ld = N + 43 through the wrapper, against test_gpu_backsolve's reference and bound (imported, unchanged)."""
    f = _fit(ngp, BN, BP, BT, method, dosage=True)
    Z = _typed(f["Z"], kind)
    bs_check(f["s"].backsolve(0, _padded_for_the_wrapper(ngp, Z)), Z, f["K"], f["U"], method)


# ---- E. single-step: A22 as the corner of a larger array ---------------------------------------------------------------------------
@gpu
def test_single_step_leading_dimension(ngp, O):
    """n_g = 65 (test_gpu_singlestep's smallest corner block): A22 as the top-left corner of an (N + 5) x (N + 5) array of NaN, ld = N + 5
    through the C entry point, gives grm_get() of the contiguous call to the bit."""
    ng, w = 65, 0.05
    s_, d_ = RP.random_pedigree(300, 20)
    F, _ = ngp.pedigree_ainv(s_, d_)
    A22 = ngp.pedigree_a22(s_, d_, F, np.random.default_rng(ng).permutation(300)[:ng])
    M = RG.hw_genotypes(O, ng, 400, seed=ng)
    big = np.full((ng + 5, ng + 5), np.nan)
    big[:ng, :ng] = A22
    assert np.isnan(big[ng:]).all() and np.isnan(big[:, ng:]).all() and big.strides == (8 * (ng + 5), 8) and np.array_equal(big[:ng, :ng], A22)
    D = []
    for corner in (False, True):
        s = ngp.Sampler(device=0)
        s.grm_begin(ng, 1); s.grm_columns(M); s.grm_end()
        if corner:
            s._chk(s.L.ngp_grm_single_step(s.h, big.ctypes.data_as(C.POINTER(C.c_double)), C.c_int64(ng + 5), C.c_double(w)))
        else:
            s.grm_single_step(A22, w)
        D.append(s.grm_get())
        s.close()
    assert np.all(np.isfinite(D[0])) and np.array_equal(D[0], D[1])


# ---- the helpers themselves (no device needed) -------------------------------------------------------------------------------------
def test_layout_helpers_on_the_host(ngp):
    """padded / short_buffer and their non-vacuity checks on the shapes of sections A and D, every type, counts and dosages; the
    wrapper's _columns hands a padded view's column ranges over with the parent's leading dimension; a contiguous copy, a padding that
    is finite or a buffer one element too long are caught."""
    for kind in ("f64", "f32", "u8"):
        for n, P in ((AN, AP), (ANC, AP), (BN, BP)):
            V = _typed(_counts(n, P, 1) if kind == "u8" else _dosages(n, P, 1), kind)
            view = padded(V)
            assert assert_poisoned(view) == n + PAD == leading_dimension(view) and np.array_equal(view, V)
            for a, b in ((0, P), (0, 64), (64, P), (128, P)):
                A, t, sfx, ld = ngp._lib._columns(view[:, a:b])
                assert A.ctypes.data == view[:, a:b].ctypes.data and (t, sfx, ld) == (CT[kind], kind, n + PAD)
            flat = short_buffer(V, n + PAD)
            assert_short(flat, V, n + PAD)
            with pytest.raises(AssertionError):
                assert_poisoned(np.asfortranarray(view))                     # a contiguous copy: no parent, no padding
            with pytest.raises(AssertionError):
                assert_short(np.append(flat, flat[-1:]), V, n + PAD)         # the last column as long as ld allows
            tame = padded(V); tame.base[n:] = 0
            with pytest.raises(AssertionError):
                assert_poisoned(tame)
    D = _dosages(65, 33, 3)
    assert D.dtype == np.float32 and D.min() >= 0.0 and D.max() <= 2.0 and np.array_equal(_typed(D, "f64"), D.astype(np.float64))
