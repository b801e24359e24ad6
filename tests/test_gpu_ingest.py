"""Every staged loader across chunk boundaries and padded columns (include/nextgp_hip.h: ngp_set_panel_*, ngp_panel_columns_*,
ngp_load_panel_file, ngp_grm_columns_*, ngp_prediction_columns_*, ngp_load_prediction_file).

Each of these stages the caller's matrix through a fixed-size device buffer, 256 MiB or 64 MiB at a time; a test-sized matrix fits one
chunk, so the chunk arithmetic (host offset, mean slice, column origin, block origin, the GRM's running column count) never moved.
ngp_debug_set_staging_bytes shrinks the chunk, and the stored panel is then read back COLUMN BY COLUMN and compared with a reference
written here in plain fp64 numpy (not the oracle's panel code):

    mean          mu_j = sequential sum over the rows / N (np.cumsum(col)[-1] / N); genotype codes: integer column sum / N
    fp32 tiles    x_ij = float32(float64(v_ij) - mu_j); under residual weights float32(s_i (float64(v_ij) - mu_j)), s_i = sqrt(w_i)
    byte tiles    the code itself

The read-back is ngp_xbeta(e_j).  It is exact for a unit vector on both storages (k_xbeta: acc = fma(x_ij, beta_j, acc) from 0.0 with
beta = e_j is x_ij itself, divided by s_i under weights; k_xbeta8: fma(g_ij, 1, 0) - fma(mu_j, 1, 0) = g_ij - mu_j in one fp64
rounding), so the comparison is np.array_equal."""
import ctypes as C
import functools
import time

import numpy as np
import pytest

import ref_gblup as RG
import ref_predict as RP
from conftest import add_sets

gpu = pytest.mark.gpu                        # every test but the wrapper's stride check needs the device

EPS = 2.0 ** -53
N, P = 333, 330                              # five full 64-column blocks and a partial one; N % 4 = 1 (two-bit columns end mid-byte)
CALLS = ((130, 330), (0, 57), (57, 130))     # boundaries inside blocks, out of order
PAD = 43
NP_ = 70                                     # prediction individuals
SPEC = [(0, 100, "PR"), (100, 230, "R")]     # one BayesPR and one BayesR set, split at column 100
SETS = [(0, 100), (100, 230)]
SCHED = (6, 2, 2)                            # kept: 4, 6
V0 = 0.01
CT = {"f64": C.c_double, "f32": C.c_float, "u8": C.c_uint8}
# what goes in, the storage it goes into, residual weights or not
KINDS = {"f64": ("f64", None, False), "f32": ("f32", None, False), "u8": ("u8", None, False), "u8c": ("u8", "u8", False),
         "f64w": ("f64", None, True)}


@functools.lru_cache(None)
def data():
    """The matrices every test shares (read-only): codes 0/1/2, the same with noise in Float64 (so that the order of the mean's sum
    matters) and rounded to Float32, residual weights, a phenotype, prediction codes."""
    rng = np.random.default_rng(20251)
    G8 = np.asfortranarray(rng.integers(0, 3, size=(N, P)).astype(np.uint8))
    V64 = np.asfortranarray(G8.astype(np.float64) + 0.01 * rng.normal(size=(N, P)))
    V32 = np.asfortranarray(V64.astype(np.float32))
    w = rng.uniform(0.25, 4.0, size=N)
    bt = np.zeros(P); bt[rng.choice(P, 8, replace=False)] = rng.normal(size=8)
    y = 10.0 + (G8 - G8.mean(axis=0)) @ bt + rng.normal(size=N)
    Gp = np.asfortranarray(rng.integers(0, 3, size=(NP_, P)).astype(np.uint8))
    d = dict(u8=G8, f64=V64, f32=V32, w=w, y=y, Gp=Gp)
    for a in d.values():
        a.setflags(write=False)
    return d


# ---- the reference ---------------------------------------------------------------------------------------------------------------
def ref_means(V):
    if V.dtype == np.uint8:
        return V.sum(axis=0, dtype=np.int64) / V.shape[0]
    return np.cumsum(V.astype(np.float64), axis=0)[-1] / V.shape[0]


def ref_columns(V, storage=None, w=None):
    """(mu, X): the column means and what ngp_xbeta(e_j) must return for every column j, as Float64."""
    mu = ref_means(V)
    D = V.astype(np.float64) - mu[None, :]
    if storage == "u8":
        return mu, D
    if w is None:
        return mu, D.astype(np.float32).astype(np.float64)
    s = np.sqrt(w)[:, None]
    return mu, (s * D).astype(np.float32).astype(np.float64) / s


@functools.lru_cache(None)
def ref_kind(kind):
    key, storage, weighted = KINDS[kind]
    return ref_columns(data()[key], storage, data()["w"] if weighted else None)


# ---- reading a handle back -------------------------------------------------------------------------------------------------------
def stored_columns(s):
    out = np.empty((s.N, s.P))
    e = np.zeros(s.P)
    for j in range(s.P):
        e[j] = 1.0
        out[:, j] = s.xbeta(e)
        e[j] = 0.0
    return out


def summary(s):
    return dict(means=s.means(), mpm=s.mpm(), gram=np.array([s.gram(t) for t in range((s.P + 63) // 64)]), layout=s.layout())


def assert_same_summary(a, b):
    assert a["layout"] == b["layout"]
    for k in ("means", "mpm", "gram"):
        assert np.array_equal(a[k], b[k]), k


def padded(V, fill_rows=PAD):
    """V on top of `fill_rows` rows that must never be read as genotypes: NaN and inf (255 for codes)."""
    big = np.empty((V.shape[0] + fill_rows, V.shape[1]), dtype=V.dtype, order="F")
    big[:V.shape[0]] = V
    if V.dtype == np.uint8:
        big[V.shape[0]:] = 255
    else:
        big[V.shape[0]::2] = np.nan
        big[V.shape[0] + 1::2] = np.inf
    view = big[:V.shape[0]]
    assert view.strides == (V.itemsize, (V.shape[0] + fill_rows) * V.itemsize) and not view.flags.f_contiguous
    return view


def short_buffer(V, ld):
    """The C contract's short form: ncol - 1 columns of ld elements and a last one of N, not an element more; NaN (255) between."""
    n, ncol = V.shape
    flat = np.full((ncol - 1) * ld + n, 255 if V.dtype == np.uint8 else np.nan, dtype=V.dtype)
    for j in range(ncol):
        flat[j * ld:j * ld + n] = V[:, j]
    return flat


def new_sampler(ngp, storage=None, weights=None, seed=1):
    s = ngp.Sampler(device=0, seed=seed, chain=0, storage=storage)
    if weights is not None:
        s.set_residual_weights(weights)
    return s


def load_ranges(ngp, V, storage=None, weights=None, cols_per_chunk=0, short_ld=0):
    """The panel in the three calls of CALLS, every call staged `cols_per_chunk` columns at a time (0: the default size).  V may be a
    padded view (the wrapper passes its leading dimension); short_ld > 0 hands over short buffers by direct C calls instead."""
    s = new_sampler(ngp, storage, weights)
    ld = short_ld if short_ld else V.strides[1] // V.itemsize
    s.debug_set_staging_bytes(cols_per_chunk * ld * V.itemsize)
    s.begin_panel(*V.shape)
    sfx = {1: "u8", 4: "f32", 8: "f64"}[V.itemsize]
    for a, b in CALLS:
        if short_ld:
            flat = short_buffer(V[:, a:b], ld)
            s._chk(getattr(s.L, "ngp_panel_columns_" + sfx)(s.h, C.c_int64(a), flat.ctypes.data_as(C.POINTER(CT[sfx])), C.c_int64(b - a),
                                                          C.c_int64(ld), C.c_int32(1)))
        else:
            s.panel_columns(a, V[:, a:b], centre=True)
    s.end_panel()
    return s


_DEFAULT = {}


def default_summary(ngp, kind):
    """The same three calls at the default staging size (one chunk each), once per kind."""
    if kind not in _DEFAULT:
        key, storage, weighted = KINDS[kind]
        _DEFAULT[kind] = summary(load_ranges(ngp, data()[key], storage, data()["w"] if weighted else None))
    return _DEFAULT[kind]


def assert_panel(ngp, s, kind):
    """Every column and the means against the reference; means, x'x, every Gram block and the layout against the default-size upload."""
    mu, X = ref_kind(kind)
    assert np.array_equal(s.means(), mu)
    got = stored_columns(s)
    wrong = np.flatnonzero((got != X).any(axis=0))
    assert wrong.size == 0, f"columns that differ from the reference: {wrong[:20]}"
    assert_same_summary(summary(s), default_summary(ngp, kind))


# ---- the wrapper's leading dimension (no device needed) ------------------------------------------------------------------------------
def test_wrapper_hands_over_a_taller_parent_without_a_copy(ngp):
    """Sampler.set_panel / panel_columns / prediction_columns take what _columns returns: big[:N] and its column ranges as they are with
    the parent's leading dimension, contiguous Fortran arrays as they are with ld = N, everything else as a Fortran copy."""
    cols = ngp._lib._columns
    for dt, t, sfx in ((np.float64, C.c_double, "f64"), (np.float32, C.c_float, "f32"), (np.uint8, C.c_uint8, "u8")):
        V = np.asfortranarray(np.arange(12 * 7).reshape(12, 7).astype(dt))
        view = padded(V)
        for M, ld in ((view, 12 + PAD), (view[:, 2:5], 12 + PAD), (view[:, 6:], 12 + PAD), (view[:, ::2], 2 * (12 + PAD)), (V, 12), (V[:, 1:4], 12)):
            A, tt, ss, l = cols(M)
            assert np.shares_memory(A, M) and A.ctypes.data == M.ctypes.data and (tt, ss, l) == (t, sfx, ld) and np.array_equal(A, M)
        for M in (np.ascontiguousarray(V), V[::2], V[3:9:2, 1:3], view[::-1]):      # row-major, strided rows, reversed rows
            A, tt, ss, l = cols(M)
            assert A.flags.f_contiguous and l == M.shape[0] and (tt, ss) == (t, sfx) and np.array_equal(A, M)
    A, tt, ss, l = cols(np.arange(6).reshape(3, 2))                                # any other type goes as Float64
    assert A.dtype == np.float64 and A.flags.f_contiguous and (tt, ss, l) == (C.c_double, "f64", 3)


# ---- a. training columns across chunk boundaries -----------------------------------------------------------------------------------
# 0: the default size; 1: one column per chunk; 37 divides neither 64 nor any call's width (200, 57, 73), so every call ends on a short
# chunk; 8 leaves a last chunk of exactly one column in two calls (57 = 7 x 8 + 1, 73 = 9 x 8 + 1) and divides the third (200)
@gpu
@pytest.mark.parametrize("chunk", [0, 1, 37, 8])
@pytest.mark.parametrize("kind", list(KINDS))
def test_training_columns_across_chunks(ngp, kind, chunk):
    key, storage, weighted = KINDS[kind]
    s = load_ranges(ngp, data()[key], storage, data()["w"] if weighted else None, cols_per_chunk=chunk)
    assert_panel(ngp, s, kind)
    if not weighted:                         # x'x in fp64 numpy on the reference tiles, at the relative 1e-12 of test_gram_and_mpm
        X = ref_kind(kind)[1]
        assert np.allclose(s.mpm(), (X * X).sum(axis=0), rtol=1e-12, atol=0)


# ---- b. padded columns -----------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("chunk", [0, 37])
@pytest.mark.parametrize("kind", ["f64", "f32", "u8", "u8c"])
def test_padded_columns(ngp, kind, chunk):
    """ld = N + 43, the rows below N hold NaN and inf (255 for codes): the upload succeeds (k_cols_mean must not flag the padding) and
    the tiles are those of the contiguous matrix.  The view big[:N] is ALLOCATED TO FULL ld in its last column too (numpy owns
    (N + 43) x P elements); the form the C contract also allows, a last column of only N elements, is the next test."""
    key, storage, _ = KINDS[kind]
    view = padded(data()[key])
    assert_panel(ngp, load_ranges(ngp, view, storage, cols_per_chunk=chunk), kind)
    # the whole panel in one call: ngp_set_panel_f64 / _f32 (the column loop), ngp_set_panel_u8 (the block ingest) with the same ld
    s = new_sampler(ngp, storage)
    s.debug_set_staging_bytes(chunk * (N + PAD) * view.itemsize)
    s.set_panel(view, centre=True)
    assert_panel(ngp, s, kind)


@gpu
@pytest.mark.parametrize("chunk", [0, 37])
@pytest.mark.parametrize("kind", ["f64", "f32", "u8", "u8c"])
def test_short_last_column(ngp, kind, chunk):
    """Buffers of exactly (ncol - 1) ld + N elements, by direct C calls: what the copy length (nc - 1) ld + N of every chunk is for.
    (A copy that took ld for the last column would read 43 elements past the buffer: host memory the results do not depend on --
    only a host memory checker sees that, no assertion here can.)"""
    key, storage, _ = KINDS[kind]
    V = data()[key]
    assert_panel(ngp, load_ranges(ngp, V, storage, cols_per_chunk=chunk, short_ld=N + PAD), kind)
    if key == "u8":                          # ngp_set_panel_u8 takes the same short form
        s = new_sampler(ngp, storage)
        s.debug_set_staging_bytes(chunk * (N + PAD))
        flat = short_buffer(V, N + PAD)
        s._chk(s.L.ngp_set_panel_u8(s.h, flat.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_int64(N), C.c_int64(P), C.c_int64(N + PAD), C.c_int32(1)))
        s.N, s.P = N, P
        assert_panel(ngp, s, kind)


# ---- c. the block ingest: ngp_set_panel_u8 and ngp_load_panel_file -----------------------------------------------------------------
# blocks per chunk.  P = 330 is six blocks: 1 -> six chunks; 2 -> three chunks, the partial block the second of the last one;
# 5 -> two chunks, the partial block alone in the last one
@gpu
@pytest.mark.parametrize("blocks", [1, 2, 5])
@pytest.mark.parametrize("storage", [None, "u8"])
def test_block_ingest_across_chunks(ngp, tmp_path, storage, blocks):
    kind = "u8c" if storage else "u8"
    G = data()["u8"]
    staging = blocks * 64 * N
    got = {}
    s = new_sampler(ngp, storage)
    s.debug_set_staging_bytes(staging)
    s.set_panel(G, centre=True)
    assert_panel(ngp, s, kind)
    got["set_panel_u8"] = summary(s)
    for bits in (8, 2):
        path = tmp_path / f"p{bits}.ngp"
        ngp.write_panel_file(path, G, bits=bits)
        s = new_sampler(ngp, storage)
        s.debug_set_staging_bytes(staging)
        s.load_panel_file(path, centre=True)
        assert_panel(ngp, s, kind)
        got[f"file{bits}"] = summary(s)
    for k, v in got.items():                 # ... and all of them the panel of ngp_panel_columns_u8 in ranges (assert_panel), layout included
        assert_same_summary(v, got["set_panel_u8"])


# ---- chains ----------------------------------------------------------------------------------------------------------------------
def short_chain(s, spec=SPEC, niter=6):
    y = data()["y"]
    add_sets(s, spec, V0)
    s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var()); s.set_schedule(*SCHED)
    s.run(niter)
    return s.get_state()


def assert_same_state(a, b):
    for k in ("beta", "ycorr", "delta"):
        assert np.array_equal(a[k], b[k]), k
    assert a["varE"] == b["varE"]


# ---- g. the chain does not care --------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", ["f64", "u8c"])
def test_chain_after_a_chunked_upload(ngp, O, kind):
    """One BayesPR and one BayesR set over a panel of (a) loaded 37 columns at a time: after 6 iterations the state is that of the
    default-size handle and of the blocked oracle on the same matrix, bit for bit.  Float64 into fp32 tiles: the oracle is given the
    reference tiles (the chain never reads the stored means there); codes into byte tiles: the oracle centres them itself, and the
    chain does read the means."""
    key, storage, _ = KINDS[kind]
    V = data()[key]
    states = []
    for chunk in (37, 0):
        s = load_ranges(ngp, V, storage, cols_per_chunk=chunk)
        states.append(short_chain(s))
    R, S, _ = s.layout()
    o = O.Oracle(order=1, seed=1, chain=0)
    if storage:
        o.set_panel_u8(V, R=R, S=S, D=s.config()[1], near=s.near(), tform=s.chain_form())
    else:
        o.set_panel_f32(ref_kind(kind)[1].astype(np.float32), R=R, S=S, D=s.config()[1], near=s.near(), nchain=s.streamer()[1], tform=s.chain_form())
    states.append(short_chain(o))
    assert np.abs(states[0]["beta"]).max() > 0
    assert_same_state(states[0], states[1])
    assert_same_state(states[0], states[2])


# ---- d. refusals after the first chunk -------------------------------------------------------------------------------------------
@gpu
def test_training_refusals_in_a_later_chunk(ngp, tmp_path):
    """A non-finite value in the third chunk of ngp_set_panel_f64, a panel file truncated inside its second chunk and a two-bit file
    with code 3 there: NGP_ERR_ARG with the documented message, after the tiles of the earlier chunks were written; the handle then
    takes a good panel and runs the chain of a fresh handle."""
    d = data()
    fresh = new_sampler(ngp); fresh.set_panel(d["f64"], centre=True)
    want = short_chain(fresh)
    bad = d["f64"].copy(order="F"); bad[200, 100] = np.inf      # column 100: chunk [74, 111) of 37
    s = new_sampler(ngp)
    s.debug_set_staging_bytes(37 * N * 8)
    with pytest.raises(ngp.NextGPHipError, match="error -1: non-finite"):
        s.set_panel(bad, centre=True)
    s.set_panel(d["f64"], centre=True)
    assert_same_state(short_chain(s), want)

    good8, good2, trunc, code3 = (tmp_path / n for n in ("good8.ngp", "good2.ngp", "trunc.ngp", "code3.ngp"))
    ngp.write_panel_file(good8, d["u8"], bits=8)
    ngp.write_panel_file(good2, d["u8"], bits=2)
    trunc.write_bytes(good8.read_bytes()[:32 + 100 * N + 17])              # column 100 is in block 1: the second chunk of one block
    raw = bytearray(good2.read_bytes())
    raw[32 + 100 * ((N + 3) // 4) + 5 // 4] |= 3 << (2 * (5 % 4))          # row 5 of column 100 becomes code 3
    code3.write_bytes(bytes(raw))
    for storage in (None, "u8"):
        fresh = new_sampler(ngp, storage); fresh.set_panel(d["u8"], centre=True)
        want = short_chain(fresh)
        for path, msg in ((trunc, "error -1: panel file truncated"), (code3, r"error -1: .*code 3")):
            s = new_sampler(ngp, storage)
            s.debug_set_staging_bytes(64 * N)
            with pytest.raises(ngp.NextGPHipError, match=msg):
                s.load_panel_file(path, centre=True)
            with pytest.raises(ngp.NextGPHipError, match="error -2"):      # the failed set-up left no panel behind
                s.layout()
            s.load_panel_file(good2, centre=True)
            assert_same_state(short_chain(s), want)


@gpu
def test_prediction_refusals_in_a_later_chunk(ngp, tmp_path):
    """The same for the prediction panel: ngp_prediction_columns_f64 with an inf in its third chunk, a prediction file truncated in
    and one with code 3 in its second chunk.  The training chain then runs unchanged; a good prediction panel uploaded behind the
    refused columns predicts what a fresh handle predicts."""
    d = data()
    Gp = d["Gp"]
    fresh = new_sampler(ngp); fresh.set_panel(d["u8"], centre=True); fresh.set_prediction_panel(Gp, centre=True)
    want = short_chain(fresh)
    want_pred = fresh.prediction_sums()
    bad = Gp.astype(np.float64, order="F"); bad[3, 100] = np.inf
    s = new_sampler(ngp); s.set_panel(d["u8"], centre=True)
    s.begin_prediction_panel(NP_)
    s.debug_set_staging_bytes(37 * NP_ * 8)
    with pytest.raises(ngp.NextGPHipError, match="error -1: non-finite"):
        s.prediction_columns(0, bad, centre=True)
    s.prediction_columns(0, Gp, centre=True)
    s.end_prediction_panel()
    assert_same_state(short_chain(s), want)
    got = s.prediction_sums()
    assert got["nKept"] == want_pred["nKept"] == 2 and np.array_equal(got["sum"], want_pred["sum"]) and np.array_equal(got["sum2"], want_pred["sum2"])

    good2, trunc, code3 = (tmp_path / n for n in ("good2.ngp", "trunc.ngp", "code3.ngp"))
    ngp.write_panel_file(trunc, Gp, bits=8)
    trunc.write_bytes(trunc.read_bytes()[:32 + 100 * NP_ + 17])            # 64 columns per chunk: column 100 is in the second
    ngp.write_panel_file(good2, Gp, bits=2)
    raw = bytearray(good2.read_bytes())
    raw[32 + 100 * ((NP_ + 3) // 4) + 5 // 4] |= 3 << (2 * (5 % 4))
    code3.write_bytes(bytes(raw))
    for path, msg in ((trunc, "error -1: panel file truncated"), (code3, r"error -1: .*code 3")):
        s = new_sampler(ngp); s.set_panel(d["u8"], centre=True)
        s.debug_set_staging_bytes(64 * NP_)
        with pytest.raises(ngp.NextGPHipError, match=msg):
            s.load_prediction_file(path, centre=True)
        assert_same_state(short_chain(s), want)                            # no prediction panel, the training chain as it was
        assert s.prediction_stats() == (0, 0)
        s.load_prediction_file(good2, centre=True)                         # ... and the handle takes a good one
        s.set_y(d["y"]); s.run(6)
        got = s.prediction_sums()
        assert np.array_equal(got["sum"], want_pred["sum"]) and np.array_equal(got["sum2"], want_pred["sum2"])


# ---- e. the relationship matrix --------------------------------------------------------------------------------------------------
GN, GP = 257, 1000


@functools.lru_cache(None)
def grm_data(O):
    M8 = RG.hw_genotypes(O, GN, GP, seed=21)
    M8.setflags(write=False)
    return M8


def grm_build(s, calls, method, cols_per_chunk=0):
    """calls: the matrices of one ngp_grm_columns_* call each.  A chunk of c columns is c x max(ld, Npad) Float64 (Npad = 320)."""
    s.grm_begin(GN, method)
    s.debug_set_staging_bytes(cols_per_chunk * 320 * 8)
    for M in calls:
        s.grm_columns(M)
    s.grm_end()
    return s.grm_get()


@gpu
@pytest.mark.parametrize("method", [1, 2])
def test_grm_across_chunks(ngp, O, method):
    """Chunks of 64 and of 128 columns (sixteen and eight of them, the last one short) against the one-chunk build, bit for bit --
    internal chunks are multiples of 64, which the contract makes split-independent -- and against ref_gblup.make_g within the bound
    of test_grm_against_restatement; a padded view at 64 columns per chunk."""
    M8 = grm_data(O)
    Gref, scale = RG.make_g(M8, method)
    bound = (2 * GP + 2 * GN + 8) * EPS * scale
    s = ngp.Sampler(device=0)
    for dt in (np.float64, np.float32, np.uint8):
        M = np.asfortranarray(M8.astype(dt))
        one = grm_build(s, [M], method)
        assert np.all(np.abs(one - Gref) <= bound), dt
        for c in (64, 128):
            G = grm_build(s, [M], method, cols_per_chunk=c)
            assert np.array_equal(G, one), (dt, c)
        big = np.asfortranarray(np.vstack([M8, np.full((PAD, GP), 7, dtype=np.uint8)]).astype(dt))
        view = big[:GN]
        assert view.strides[1] == (GN + PAD) * big.itemsize
        assert np.array_equal(grm_build(s, [view], method, cols_per_chunk=64), one), dt
    s.close()


@gpu
def test_grm_monomorphic_column_in_a_later_chunk(ngp, O):
    """Method 2 names the monomorphic column counted over all calls: 130 when it falls in the third chunk of one call (c0 = 128), and
    130 when an earlier call contributed 30 columns and it falls in the second chunk of the next (col_base = 30, c0 = 64)."""
    bad = np.array(grm_data(O)[:, :400]); bad[:, 130] = 0
    s = ngp.Sampler(device=0)
    for calls in ([bad], [bad[:, :30], bad[:, 30:]]):
        s.grm_begin(GN, 2)
        s.debug_set_staging_bytes(64 * 320 * 8)
        with pytest.raises(ngp.NextGPHipError, match=r"error -1: .*column 130 "):
            for M in calls:
                s.grm_columns(M)
    good = np.array(grm_data(O)[:, :400])
    G2 = grm_build(s, [good], 2, cols_per_chunk=64)                      # the handle builds on
    Gref, scale = RG.make_g(good, 2)
    assert np.all(np.abs(G2 - Gref) <= (2 * 400 + 2 * GN + 8) * EPS * scale)
    s.close()


# ---- f. the prediction panel -----------------------------------------------------------------------------------------------------
def kept(it):
    n, burn, thin = SCHED
    return burn + thin <= it <= n and (it - burn) % thin == 0


def predict(ngp, tmp_path, storage, how, chunk):
    """A training panel of the shared codes, the prediction panel filled `how`, `chunk` columns staged at a time (0: the default), then
    six iterations one at a time with tests/ref_predict.py restating every kept draw as test_gpu_predict.py does.  Returns the sums."""
    d = data()
    Gp = d["Gp"]
    s = new_sampler(ngp, storage, seed=41)
    s.set_panel(d["u8"], centre=True)
    if how in ("file8", "file2"):
        path = tmp_path / f"{how}.ngp"
        ngp.write_panel_file(path, Gp, bits=int(how[4:]))
        s.debug_set_staging_bytes(chunk * NP_)
        s.load_prediction_file(path, centre=True)
    else:
        s.begin_prediction_panel(NP_)
        # fp32 tiles: another input type for every range (the codes in each); byte tiles take codes only
        dts = (np.uint8,) * 3 if storage else (np.float32, np.float64, np.uint8)
        for (a, b), dt in zip(CALLS, dts):
            M = np.asfortranarray(Gp[:, a:b].astype(dt))
            ld = NP_
            if how == "padded":
                M = padded(M)
                ld = NP_ + PAD
            s.debug_set_staging_bytes(chunk * ld * M.itemsize)
            if how == "short":
                ld = NP_ + PAD
                s.debug_set_staging_bytes(chunk * ld * M.itemsize)
                flat = short_buffer(M, ld)
                sfx = {1: "u8", 4: "f32", 8: "f64"}[M.itemsize]
                s._chk(getattr(s.L, "ngp_prediction_columns_" + sfx)(s.h, C.c_int64(a), flat.ctypes.data_as(C.POINTER(CT[sfx])), C.c_int64(b - a),
                                                                   C.c_int64(ld), C.c_int32(1)))
            else:
                s.prediction_columns(a, M, centre=True)
        s.end_prediction_panel()
    y = d["y"]
    add_sets(s, SPEC, V0)
    s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var()); s.set_schedule(*SCHED)
    if storage:
        X, mean = Gp.astype(np.float64), s.means()
    else:
        X, mean = RP.stored_f32(Gp, s.means()), None
    s1 = np.zeros((len(SETS) + 1, NP_)); s2 = np.zeros_like(s1)
    nk = 0
    for it in range(1, SCHED[0] + 1):
        s.run(1)
        if kept(it):
            g = RP.predict_draw(X, s.get_state()["beta"], SETS, mean)
            RP.accumulate(s1, s2, g)
            assert np.array_equal(s.prediction_last(), g), (how, chunk, it)
            nk += 1
    ps = s.prediction_sums()
    assert nk == 2 and ps["nKept"] == 2 and np.array_equal(ps["sum"], s1) and np.array_equal(ps["sum2"], s2) and np.abs(s1[:2]).max(axis=1).min() > 0
    return s.prediction()


@gpu
@pytest.mark.parametrize("storage", [None, "u8"])
def test_prediction_panel_across_chunks(ngp, tmp_path, storage):
    """Columns staged one and 37 at a time, from contiguous ranges, from padded views (ld = Np + 43, NaN / inf / 255 below Np), from
    short buffers and from files of either width: prediction() -- mean and sd, per set and in all -- is that of the default-size
    upload bit for bit, and every one of them is the restatement of tests/ref_predict.py."""
    base = predict(ngp, tmp_path, storage, "cols", 0)
    for how, chunk in (("cols", 1), ("cols", 37), ("padded", 0), ("padded", 37), ("short", 37), ("file8", 1), ("file8", 37), ("file2", 37)):
        got = predict(ngp, tmp_path, storage, how, chunk)
        assert got["nKept"] == base["nKept"]
        for a, b in [(got, base)] + list(zip(got["sets"], base["sets"])):
            assert np.array_equal(a["mean"], b["mean"]) and np.array_equal(a["sd"], b["sd"]), (how, chunk)


# ---- h. one case per real constant, without the override ---------------------------------------------------------------------------
HN, HLD, HP = 70, 2 ** 19, 200


def _long_columns(ngp, dt, storage=None):
    rng = np.random.default_rng(8)
    G = np.asfortranarray(rng.integers(0, 3, size=(HN, HP)).astype(np.uint8))
    V = G if dt == np.uint8 else np.asfortranarray((G + 0.01 * rng.normal(size=(HN, HP))).astype(dt))
    plain = new_sampler(ngp, storage)
    t0 = time.perf_counter(); plain.set_panel(V, centre=True); t1 = time.perf_counter()
    big = np.zeros((HLD, HP), dtype=dt, order="F")
    big[:HN] = V                             # only the top N rows are ever written (the rest are untouched zero pages)
    view = big[:HN]
    s = new_sampler(ngp, storage)
    t2 = time.perf_counter(); s.set_panel(view, centre=True); t3 = time.perf_counter()
    print(f"long columns {np.dtype(dt).name}: ld = 2^19 upload {t3 - t2:.3f} s, plain {HN} x {HP} set_panel {t1 - t0:.4f} s")
    mu, X = ref_columns(V, storage)
    assert np.array_equal(s.means(), mu) and np.array_equal(stored_columns(s), X)
    assert_same_summary(summary(s), summary(plain))


@gpu
def test_u8_blocks_across_the_real_64_MiB(ngp):
    """ngp_set_panel_u8 with N = 70, ld = 2^19, P = 200: a block is 32 MiB, a chunk two blocks -- two chunks, the second with a partial
    last block (200 = 3 x 64 + 8); the host buffer is 100 MiB.  Measured on an MI355X host: this upload 0.004 s, a plain set_panel of
    the same 70 x 200 codes 0.0005 s on the commit before this test (0.0006 s on this one; the first upload of a process 0.04 s)."""
    _long_columns(ngp, np.uint8)


@gpu
def test_f32_columns_across_the_real_256_MiB(ngp):
    """ngp_panel_columns_f32 (through ngp_set_panel_f32) with N = 70, ld = 2^19, P = 200: 128 columns per chunk, two chunks, the second
    of 72; 400 MiB of host memory.  Measured on an MI355X host: this upload 0.016 s, a plain set_panel of the same 70 x 200 values
    0.0005 s on the commit before this test (0.0006 s on this one)."""
    _long_columns(ngp, np.float32)
