"""Sparse fixed-effect sets, the parts that need no device: the builders of tests/ref_fixed_sparse.py against dense numpy, the Gauss-Seidel
depths, design_codes against design_columns, the CSC helpers of the host mirror, runLMEM's routing by width (a stand-in Sampler) and the
binding: ABI symbol, header text, Julia shim."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ref_fixed_sparse as RF
from ref_random_tuple import fma
from test_julia_shim_static import c_declarations, julia_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _random_design(rng, N, ncol, density, dyadic):
    X = np.zeros((N, ncol))
    mask = rng.random((N, ncol)) < density
    mask[rng.integers(0, N, size=ncol), np.arange(ncol)] = True       # every column has an entry
    vals = rng.integers(-16, 17, size=(N, ncol)) / 8.0 if dyadic else rng.normal(size=(N, ncol))
    X[mask] = vals[mask]
    return X


def _dense_xpx_fma(X):
    """The dense set's x0: every entry the fma chain over ALL records from 0.0 (ngp_add_fixed_set)."""
    N, nc = X.shape
    out = np.zeros((nc, nc))
    for a in range(nc):
        for b in range(a + 1):
            acc = 0.0
            for i in range(N):
                acc = fma(float(X[i, a]), float(X[i, b]), acc)
            out[a, b] = out[b, a] = acc
    return out


@pytest.mark.parametrize("dyadic", [True, False], ids=["dyadic", "general"])
def test_builders_against_dense_numpy(ngp, dyadic):
    rng = np.random.default_rng(5)
    for N, ncol, density in ((40, 7, 0.3), (70, 12, 0.08), (25, 5, 1.0)):
        X = _random_design(rng, N, ncol, density, dyadic)
        _, _, cp, row, val = ngp.dense_csc(X)
        assert np.array_equal(RF.dense_of_csc(N, ncol, cp, row, val), X)
        for a in range(ncol):
            assert np.all(np.diff(row[cp[a]:cp[a + 1]]) > 0) and cp[a + 1] > cp[a]
        recs = RF.csr_of_csc(N, ncol, cp, row, val)
        for i in range(N):
            assert [c for c, _ in recs[i]] == np.nonzero(X[i])[0].tolist() and [v for _, v in recs[i]] == X[i][X[i] != 0].tolist()
        rows = RF.xpx_rows(N, ncol, cp, row, val)
        G = np.zeros((ncol, ncol))
        for a, r in enumerate(rows):
            assert [c for c, _ in r] == sorted(c for c, _ in r) and len({c for c, _ in r}) == len(r)
            for c, v in r:
                G[a, c] = v
        want = X.T @ X if dyadic else _dense_xpx_fma(X)             # (dyadic values: every product and sum is exact, any order gives these bits)
        assert np.array_equal(G, want)
        stored = {(a, c) for a, r in enumerate(rows) for c, _ in r}
        assert stored == {(a, c) for a in range(ncol) for c in range(ncol) if np.any((X[:, a] != 0) & (X[:, c] != 0))}
        diagR = RF.ridge_diag(rows)
        assert diagR == [want[a, a] + np.abs(np.diag(want)).min() / 10000.0 for a in range(ncol)]


def test_depths_of_factors(ngp):
    rng = np.random.default_rng(2)
    N = 300
    herd = rng.integers(-1, 20, size=N); herd[:21] = np.arange(-1, 20)
    pen = rng.integers(-1, 4, size=N); pen[:5] = np.arange(-1, 4)
    one = ngp.factors_csc([herd])
    dep = RF.depths(RF.xpx_rows(*one))
    assert one[1] == 20 and dep == [0] * 20                          # one factor: X'X is diagonal
    two = ngp.factors_csc([herd, pen])
    rows = RF.xpx_rows(*two)
    dep = RF.depths(rows)
    assert two[1] == 24 and len(set(dep)) <= 2 and dep[:20] == [0] * 20
    full = ngp.factors_csc([herd, pen], rng.normal(size=(N, 2)))     # two covariates behind them: each reads everything in front of it
    dep = RF.depths(RF.xpx_rows(*full))
    assert full[1] == 26 and dep[24] == max(dep[:24]) + 1 and dep[25] == dep[24] + 1 and max(dep) >= 3
    X = RF.dense_of_csc(*full)
    assert np.array_equal(X[:, :20], (herd[:, None] == np.arange(20)[None, :]).astype(float)) and np.array_equal(X[:, 20:24], (pen[:, None] == np.arange(4)).astype(float))
    with pytest.raises(ValueError, match="no record"):
        ngp.factors_csc([np.array([0, 2, 2, -1])])


def test_step_needs_no_zeros(O, ngp):
    """The restatement on the stored entries equals the restatement with every zero of a column stored as well: a zero is a no-op."""
    rng = np.random.default_rng(8)
    N, ncol = 1100, 6
    X = _random_design(rng, N, ncol, 0.2, False)
    sp = ngp.dense_csc(X)
    cpf = np.arange(ncol + 1) * N
    rowf, valf = np.tile(np.arange(N), ncol), X.T.ravel()
    y, b0 = rng.normal(size=N), rng.normal(size=ncol)
    a = RF.sparse_step(O, 3, 1, 2, 0, *sp, y, b0, 1.7)
    full_rows = RF.xpx_rows(N, ncol, cpf, rowf, valf)
    sparse_rows = RF.xpx_rows(*sp)
    for ra, rb in zip(full_rows, sparse_rows):
        keep = {c for c, _ in rb}
        assert [(c, v) for c, v in ra if c in keep] == rb and all(v == 0.0 for c, v in ra if c not in keep)
    b = RF.sparse_step(O, 3, 1, 2, 0, N, ncol, cpf, rowf, valf, y, b0, 1.7)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.abs(a[0] - b0).max() > 0


def test_design_codes_against_design_columns(ngp):
    from nextgp_jl_amd import api
    rng = np.random.default_rng(1)
    for col in (np.array([f"h{k:03d}" for k in rng.integers(0, 30, size=200)]), rng.integers(5, 17, size=200), np.array(["b", "a", "c", "a"])):
        X, names = api.design_columns("herd", col)
        codes, names2 = api.design_codes("herd", col)
        assert names2 == names and codes.min() == -1 and codes.max() == X.shape[1] - 1
        assert np.array_equal(RF.dense_of_csc(*ngp.factors_csc([codes])), X)
    with pytest.raises(ValueError, match="single level"):
        api.design_codes("herd", np.array(["a", "a"]))
    with pytest.raises(ValueError, match="covariate"):
        api.design_codes("w", np.array([0.5, 1.5]))


class _StandIn:
    """What runLMEM calls on a Sampler, recorded; no library, no device."""
    made = []

    def __init__(self, **kw):
        self.calls, self.randoms, self.N, self.nfixcol = [], [], 0, 0
        _StandIn.made.append(self)

    def set_records(self, N):
        self.N = N

    def add_fixed_set(self, X, lhs0=None, rhs0=None):
        X = np.asarray(X, dtype=np.float64)
        X = X[:, None] if X.ndim == 1 else X
        self.calls.append(("dense", X))
        self.nfixcol += X.shape[1]

    def add_fixed_set_sparse(self, N, ncol, col_ptr, row, val):
        self.calls.append(("sparse", RF.dense_of_csc(N, ncol, col_ptr, row, val)))
        self.nfixcol += ncol

    def add_random_set(self, level, q, K=None, df=4.0, scale=None, varU0=100.0):
        self.q = q
        return 0

    def get_fixed(self):
        return dict(b=np.arange(self.nfixcol, dtype=np.float64), sum_b=np.arange(self.nfixcol, dtype=np.float64))

    def get_random(self, set_id):
        return dict(u=np.zeros(self.q), sum_u=np.zeros(self.q), varU=1.0, sum_varU=1.0)

    def get_state(self):
        return dict(b=1.0, varE=2.0, beta=np.zeros(0), delta=np.zeros(0), varBeta=np.zeros(0), piHat=np.zeros(0))

    def get_posterior_sums(self):
        return dict(nKept=1, sum_b=1.0, sum_varE=2.0, sum_beta=np.zeros(0), sum_delta=np.zeros(0), sum_varBeta=np.zeros(0), sum_pi=np.zeros(0))

    def __getattr__(self, name):
        return lambda *a, **kw: None


def test_runLMEM_routes_fixed_units_by_width(ngp, tmp_path, monkeypatch):
    from nextgp_jl_amd import api
    monkeypatch.setattr(api, "Sampler", _StandIn)
    rng = np.random.default_rng(4)
    N = 400
    herd = np.array([f"h{k:03d}" for k in np.concatenate([np.arange(70), rng.integers(0, 70, size=N - 70)])])     # 69 columns
    pen = np.concatenate([np.arange(5), rng.integers(0, 5, size=N - 5)])                                           # 4 columns
    ids = [f"a{k}" for k in range(1, 31)]                             # (a model without SNP terms needs a PED term: founders only)
    data = dict(y=rng.normal(size=N), herd=herd, pen=pen, w=rng.normal(size=N), ID=np.array(ids)[rng.integers(0, 30, size=N)])
    Xh, nh = api.design_columns("herd", herd)
    Xp, npn = api.design_columns("pen", pen)
    Xw, nw = api.design_columns("w", data["w"])
    n = [0]

    def run(**kw):
        _StandIn.made.clear()
        n[0] += 1
        res = api.runLMEM("y ~ 1 + herd + pen + w + PED(ID)", data, 2, 0, 1, outFolder=str(tmp_path / f"o{n[0]}"), VCV={"ID": api.Random("A", 1.0)},
                          userPedData=[(a, "0", "0") for a in ids], samples="none", **kw)
        return _StandIn.made[0].calls, res

    calls, res = run()                                               # "auto": only the unit wider than 64 columns
    assert [k for k, _ in calls] == ["sparse", "dense", "dense"]
    assert np.array_equal(calls[0][1], Xh) and np.array_equal(calls[1][1], Xp) and np.array_equal(calls[2][1], Xw)
    assert res["fixed_names"] == ["(Intercept)"] + nh + npn + nw and nh[0] == "herd: h001"
    calls, _ = run(sparseFixed=True)                                 # every unit of several columns; a single column stays dense
    assert [k for k, _ in calls] == ["sparse", "sparse", "dense"] and np.array_equal(calls[1][1], Xp)
    calls, _ = run(sparseFixed=False)
    assert [k for k, _ in calls] == ["dense", "dense", "dense"] and np.array_equal(calls[0][1], Xh)
    calls, res = run(blockThese=[["pen", "w"]])                      # a block of 5 columns: dense by default, blocks first
    assert [k for k, _ in calls] == ["dense", "sparse"] and np.array_equal(calls[0][1], np.column_stack([Xp, Xw]))
    assert res["fixed_names"] == ["(Intercept)"] + npn + nw + nh
    calls, _ = run(blockThese=[["pen", "w"]], sparseFixed=True)      # the block's covariate as a full column behind the factor's
    assert [k for k, _ in calls] == ["sparse", "sparse"] and np.array_equal(calls[0][1], np.column_stack([Xp, Xw]))
    calls, res = run(blockThese=[["herd", "pen", "w"]])              # 74 columns in one block
    assert [k for k, _ in calls] == ["sparse"] and np.array_equal(calls[0][1], np.column_stack([Xh, Xp, Xw]))
    with pytest.raises(ValueError, match="sparseFixed"):
        run(sparseFixed="yes")


def test_abi_symbol_header_and_julia_binding(ngp):
    assert "ngp_add_fixed_set_sparse" in ngp.SYMBOLS
    lib = ngp.load()
    lib.ngp_add_fixed_set_sparse.restype = C.c_int32
    assert lib.ngp_add_fixed_set_sparse(None, C.c_int64(4), C.c_int64(2), None, None, None, None) == -1      # a null handle: an argument error, not a crash
    decl = c_declarations()
    assert decl["ngp_add_fixed_set_sparse"] == ["ngp_handle*", "int64_t", "int64_t", "int64_t*", "int32_t*", "double*", "int32_t*"]
    hdr = open(os.path.join(ROOT, "include", "nextgp_hip.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int32_t ngp_add_fixed_set_sparse", hdr, flags=re.S)
    text = " ".join(m.group(1).replace("*", " ").split())
    for phrase in ("CSC", "strictly ascending", "2 <= ncol <= 2^20", "(set + 1) << 20 | column", "fewer than 2^31 entries", "bit for bit the dense set",
                   "Sparse fixed-effect sets"):
        assert phrase in text, phrase
    calls = [c for c in julia_ccalls() if c[0] == "ngp_add_fixed_set_sparse"]
    assert len(calls) == 1 and calls[0][2] == ["Ptr{Cvoid}", "Int64", "Int64", "Ptr{Int64}", "Ptr{Int32}", "Ptr{Float64}", "Ref{Int32}"]
    jl = open(os.path.join(ROOT, "nextgp.jl_amd", "julia", "NextGPHIP.jl")).read()
    assert "function add_fixed_set_sparse!(h::Handle, X::SparseMatrixCSC)" in jl and "using SparseArrays" in jl
    assert re.search(r"if X\[x\]\.nCol > 64[^\n]*\n\s*add_fixed_set_sparse!\(h, SparseArrays\.sparse\(", jl)
    assert "Xs.colptr .- 1" in jl and "Xs.rowval .- 1" in jl            # 0-based offsets and rows at the ABI
    src = open(os.path.join(ROOT, "nextgp.jl_amd", "csrc", "ngp_fixed_sparse.h")).read()
    for k in ("k_fixs_yi", "k_fixs_gs_wide", "k_fixs_gs_fused", "k_fixs_update"):
        body = src[src.index(f"void {k}("):]
        assert "if (abort_w && *abort_w != 0u) return;" in body[:body.index("\n}")], k
    assert "#pragma clang fp contract(off)" in src and "__builtin_fma" in src
