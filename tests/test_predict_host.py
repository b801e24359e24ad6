"""Prediction of new individuals, the parts that need no device: the restatement of the normative arithmetic (tests/ref_predict.py)
against plain Float64 products on the same stored values, runLMEM's argument checks, the gebvPredict.txt file, the symbol list and the
Julia bindings."""
import os
import re

import numpy as np
import pytest

import ref_predict as RP
from ref_random_tuple import fma
from test_julia_shim_static import C2J, c_declarations, julia_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ngp_begin_prediction_panel", "ngp_prediction_columns_f64", "ngp_prediction_columns_f32", "ngp_prediction_columns_u8",
       "ngp_end_prediction_panel", "ngp_load_prediction_file", "ngp_get_prediction_layout", "ngp_get_prediction", "ngp_set_prediction",
       "ngp_get_prediction_last", "ngp_get_prediction_stats"]


def test_fma_vec_is_the_scalar_fma():
    rng = np.random.default_rng(1)
    a = np.concatenate([rng.normal(size=3000).astype(np.float32).astype(np.float64), rng.integers(0, 3, size=1000).astype(np.float64), [0.0, 1e-200, 1e200]])
    c = rng.normal(size=a.size) * rng.choice([0.0, 1e-12, 1.0, 1e9], size=a.size)
    for b in (0.0, 0.3, -1.7e-5, 12345.678, 1e-170, float(np.nextafter(1.0, 2.0))):
        assert np.array_equal(RP.fma_vec(a, b, c), np.array([fma(float(x), b, float(y)) for x, y in zip(a, c)]))


def test_chunks_of_a_set():
    assert RP.chunks(0, 330) == [(0, 330)]
    assert RP.chunks(100, 92) == [(100, 192)]
    assert RP.chunks(0, 4400) == [(0, 2048), (2048, 4096), (4096, 4400)]
    assert RP.chunks(100, 4400) == [(100, 2112), (2112, 4160), (4160, 4500)]      # counted from the set's first block, 64 (100 // 64) = 64
    assert RP.chunks(2047, 2) == [(2047, 2049)] and RP.chunks(2048, 2048) == [(2048, 4096)]


@pytest.mark.parametrize("Np,P", [(1, 330), (63, 330), (40, 4500)])
def test_restatement_against_float64_products(Np, P):
    """fp32 storage: g on the fp32-rounded centred values against the Float64 product of the same values, inside the derived bound
    |delta_i| <= (n_cols + 2) 2^-53 sum_j |x_ij| |beta_j| per set and for all sets together.  The exact value is taken in rationals
    for three rows, and the Float64 product X @ beta (itself within the same bound of it) for all."""
    from fractions import Fraction
    rng = np.random.default_rng(P + Np)
    G = rng.integers(0, 3, size=(Np, P)).astype(np.uint8)
    mu = rng.uniform(0.1, 1.9, size=P)
    X = RP.stored_f32(G, mu)
    assert np.array_equal(X, X.astype(np.float32).astype(np.float64))
    beta = rng.normal(size=P) * rng.choice([0.0, 1e-3, 1.0], size=P)
    sets = [(0, 100), (100, 92), (256, P - 256)]
    g = RP.predict_draw(X, beta, sets)
    B = RP.bound(X, beta, sets)
    for s, (c0, n) in enumerate(sets):
        assert np.all(np.abs(g[s] - X[:, c0:c0 + n] @ beta[c0:c0 + n]) <= 2 * B[s])
    owned = np.r_[0:192, 256:P]
    assert np.all(np.abs(g[3] - X[:, owned] @ beta[owned]) <= 2 * B[3])
    assert np.array_equal(g[3], ((0.0 + g[0]) + g[1]) + g[2])
    for i in range(min(Np, 3)):
        for s, (c0, n) in enumerate(sets):
            exact = sum(Fraction(float(X[i, j])) * Fraction(float(beta[j])) for j in range(c0, c0 + n))
            assert abs(Fraction(float(g[s, i])) - exact) <= Fraction(float(B[s, i]))
    # columns no set owns contribute nothing
    beta2 = beta.copy(); beta2[192:256] = 7.0
    assert np.array_equal(RP.predict_draw(X, beta2, sets), g)


def test_restatement_with_analytic_centring():
    """Byte tiles: the code sum minus sum_j m_j beta_j, each formed in chunks, against Float64 (G - m) @ beta; the bound counts both sums."""
    rng = np.random.default_rng(4)
    Np, P = 30, 2500
    G = rng.integers(0, 3, size=(Np, P)).astype(np.float64)
    m = rng.uniform(0.1, 1.9, size=P)
    beta = rng.normal(size=P)
    sets = [(0, 2200), (2200, 300)]
    g = RP.predict_draw(G, beta, sets, mean=m)
    B = RP.bound(G, beta, sets, mean=m)
    assert np.all(np.abs(g[2] - (G - m[None, :]) @ beta) <= 2 * B[2])
    s1 = np.zeros_like(g); s2 = np.zeros_like(g)
    RP.accumulate(s1, s2, g); RP.accumulate(s1, s2, g)
    assert np.array_equal(s1, g + g) and np.array_equal(s2, g * g + g * g)


def test_prediction_summary_and_file(ngp, tmp_path):
    rng = np.random.default_rng(2)
    g = rng.normal(size=(5, 3, 7))                                  # five draws, two sets + total, seven individuals
    ps = dict(sum=g.sum(axis=0), sum2=(g * g).sum(axis=0), nKept=5)
    pr = ngp.prediction_summary(ps)
    assert np.allclose(pr["mean"], g[:, 2].mean(axis=0)) and np.allclose(pr["sd"], g[:, 2].std(axis=0))
    assert np.allclose(pr["sets"][1]["sd"], g[:, 1].std(axis=0)) and len(pr["sets"]) == 2
    flat = dict(sum=np.ones((2, 3)), sum2=np.ones((2, 3)) * (1 - 1e-17), nKept=1)  # a variance that rounds below zero is an SD of zero
    assert np.array_equal(ngp.prediction_summary(flat)["sd"], np.zeros(3))
    with pytest.raises(ValueError):
        ngp.prediction_summary(dict(sum=np.zeros((2, 3)), sum2=np.zeros((2, 3)), nKept=0))
    pred = dict(ids=[f"a{i}" for i in range(7)], mean=pr["mean"], sd=pr["sd"], sets={"M1": pr["sets"][0], "M2": pr["sets"][1]})
    path = tmp_path / "gebvPredict.txt"
    ngp.write_prediction_file(path, pred)
    lines = path.read_text().splitlines()
    assert lines[0].split("\t") == ["ID", "mean", "sd", "mean_M1", "sd_M1", "mean_M2", "sd_M2"] and len(lines) == 8
    assert lines[1].split("\t")[0] == "a0" and float(lines[1].split("\t")[1]) == pr["mean"][0]
    back = ngp.read_prediction_file(path)
    assert back["ids"] == pred["ids"] and np.array_equal(back["mean"], pred["mean"]) and np.array_equal(back["sd"], pred["sd"])
    assert list(back["sets"]) == ["M1", "M2"] and np.array_equal(back["sets"]["M2"]["sd"], pred["sets"]["M2"]["sd"])


def test_runlmem_predict_arguments_are_checked_before_any_device_work(ngp, tmp_path):
    """Every mistake in predict= is a ValueError (a GBLUP term: NotImplementedError) raised from host checks -- this test runs where
    there is no device, so a check that came after the first device call could not raise what is expected here."""
    rng = np.random.default_rng(3)
    N = 30
    A, B = rng.integers(0, 3, size=(N, 20)).astype(np.uint8), rng.integers(0, 3, size=(N, 12)).astype(np.uint8)
    np.save(tmp_path / "a.npy", A); np.save(tmp_path / "b.npy", B)
    f = f'y ~ 1 + SNP(M1,"{tmp_path / "a.npy"}") + SNP(M2,"{tmp_path / "b.npy"}")'
    data = {"y": rng.normal(size=N)}
    k = [0]

    def run(**kw):
        k[0] += 1
        return ngp.runLMEM(f, data, 4, 2, 1, outFolder=str(tmp_path / f"o{k[0]}"), **kw)

    pa, pb = A[:5], B[:5]
    with pytest.raises(ValueError, match="one source per SNP"):
        run(predict={"M1": pa})
    with pytest.raises(ValueError, match="one source per SNP"):
        run(predict={"M1": pa, "M2": pb, "M3": pb})
    with pytest.raises(ValueError, match="mapping"):
        run(predict=[pa, pb])
    with pytest.raises(ValueError, match="columns"):
        run(predict={"M1": pa, "M2": pb[:, :11]})
    with pytest.raises(ValueError, match="same individuals"):
        run(predict={"M1": pa, "M2": pb[:4]})
    with pytest.raises(ValueError, match="predict_ids"):
        run(predict={"M1": pa, "M2": pb}, predict_ids=["x"] * 4)
    with pytest.raises(ValueError, match="predict_ids"):
        run(predict_ids=["x"] * 5)
    with pytest.raises(NotImplementedError, match="GBLUP"):
        run(predict={"M1": pa, "M2": pb}, VCV={"M2": ngp.Random("G", 1.0)})
    with pytest.raises(ValueError, match="0..255"):
        run(predict={"M1": pa.astype(np.float64) + 0.5, "M2": pb}, storage="u8")


def test_symbols_header_and_library(ngp):
    hdr = open(os.path.join(ROOT, "include", "nextgp_hip.h")).read()
    assert "#define NGP_ABI_VERSION 4" in hdr                       # additive: the version stays
    decl = c_declarations()
    for s in NEW:
        assert s in ngp.SYMBOLS and s in decl, s
    assert decl["ngp_get_prediction"] == ["ngp_handle*", "double*", "double*", "int64_t", "int64_t", "int64_t*"]
    assert decl["ngp_prediction_columns_u8"] == ["ngp_handle*", "int64_t", "uint8_t*", "int64_t", "int64_t", "int32_t"]
    src = open(os.path.join(ROOT, "nextgp.jl_amd", "csrc", "ngp_api.hip")).read()
    for s in NEW:                                                   # every entry point behind the exception barrier
        m = re.search(r"int32_t " + s + r"\([^)]*\) \{\n    NGP_TRY\n", src)
        assert m, s
    for unit in ("ngp_sweep.h", "ngp_sweep_inst.hip", "ngp_sweep_body.inc", "ngp_sweep_multi_body.inc"):   # the sweep units do not know it
        txt = open(os.path.join(ROOT, "nextgp.jl_amd", "csrc", unit)).read()
        assert "ngp_predict" not in txt and "k_predict" not in txt and "PredItem" not in txt


def test_julia_binds_the_prediction_entry_points():
    decl = c_declarations()
    calls = {name: (ret, types, vals) for name, ret, types, vals in julia_ccalls()}
    for s in NEW:
        assert s in calls, s
        ret, types, vals = calls[s]
        assert ret == "Int32" and len(types) == len(decl[s]) == len(vals)
        assert all(jt in C2J[ct] for jt, ct in zip(types, decl[s])), s
    jl = open(os.path.join(ROOT, "nextgp.jl_amd", "julia", "NextGPHIP.jl")).read()
    assert "function setPrediction!(h::Handle, Mpred::Dict" in jl and "function getPrediction(h::Handle)" in jl
    body = jl[jl.index("function setPrediction!"):jl.index("function getPrediction")]
    assert "begin_prediction_panel!" in body and "prediction_columns!(h, col0, Mpred[s]" in body and "end_prediction_panel!" in body
