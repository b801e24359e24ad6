"""Weighted residuals (E.str == "D", src/mme.jl:71-75) without a device: the two new entry points of the C ABI, the front door of
runLMEM up to the point where a device is needed, and the weighted reference-order restatement against a closed form."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ngp_set_residual_weights", "ngp_get_residual_weights")


def test_header_declares_and_library_exports_the_weight_calls(ngp):
    hdr = open(os.path.join(ROOT, "include", "nextgp_hip.h")).read()
    assert re.search(r"int32_t ngp_set_residual_weights\(ngp_handle \*h, const double \*w, int64_t N\);", hdr)
    assert re.search(r"int32_t ngp_get_residual_weights\(ngp_handle \*h, double \*w, int64_t N\);", hdr)
    import __graft_entry__ as g
    g.build()
    lib = ngp.load()
    for s in NEW:
        assert hasattr(lib, s) and s in ngp.SYMBOLS
    lib.ngp_abi_version.restype = C.c_int32
    assert lib.ngp_abi_version() == 4                          # a new function is backward compatible: no bump
    # a null handle is an argument error with a message, never a crash (no device needed to see that)
    for s in NEW:
        f = getattr(lib, s)
        f.restype = C.c_int32
        assert f(None, None, C.c_int64(0)) == -1


def test_weight_calls_sit_behind_the_exception_barrier():
    src = open(os.path.join(ROOT, "nextgp.jl_amd", "csrc", "ngp_api.hip")).read().split("\n")
    for s in NEW:
        i = next(k for k, line in enumerate(src) if line.startswith(f"int32_t {s}("))
        end = next(k for k in range(i, len(src)) if src[k] == "}")
        body = src[i:end]
        assert any("NGP_TRY" in b for b in body) and any("NGP_CATCH(h)" in b for b in body), s


def test_julia_shim_sets_the_weights_on_both_seams():
    jl = open(os.path.join(ROOT, "nextgp.jl_amd", "julia", "NextGPHIP.jl")).read()
    assert "set_residual_weights!(h, Vector{Float64}(E.iVarStr))" in jl
    assert 'error("weighted residuals: use the reference sampler")' not in jl
    integ = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert '&& E.str == "I"' not in integ and "set_residual_weights!" in integ


def _write_geno(tmp_path, N=12, P=5):
    g = np.random.default_rng(0).integers(0, 3, size=(N, P))
    path = tmp_path / "g.txt"
    np.savetxt(path, g, fmt="%d", delimiter=" ")
    return str(path)


def test_runLMEM_front_door_for_D(ngp, tmp_path):
    N = 12
    y = np.linspace(0.0, 1.0, N)
    d = np.linspace(0.5, 2.0, N)
    # the refusal is gone: a D structure now gets as far as the genotype file (which does not exist here -- no device involved)
    with pytest.raises(FileNotFoundError):
        ngp.runLMEM('y ~ 1 + SNP(M, "/nonexistent/geno.txt")', {"y": y}, 2, 0, 1, outFolder=str(tmp_path / "o1"),
                    VCV={"M": ngp.BayesPR(9999, 0.01), "e": ngp.Random(d, 1.0)})
    from nextgp_jl_amd.api import _residual_weights
    w = _residual_weights(ngp.Random(list(d), 1.0), N)
    assert np.array_equal(w, 1.0 / d)                           # inv.(d): the same IEEE division
    assert _residual_weights(ngp.Random("I", 1.0), N) is None and _residual_weights(ngp.Random([], 1.0), N) is None
    geno = _write_geno(tmp_path, N)
    for bad in (d[:-1], np.r_[d[:-1], 0.0], np.r_[d[:-1], -1.0], np.r_[d[:-1], np.nan], np.r_[d[:-1], np.inf]):
        with pytest.raises(ValueError, match="residual structure D"):
            ngp.runLMEM(f'y ~ 1 + SNP(M, "{geno}")', {"y": y}, 2, 0, 1, outFolder=str(tmp_path / "o2"), overwrite=True,
                        VCV={"M": ngp.BayesPR(9999, 0.01), "e": ngp.Random(bad, 1.0)})
    with pytest.raises(NotImplementedError, match="compact storage"):
        ngp.runLMEM(f'y ~ 1 + SNP(M, "{geno}")', {"y": y}, 2, 0, 1, outFolder=str(tmp_path / "o3"), storage="u8",
                    VCV={"M": ngp.BayesPR(9999, 0.01), "e": ngp.Random(d, 1.0)})
    with pytest.raises(NotImplementedError, match="only"):
        ngp.runLMEM(f'y ~ 1 + SNP(M, "{geno}")', {"y": y}, 2, 0, 1, outFolder=str(tmp_path / "o4"), overwrite=True,
                    VCV={"M": ngp.BayesPR(9999, 0.01), "e": ngp.Random("A", 1.0)})


def test_weighted_restatement_against_the_closed_form(O):
    """One SNP, no intercept, variances held: the draw of beta is mean + sd z with mean = x'Wy / (x'Wx + varE / varBeta) and
    sd = sqrt(varE / (x'Wx + varE / varBeta)); varE = (df S + sum w ycorr^2) / chi2.  Plain Python floats, no numpy dots."""
    from ref_numpy_weighted import WeightedRefChain
    x = [1.0, -1.0, 0.5, -0.5, 2.0, -2.0]
    y = [0.3, -0.2, 0.1, 0.4, 1.1, -0.9]
    w = [0.5, 2.0, 1.0, 4.0, 0.25, 1.5]
    vb, e_df, e_scale = 0.05, 4.0, 0.1
    ref = WeightedRefChain(O, np.array(x).reshape(6, 1), np.array(y), np.array(w), seed=4, chain=0, intercept=False)
    ref.add_set(0, 1, 0, 4.0, 0.02, [(0, 1)], [vb])
    ref.E_df, ref.E_scale = e_df, e_scale
    ref.sampleBayesPR = lambda si, varE: _pr_fixed_variance(ref, si, varE)   # hold varBeta: only the conditional of beta is checked
    ref.run(1)
    chi = float(O.draws(4, 0, 1, 1, 0, 2, 1, e_df + 6, 0.0, indexed=True)[0])
    z = float(O.draws(4, 0, 1, 3, 0, 1, 1, indexed=True)[0])
    varE = (e_df * e_scale + sum(wi * yi * yi for wi, yi in zip(w, y))) / chi
    xwx = sum(wi * xi * xi for wi, xi in zip(w, x))
    xwy = sum(wi * xi * yi for wi, xi, yi in zip(w, x, y))
    lhs = xwx + varE / vb
    beta = xwy / lhs + math.sqrt(varE / lhs) * z
    assert abs(ref.varE - varE) <= 1e-14 * varE
    assert abs(ref.beta[0][0] - beta) <= 1e-12 * max(1.0, abs(beta))
    assert np.allclose(ref.ycorr, np.array(y) - np.array(x) * beta, rtol=0, atol=1e-14)


def _pr_fixed_variance(ref, si, varE):
    M, beta, vb = ref.M[si], ref.beta[si], ref.varBeta[si]
    iVarE = 1.0 / varE
    for locus in range(len(beta)):
        ref.ycorr += beta[locus] * M["data"][:, locus]
        rhs = np.dot(M["Mp"][locus], ref.ycorr) * iVarE + M["rhs"][locus]
        lhs = M["mpm"][locus] * iVarE + M["lhs"][locus] + 1.0 / vb[0]
        beta[locus] = ref.sampleBeta(si, locus, rhs / lhs, lhs)
        ref.ycorr -= beta[locus] * M["data"][:, locus]
