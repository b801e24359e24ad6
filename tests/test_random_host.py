"""(1|g) random-effect sets on the host side: formula parsing, level coding, K as CSR, priors, file names, and closed-form checks of the
blocked restatement (tests/ref_random.py).  No GPU needed."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ngp_pkg import load_pkg  # noqa: E402

ngp = load_pkg()
from nextgp_jl_amd import api  # noqa: E402
from nextgp_jl_amd._lib import k_csr  # noqa: E402


def test_header_declares_and_library_exports_the_random_calls():
    import ctypes as C
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "nextgp_hip.h")).read()
    for name in ("ngp_add_random_set", "ngp_get_random", "ngp_set_random", "ngp_sample_random_set"):
        assert re.search(rf"int32_t {name}\(ngp_handle \*h,", hdr), name
        assert name in ngp.SYMBOLS
    import __graft_entry__ as g
    g.build()
    lib = ngp.load()
    lib.ngp_abi_version.restype = C.c_int32
    assert lib.ngp_abi_version() == 4                          # new functions, unchanged layouts without random sets: no bump
    f = lib.ngp_add_random_set
    f.restype = C.c_int32
    assert f(None, None, C.c_int64(1), None, None, None, C.c_double(4.0), C.c_double(1.0), C.c_double(1.0), None) == -1


def test_parse_formula_accepts_random_intercepts():
    p = api.parse_formula('y ~ 1 + x + (1|herd) + (1 | litter) + SNP(M, "g.txt")', random_effects=True)
    assert p.random == ["herd", "litter"]
    assert p.covariates == ["x"]
    assert [t.name for t in p[2]] == ["M"]
    assert api.parse_formula("y ~ 1 + x", random_effects=True).random == []
    with pytest.raises(NotImplementedError, match="random_effects=True"):   # the plain call refuses them, as it always did
        api.parse_formula('y ~ 1 + (1|herd) + SNP(M, "g.txt")')


@pytest.mark.parametrize("term,what", [("PED(ID)", "PedigreeBase"), ("(x|herd)", "functions.jl:75-89"), ("(1|herd & year)", "functions.jl:75-89"),
                                       ("x & z", "interactions")])
def test_parse_formula_refusals_name_the_reference(term, what):
    with pytest.raises(NotImplementedError, match=what):
        api.parse_formula(f"y ~ 1 + {term}", random_effects=True)


def test_random_levels_are_sorted_unique_values():
    codes, names = api.random_levels(np.array(["h3", "h1", "h3", "h2", "h1"]))
    assert names == ["h1", "h2", "h3"]
    assert codes.tolist() == [2, 0, 2, 1, 0] and codes.dtype == np.int32
    codes, names = api.random_levels(np.array([30, 10, 20, 10]))
    assert names == ["10", "20", "30"] and codes.tolist() == [2, 0, 1, 0]


def test_k_csr_of_dense_and_triple():
    K = np.array([[2.0, -1.0, 0.0], [-1.0, 3.0, 0.5], [0.0, 0.5, 1.0]])
    kp, kc, kv = k_csr(K)
    assert kp.tolist() == [0, 2, 5, 7] and kc.tolist() == [0, 1, 0, 1, 2, 1, 2]
    assert kv.tolist() == [2.0, -1.0, -1.0, 3.0, 0.5, 0.5, 1.0]
    assert kp.dtype == np.int64 and kc.dtype == np.int32 and kv.dtype == np.float64
    kp2, kc2, kv2 = k_csr(([0, 1], [0], [4.0]))
    assert kp2.tolist() == [0, 1] and kc2.tolist() == [0] and kv2.tolist() == [4.0]


def test_random_prior_df_scale_per_mme():
    K, df, scale, v = api.random_prior({}, "herd", 5)            # no prior: Random("I", 100), src/mme.jl:40-44
    assert K is None and df == 4.0 and v == 100.0 and scale == 100.0 * (4.0 - 2.0) / 4.0
    K, df, scale, v = api.random_prior({"1|herd": api.Random("I", 2.5)}, "herd", 5)
    assert K is None and df == 4.0 and scale == 2.5 * 2.0 / 4.0 and v == 2.5
    S = np.array([[2.0, 0.5], [0.5, 1.0]])
    K, df, scale, v = api.random_prior({"(1|herd)": api.Random(S, 1.0)}, "herd", 2)
    assert np.allclose(K @ S, np.eye(2)) and np.array_equal(K, K.T)
    with pytest.raises(NotImplementedError, match="PedigreeBase"):
        api.random_prior({"1|herd": api.Random("A", 1.0)}, "herd", 2)
    with pytest.raises(ValueError):
        api.random_prior({"1|herd": api.Random(np.eye(3), 1.0)}, "herd", 2)


def test_random_file_names_pinned():
    # Julia: string(:(1|herd)) == "1 | herd"; join(:(1|herd).args)[2:end] == "1herd" (src/mme.jl:548-556)
    assert api.random_file_names("herd") == ("u1 | herd", "varU1 | herd", "1herd")


class _FakeOracle:
    """Draw layer stand-in for the closed-form checks: every normal is z, every chi-square c (the restatement only asks for these)."""

    def __init__(self, z, c):
        self.z, self.c = z, c

    def draws(self, seed, chain, it, kind, index, what, n, p1, p2, indexed=True):
        return np.array([self.z if what == 1 else self.c])


def test_blocked_restatement_closed_form_identity():
    import ref_random as RR
    rng = np.random.default_rng(5)
    N, q = 300, 7
    level = rng.integers(0, q - 1, size=N)          # the last level has no records: drawn from its prior conditional
    y = rng.normal(size=N)
    u = rng.normal(size=q)
    varE, varU, z, c = 1.7, 0.6, 0.25, 9.0
    zpz = RR.zpz_of(level, q)
    yt, un, vU = RR.random_step_blocked(_FakeOracle(z, c), 1, 0, 1, 0, y, None, level, q, None, zpz, u, varU, varE, 4.0, 0.3)
    for l in range(q):
        m = level == l
        Yi = (y[m].sum() + m.sum() * u[l]) / varE
        lhs = m.sum() / varE + 1.0 / varU
        assert zpz[l] == m.sum()
        assert math.isclose(un[l], Yi / lhs + math.sqrt(1.0 / lhs) * z, rel_tol=1e-12, abs_tol=1e-12)
    assert math.isclose(un[q - 1], math.sqrt(varU) * z, rel_tol=1e-12)
    assert np.allclose(yt, y - (np.asarray(un) - u)[level], rtol=0, atol=1e-12)
    assert math.isclose(vU, (0.3 * 4.0 + float(np.dot(un, un))) / c, rel_tol=1e-12)


def test_blocked_restatement_matches_reference_gauss_seidel():
    import ref_random as RR
    rng = np.random.default_rng(6)
    N, q = 200, 6
    level = rng.integers(0, q, size=N)
    A = rng.normal(size=(q, q))
    K = A @ A.T + q * np.eye(q)
    K[np.abs(K) < 1.0] = 0.0
    K = (K + K.T) / 2
    y, u = rng.normal(size=N), rng.normal(size=q)
    varE, varU, z, c = 1.3, 0.8, -0.4, 7.0
    zpz = RR.zpz_of(level, q)
    yt, un, vU = RR.random_step_blocked(_FakeOracle(z, c), 1, 0, 1, 0, y, None, level, q, K, zpz, u, varU, varE, 4.0, 0.3)
    ref = u.copy()
    Yi = np.array([(y[level == l].sum() + zpz[l] * u[l]) / varE for l in range(q)])
    for l in range(q):                               # src/functions.jl:63-71
        ref[l] = 0.0
        rhs = Yi[l] - np.dot(K[:, l], ref) / varU
        lhs = zpz[l] / varE + K[l, l] / varU
        ref[l] = rhs / lhs + math.sqrt(1.0 / lhs) * z
    assert np.allclose(un, ref, rtol=1e-12, atol=1e-12)
    assert math.isclose(vU, (0.3 * 4.0 + float(ref @ K @ ref)) / c, rel_tol=1e-10)
