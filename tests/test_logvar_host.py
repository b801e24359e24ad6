"""BayesLV sets without a GPU: the C ABI's new names, the BayesLV prior and its design matrix, file names and headers, and the two
restatements of tests/ref_logvar.py against each other and against libm."""
import math
import os
import re

import numpy as np
import pytest

import ref_logvar as RL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ngp_add_marker_set_lv", "ngp_get_lv_state", "ngp_set_lv_state")


def test_header_declares_and_library_exports_the_new_calls(ngp):
    import __graft_entry__ as g
    g.build()
    hdr = open(os.path.join(ROOT, "include", "nextgp_hip.h")).read()
    lib = ngp.load()
    for s in NEW:
        assert re.search(r"int32_t\s+" + s + r"\s*\(", hdr), s
        assert hasattr(lib, s) and s in ngp.SYMBOLS, s
    assert re.search(r"#define\s+NGP_METHOD_BAYESLV\s+5\b", hdr) and re.search(r"#define\s+NGP_ABI_VERSION\s+4\b", hdr)
    rng = open(os.path.join(ROOT, "nextgp.jl_amd", "csrc", "ngp_rng.h")).read()
    for name, kind in (("NGP_KIND_LV_UNIFORM", 14), ("NGP_KIND_LV_NORMAL", 15), ("NGP_KIND_LV_START", 16)):
        assert re.search(rf"#define\s+{name}\s+{kind}\b", rng), name
    assert not re.search(r"#define\s+NGP_KIND_\w+\s+10\b", rng)     # kind 10 stays unused


def _api(ngp):
    from nextgp_jl_amd import api
    return api


def test_bayeslv_prior_and_design_matrix(ngp):
    api = _api(ngp)
    cov = dict(x1=np.arange(6.0), x2=np.array([0, 1, 0, 1, 1, 0]), s=np.array(list("abcabc")))
    p = api.BayesLV(0.001, "0 ~ x1 + x2", cov, 0.5)
    assert (p.v, p.varZeta, p.name, p.estimateVarZeta) == (0.001, 0.5, "BayesLV", False)
    assert api.BayesLV(0.001, "0 ~ x1", cov, 0.5, estimateVarZeta=0.01).estimateVarZeta == 0.01
    C, names = api.lv_design_matrix(p.f, cov)                       # modelmatrix: the intercept column first
    assert names == ["(Intercept)", "x1", "x2"] and C.shape == (6, 3)
    assert np.array_equal(C[:, 0], np.ones(6)) and np.array_equal(C[:, 1], cov["x1"]) and np.array_equal(C[:, 2], cov["x2"].astype(float))
    for f in ("0 ~ 0 + x2 + x1", "0 ~ x2 + x1 - 1", "y~-1+x2+x1"):   # no intercept; the formula's order, not the mapping's
        C, names = api.lv_design_matrix(f, cov)
        assert names == ["x2", "x1"] and np.array_equal(C[:, 0], cov["x2"].astype(float)), f
    assert api.lv_design_matrix("0 ~ 1", cov)[1] == ["(Intercept)"]
    with pytest.raises(NotImplementedError, match="StatsModels"):
        api.lv_design_matrix("0 ~ x1 + s", cov)                     # a non-numeric column names the reference
    for f in ("0 ~ x1 * x2", "0 ~ x1 + x1 & x2", "0 ~ log(x1)"):
        with pytest.raises(NotImplementedError, match="mme.jl"):
            api.lv_design_matrix(f, cov)
    with pytest.raises(KeyError):
        api.lv_design_matrix("0 ~ x9", cov)
    with pytest.raises(ValueError):
        api.lv_design_matrix("0 ~ 0", cov)
    with pytest.raises(ValueError):
        api.BayesLV(0.001, "x1 + x2", cov, 0.5)
    with pytest.raises(ValueError):
        api.BayesLV(0.001, "0 ~ x1", cov, 0.5, estimateVarZeta=1)
    with pytest.raises(ValueError):
        api.lv_design_matrix("0 ~ " + " + ".join(f"z{i}" for i in range(17)), {f"z{i}": np.ones(3) for i in range(17)})
    assert "BayesLV" not in api.__doc__.split("outside the")[1].split("accelerated path")[0]


def test_file_names_and_headers(ngp, tmp_path):
    api = _api(ngp)
    prior = api.BayesLV(0.01, "0 ~ x1 + x2", dict(x1=np.zeros(4), x2=np.zeros(4)), 1.0)
    sets = [dict(id=0, name="M", members=["M"], cols=np.arange(4)[:, None], P=4, prior=prior, nreg=4, nvb=4, k=1, lv=0, ncov=3,
                 cnames=["(Intercept)", "x1", "x2"])]
    api._write_headers(str(tmp_path), sets, ["(Intercept)"])
    head = lambda n: open(os.path.join(str(tmp_path), n)).readline().rstrip("\n").split("\t")
    assert head("cMOut") == ["c1", "c2", "c3"]                      # src/mme.jl:577-580
    assert head("varZetaMOut") == ["varZeta"]
    assert head("varMOut") == ["reg_1", "reg_2", "reg_3", "reg_4"]  # one column per locus (nVarCov = loci, src/mme.jl:589-591)
    assert head("betaMOut") == ["M1", "M2", "M3", "M4"]
    assert api._regions_for(prior, 3, "", str(tmp_path), "M") == [(0, 1), (1, 2), (2, 3)]


def test_icpc_restated(ngp):
    rng = np.random.default_rng(2)
    for ncov in (1, 3, 16):
        C = rng.normal(size=(500, ncov))
        C[:, 0] = 1.0
        A = C.T @ C
        ridge = np.abs(np.diag(A)).min() / 10000
        assert np.allclose(RL.icpc(C), np.linalg.inv(A + ridge * np.eye(ncov)), rtol=1e-12, atol=0)


def _ulp_gap(a, b):
    return abs(a - b) / math.ulp(b)


def test_det_exp_any_within_2_ulp(O):
    rng = np.random.default_rng(1)
    mags = np.exp(rng.uniform(math.log(1e-3), math.log(700.0), 4000))
    worst = 0.0
    for x in np.concatenate([mags, -mags]):
        worst = max(worst, _ulp_gap(RL.det_exp_any(O, float(x)), math.exp(float(x))))
    print("det_exp_any: largest gap to math.exp", worst, "ulp")
    assert worst <= 2.0
    assert RL.det_exp_any(O, 0.0) == 1.0 and RL.det_exp_any(O, -0.0) == 1.0
    assert RL.det_exp_any(O, -800.0) == 0.0 and RL.det_exp_any(O, 800.0) == math.inf
    assert math.isnan(RL.det_exp_any(O, math.nan))


def _inputs(n, ncov, seed, spread=1.0):
    rng = np.random.default_rng(seed)
    C = rng.normal(size=(n, ncov))
    C[:, 0] = 1.0
    if ncov > 1:
        C[:, 1] = rng.integers(0, 2, n)
    vb = np.exp(rng.normal(-5.0, spread, n))
    beta = rng.normal(size=n) * np.sqrt(vb)
    beta[::7] = 0.0                                                  # exact zeros
    # very large effects: bi^2 / (2 vari) = 300 (exp(-300) is a normal number) or 2000 (exp underflows to 0 in libm and in det_exp alike).
    # Between 708 and 745 libm returns a subnormal where det_exp returns 0 (ngp_rng.h): there the device drops the lower clamp of the
    # slice a little earlier than the reference, a documented difference ("BayesLV sets"), kept out of the 1e-12 comparison
    big = np.arange(3, n, 11)
    beta[big] = np.sign(beta[big]) * np.sqrt(2.0 * vb[big] * np.where(np.arange(len(big)) % 2 == 0, 300.0, 2000.0))
    zeta = rng.uniform(size=n)
    return C, vb, beta, zeta


def test_slice_contains_the_current_variance(O):
    """The slice is cut around the current variance, so lbound <= vari <= rbound up to rounding and no locus is trapped."""
    C, vb, beta, zeta = _inputs(1500, 3, 5)
    bounds = []
    out = RL.lv_step_blocked(O, 7, 1, 1, 2, beta, vb, zeta, C, RL.icpc(C), 0.8, 1, bounds=bounds)
    assert out[4] == 0 and len(bounds) == 1500
    for v, lb, rb in bounds:
        assert lb <= v * (1 + 1e-12) and v <= rb * (1 + 1e-12), (v, lb, rb)
    assert np.all(out[0] > 0) and np.all(np.isfinite(out[2])) and out[3] > 0


@pytest.mark.parametrize("est", [False, True, 0.25], ids=["fixed", "var_zeta", "fraction"])
@pytest.mark.parametrize("ncov", [1, 3, 16])
def test_blocked_step_against_reference_order(O, ncov, est):
    n = 1000
    C, vb, beta, zeta = _inputs(n, ncov, 11 + ncov)
    X = np.zeros((4, n)); y = np.zeros(4)
    ref = RL.LVRefChain(O, X, y, seed=5, chain=2)
    ref.add_set_lv(0, n, 0.01, C, 0.6, est=est, zeta0=zeta)
    M = ref.M[0]
    ref.varBeta[0][:] = vb; M["logVar"][:] = np.log(vb); ref.beta[0][:] = beta
    ref.iter = 3
    # the variance model alone: a sweep over a zero panel with varE = 1 redraws beta from its prior -- put the test's beta back
    draw = ref.sampleBeta
    ref.sampleBeta = lambda si, locus, meanBeta, lhs: beta[locus]
    ref.sampleBayesLV(0, 1.0)
    ref.sampleBeta = draw
    mode = 0 if est is False else 1 if est is True else 2
    v2, c, z, vz, tr = RL.lv_step_blocked(O, 5, 2, 3, 0, beta, vb, zeta, C, M["iCpC"], 0.6, mode, 0.25 if mode == 2 else 0.0)
    rel = lambda a, b: np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)
    gaps = dict(varBeta=np.abs(v2 / ref.varBeta[0] - 1).max(), c=rel(c, M["c"]), zeta=rel(z, M["SNPVARRESID"]), varZeta=abs(vz / M["varZeta"][0] - 1))
    print("blocked against reference order:", gaps, "trapped", tr, M["trapped"])
    assert tr == 0 and M["trapped"] == 0
    for k, g in gaps.items():
        assert g <= 1e-12, (k, g)
    assert (vz == 0.6) == (mode == 0)


def test_variance_step_chains_differ_by_rounding_only(O):
    """What the whole-chain GPU test's tolerance rests on: two reference-order chains that differ only in the rounding of the
    variance step (libm and numpy dots against det_log / det_exp and the segment order) over 30 iterations."""
    N, P = 120, 96
    X, _ = O.generate_panel(N, P, seed=3)
    X = X.astype(np.float64)
    rng = np.random.default_rng(4)
    a = rng.integers(0, 2, 64).astype(float)
    bt = rng.normal(size=64) * np.where(a == 1, 0.5, 0.05)
    y = 3.0 + X[:, :64] @ bt + rng.normal(size=N)
    C = np.column_stack([np.ones(64), a])
    chains = []
    for blocked in (False, True):
        ch = RL.LVRefChain(O, X, y, seed=9, chain=0, blocked_step=blocked)
        ch.add_fixed(np.linspace(-1, 1, N))
        ch.add_set_lv(0, 64, 0.01, C, 0.5, est=True)
        ch.add_set(64, 32, 0, 4.0, 0.005, [(0, 32)], [0.01])
        ch.E_df, ch.E_scale = 4.0, 0.5
        chains.append(ch)
    worst = 0.0
    for it in range(30):
        for ch in chains:
            ch.run(1)
        p, q = chains
        for u, v in ((p.varBeta[0], q.varBeta[0]), (p.beta[0], q.beta[0]), (p.ycorr, q.ycorr), (p.M[0]["c"], q.M[0]["c"])):
            worst = max(worst, np.abs(u - v).max() / max(np.abs(v).max(), 1e-6))
    print("largest relative gap over 30 iterations:", worst)
    assert worst <= 1e-9
