"""BayesRCpi sets without a GPU: tests/ref_bayesrc.py -- the specification the device is held to -- against closed forms on a single
locus, the host mirror's routing, file headers and refusals, and the Julia shim's new bindings (statically)."""
import os
import re

import numpy as np
import pytest
from scipy import stats

import pivot_models as PM
import ref_bayesrc as RB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = PM.SEED


def one_locus(mask, prob, r, A=3, vc=(0.0, 0.05, 1.0), pi=(0.6, 0.3, 0.1), v=0.02, varE=0.4, mpm=128.0):
    return dict(mask=mask, prob=prob, r=r, A=A, vc=list(vc), pi=list(pi), v=v, varE=varE, mpm=mpm)


LOCI = {"all": one_locus([1, 1, 1], [0.2, 0.5, 0.3], 9.0), "two": one_locus([1, 0, 1], [0.7, 0.0, 0.3], -14.0),
        "one": one_locus([0, 1, 0], [0.0, 1.0, 0.0], 4.0), "flat": one_locus([1, 1, 1], [1 / 3, 1 / 3, 1 / 3], 0.0)}


@pytest.mark.parametrize("name", list(LOCI))
def test_blocked_rule_follows_the_exact_law_of_one_locus(O, name):
    """lane_tables + lane_eval over keyed draws (replicates by the iteration key) against locus_law evaluated exactly: annotation
    probabilities P_a S_a / sum and the class law c_v prod_{m<v} (1 - c_m) of the fresh-uniform search, the last class taking the rest.
    Randomised probability integral transform of the joint outcome; the bound is the KS condition of tests/pivots.py."""
    L = LOCI[name]
    A, K = L["A"], len(L["vc"])
    iVarE = 1.0 / L["varE"]
    logpi = [[O.det_log(p) for p in L["pi"]] for _ in range(A)]
    pa, pc = RB.locus_law(L["r"] * iVarE, L["mpm"] * iVarE, [L["v"]] * A, L["vc"], [L["pi"]] * A, L["prob"])
    assert abs(pa.sum() - 1.0) < 1e-12 and all(abs(pc[a].sum() - 1.0) < 1e-12 for a in range(A) if L["mask"][a])
    joint = (pa[:, None] * pc).ravel()
    F = np.concatenate([[0.0], np.cumsum(joint)])
    rng = np.random.default_rng(3)
    us, cnt = [], np.zeros(A * K)
    for it in range(1, 3001):
        T = RB.lane_tables(O, SEED, 0, it, 2, 11, L["mpm"], 0.0, iVarE, [L["v"]] * A, L["vc"], logpi, L["prob"], L["mask"])
        c, a, cand = RB.lane_eval(O, T, L["r"], iVarE, 0.0, 0.0)
        assert L["mask"][a] == 1 and (cand == 0.0) == (L["vc"][c] == 0.0)
        i = a * K + c
        cnt[i] += 1
        us.append(F[i] + rng.uniform() * (F[i + 1] - F[i]))
    p = float(stats.kstest(us, "uniform").pvalue)
    assert p > PM.KS_MIN, (p, cnt.tolist(), (joint * 3000).tolist())
    assert all(cnt[i] == 0 for i in range(A * K) if joint[i] == 0.0)


def test_a_wrong_law_is_seen(O):
    """Power: the same draws against the law WITHOUT the annotation probabilities fail the same bound."""
    L = LOCI["all"]
    A, K = 3, 3
    iVarE = 1.0 / L["varE"]
    logpi = [[O.det_log(p) for p in L["pi"]] for _ in range(A)]
    pa, pc = RB.locus_law(L["r"] * iVarE, L["mpm"] * iVarE, [L["v"]] * A, L["vc"], [L["pi"]] * A, [1 / 3] * 3)
    F = np.concatenate([[0.0], np.cumsum((pa[:, None] * pc).ravel())])
    rng = np.random.default_rng(3)
    us = []
    for it in range(1, 3001):
        T = RB.lane_tables(O, SEED, 0, it, 2, 11, L["mpm"], 0.0, iVarE, [L["v"]] * A, L["vc"], logpi, L["prob"], L["mask"])
        c, a, _ = RB.lane_eval(O, T, L["r"], iVarE, 0.0, 0.0)
        us.append(F[a * K + c] + rng.uniform() * (F[a * K + c + 1] - F[a * K + c]))
    assert float(stats.kstest(us, "uniform").pvalue) < PM.KS_MIN


def test_annotprob_dirichlet_moments(O):
    """annotProb[l, present] ~ Dirichlet(1 + [a == annotCat[l]]): with three annotations the chosen one is Beta(2, 2), the others
    Beta(1, 3); with two, Beta(2, 1) and Beta(1, 2); a locus with one annotation gets exactly 1.  KS against those laws, and the mean."""
    n = 2000
    mask = np.ones((n, 3), dtype=int)
    mask[n // 2:, 1] = 0
    mask[-5:, 0] = 0                                   # five loci with annotation 3 only
    ann = np.where(np.arange(n) % 2 == 0, 0, 2)
    ann[-5:] = 2
    _, _, prob = RB.behind_sweep(O, SEED, 0, 1, 1, np.zeros(n), np.zeros(n, dtype=int), ann, mask, 4.0, 0.01, [0.0, 1.0], 3, False)
    assert np.array_equal(prob[-5:], np.tile([0.0, 0.0, 1.0], (5, 1))) and np.allclose(prob.sum(axis=1), 1.0, rtol=1e-15)
    assert np.all(prob[mask == 0] == 0.0)
    three, two = np.arange(n // 2), np.arange(n // 2, n - 5)
    chosen3, other3 = prob[three, ann[three]], prob[three, 1]
    chosen2 = prob[two, ann[two]]
    for x, law in ((chosen3, stats.beta(2, 2)), (other3, stats.beta(1, 3)), (chosen2, stats.beta(2, 1))):
        assert float(stats.kstest(x, law.cdf).pvalue) > PM.KS_MIN
    assert abs(chosen3.mean() - 0.5) < 4 * np.sqrt(0.05 / len(three)) and abs(chosen2.mean() - 2 / 3) < 4 * np.sqrt((1 / 18) / len(two))


def test_prior_constructor_and_refusals(ngp):
    from nextgp_jl_amd import api
    an = np.array([[1, 0], [1, 1], [0, 1]])
    p = api.BayesRCπ([0.9, 0.1], [0.0, 1.0], 0.05, an, estimatePi=True)
    assert p.annot.dtype == np.int32 and p.estimatePi and p.name == "BayesRCπ" and api.BayesRCpi is api.BayesRCπ
    assert {"BayesRCπ", "BayesRCplus", "BayesRCpi"} <= set(api.__all__) and ngp.BayesRCπ is api.BayesRCπ
    with pytest.raises(ValueError, match="no annotation"):
        api.BayesRCπ([0.9, 0.1], [0.0, 1.0], 0.05, [[1, 0], [0, 0]])
    with pytest.raises(ValueError, match="0 / 1"):
        api.BayesRCπ([0.9, 0.1], [0.0, 1.0], 0.05, [[1, 2]])
    with pytest.raises(ValueError, match="<= 16"):
        api.BayesRCπ([0.2] * 5, [0.0, 0.1, 0.2, 0.5, 1.0], 0.05, np.ones((4, 4), dtype=int))
    with pytest.raises(ValueError, match="<= 16"):
        api.BayesRCπ([0.5, 0.5], [0.0, 1.0], 0.05, np.ones((4, 9), dtype=int))
    with pytest.raises(NotImplementedError, match=r"src/functions\.jl:362-419"):
        api.BayesRCplus([0.9, 0.1], [0.0, 1.0], 0.05, an)


def test_file_headers(ngp, tmp_path):
    """pi<set>Out: pi1 .. pi(A K), annotation-major; annot<set>Out and delta<set>Out: the set's level names; var<set>Out: reg_1 .. reg_A."""
    from nextgp_jl_amd import api
    an = np.array([[1, 0, 1], [1, 1, 0], [0, 1, 1], [1, 1, 1]])
    prior = api.BayesRCπ([0.7, 0.2, 0.1], [0.0, 0.1, 1.0], 0.05, an)
    sets = [dict(id=0, name="M", members=["M"], cols=np.arange(4)[:, None], P=4, prior=prior, nreg=3, nvb=3, k=1, A=3)]
    api._write_headers(str(tmp_path), sets, ["intercept"])
    head = lambda n: open(os.path.join(str(tmp_path), n)).readline().rstrip("\n").split("\t")
    assert head("piMOut") == [f"pi{i}" for i in range(1, 10)] and head("varMOut") == ["reg_1", "reg_2", "reg_3"]
    assert head("annotMOut") == ["M1", "M2", "M3", "M4"] == head("deltaMOut") == head("betaMOut")


def test_binding_lists_the_new_entry_points(ngp):
    assert {"ngp_add_marker_set_rc", "ngp_get_rc_state", "ngp_set_rc_state"} <= set(ngp.SYMBOLS)
    hdr = open(os.path.join(ROOT, "include", "nextgp_hip.h")).read()
    assert "#define NGP_METHOD_BAYESRC 6" in hdr and re.search(r"int32_t ngp_abi_version\(void\);", hdr)
    rng_h = open(os.path.join(ROOT, "nextgp.jl_amd", "csrc", "ngp_rng.h")).read()
    assert "#define NGP_KIND_RC_UNIFORM 19" in rng_h and "#define NGP_KIND_RC_ANNOT 20" in rng_h


def test_julia_shim_serves_the_set():
    """Static, in the style of tests/test_julia_shim_static.py (which checks every ccall's types): the shim binds the three entry points,
    has the fine seam with the reference's argument list, routes "BayesRCπ" in the coarse seam and refuses "BayesRCplus"."""
    txt = open(os.path.join(ROOT, "nextgp.jl_amd", "julia", "NextGPHIP.jl")).read()
    for sym in ("ngp_add_marker_set_rc", "ngp_get_rc_state", "ngp_set_rc_state"):
        assert f"(:{sym}, LIB)" in txt
    assert re.search(r"function sampleBayesRCπ!\(h::Handle, set_id::Integer, mSet, M, beta, delta, ycorr::Vector\{Float64\}, varE::Float64, varBeta\)", txt)
    body = txt[txt.index("function sampleBayesRCπ!"):]
    body = body[:body.index("\nend\n")]
    # the reference's layout (src/mme.jl:391-403): piHat / logPi are vectors of A vectors, replaced entry by entry as src/functions.jl:355-356
    # does (the A entries start as ONE shared vector: an in-place write would alias them); annotCat is a 1 x P matrix
    assert "length(M[mSet].piHat), length(M[mSet].vClass)" in body and "size(M[mSet].piHat" not in body and "size(M[s].piHat" not in txt
    for pat in (r"M\[mSet\]\.piHat\[a\] = ", r"M\[mSet\]\.logPi\[a\] = log\.\(", r"M\[mSet\]\.annotProb \.= ", r"vec\(M\[mSet\]\.annotCat\) \.= "):
        assert re.search(pat, body), pat
    assert "reduce(vcat, x)" in txt and "Float64.(M[s].piHat[1])" in txt and "vec(M[s].annotCat) .= " in txt
    assert "annotInput" not in body                                     # never written (nor read: the library holds it)
    coarse = txt[txt.index("function runSampler!"):]
    assert 'M[s].method == "BayesRCπ"' in coarse and "add_marker_set_rc!" in coarse and 'annot$(s)Out' in coarse
    assert re.search(r'"BayesRCplus".*error\(', coarse)
    assert '"NGPSMP04"' in txt
