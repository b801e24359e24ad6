"""Convergence diagnostics on the device (include/nextgp_hip.h, "convergence diagnostics"; DESIGN.md section 2, "Convergence diagnostics"):
behind every kept iteration one element-wise pass updates a lag-window autocovariance of every monitored scalar; a finalising kernel
gives mean, variance, ESS and MCSE.  What is checked here is the arithmetic DESIGN.md fixes, restated in tests/ref_diag.py, bit for bit,
over the kept draws a sample file holds."""
import os

import numpy as np
import pytest

import ref_diag as RD
from conftest import add_sets
from test_gpu_compact import make_codes

pytestmark = pytest.mark.gpu

N, P = 96, 130
SPEC = [(0, 50, "PR"), (50, 40, "B"), (90, 40, "R")]
OUT = ("mean", "var", "sd", "ess", "mcse", "truncated", "half_n", "half_mean", "half_var")


def build(ngp, O, lags=8, split=0, sched=(40, 2, 1), classes=False, seed=1001, chain=0, diag=True, share=None, shards=None, y_shift=0.0):
    """PR + B (pi estimated) + R sets, one covariate, one (1|g) set; classes: the same model of a trait in three ordered classes (thr).
    D = 193 without and 195 with classes: odd, and no multiple of 64."""
    G, y, v = make_codes(O, N, P)
    s = ngp.Sampler(device=0, seed=seed, chain=chain)
    if shards:
        s.set_max_shards(shards)
    if share is not None:
        s.share_panel(share)
    else:
        s.set_panel(G, centre=True)
    s.add_fixed_set(np.linspace(-1, 1, N))
    q = 8 if classes else 7
    s.add_random_set(np.arange(N) % q, q, df=4.0, scale=1.0, varU0=2.0)
    add_sets(s, SPEC, v / float(y.var()) if classes else v)
    if classes:
        cuts = np.quantile(y, [1 / 3, 2 / 3])
        s.set_classes((1 + np.searchsorted(cuts, y)).astype(np.int32), 3)
        s.set_y(np.zeros(N)); s.set_residual_prior(4.0, 0.25)
    else:
        s.set_y(y + y_shift); s.set_residual_prior(4.0, 0.25 * y.var())
    s.set_schedule(*sched)
    if diag:
        s.enable_diagnostics(True, lags, split)
    return s


def same(got, want):
    return all(np.array_equal(got[k], want[k], equal_nan=True) for k in OUT) and got["n"] == want["n"]


def everything(s):
    st, ps, rr = s.get_state(), s.get_posterior_sums(), s.get_random(0)
    return [st[k] for k in ("ycorr", "beta", "delta", "varBeta", "piHat", "varE", "b", "iter")] + [ps[k] for k in sorted(ps)] + [rr[k] for k in sorted(rr)] + \
           [s.get_fixed()[k] for k in ("b", "sum_b")]


def same_everything(a, b):
    return all(np.array_equal(x, y) for x, y in zip(everything(a), everything(b)))


@pytest.mark.parametrize("lags,split,stops,classes", [(2, 0, (1, 2, 3, 40), False), (8, 5, (3, 8, 9, 100), False), (64, 1000, (10, 64, 65, 300), False),
                                                      (8, 3, (7, 8, 9, 33), True)])
def test_bit_for_bit_against_the_restatement(ngp, O, tmp_path, lags, split, stops, classes):
    """n < L, n = L, n = L + 1 and n >> L (the ring has wrapped many times) for L = 2, 8, 64; split 0, odd inside the run, beyond it; and a
    chain with three liability classes, whose record ends with thr.  The state image and every output equal the restatement run over the
    kept draws of the sample file."""
    s = build(ngp, O, lags=lags, split=split, sched=(stops[-1] + 2, 2, 1), classes=classes)
    D = s.diagnostics_layout()[0]
    assert D == (195 if classes else 193) and s.diagnostics_layout() == (D, lags, split, 0, (3 * lags + 5) * D)
    z = s.diagnostics()
    assert z["n"] == 0 and np.isnan(z["mean"]).all() and not s.diagnostics_state()["state"].any() and len(s.diagnostics_names()) == D
    path = str(tmp_path / "k.ngpsmp")
    s.set_sample_file(path)
    done = 0
    for n in stops:
        s.run(n + 2 - done)
        done = n + 2
        theta = RD.sample_theta(ngp.read_sample_file(path))
        assert theta.shape == (n, D)
        m = RD.run(theta, lags=lags, split=split)
        ds = s.diagnostics_state()
        assert ds["n"] == n and s.diagnostics_stats() == n
        assert np.array_equal(ds["state"], m.image())
        assert same(s.diagnostics(), m.finalise())
    s.set_sample_file(None)
    S = ngp.read_sample_file(path)
    q = 8 if classes else 7                                    # record order: varE | b | covariate | u[q] | varU | beta[P] | ...
    assert np.array_equal(theta[:, 0], S["varE"]) and np.array_equal(theta[:, 3:3 + q], S["u"][0]) and np.array_equal(theta[:, 4 + q:4 + q + P], S["beta"])
    if classes:
        assert np.array_equal(theta[:, -1:], S["thr"])
    f = s.diagnostics()
    assert np.all(f["ess"] <= f["n"]) and np.all(f["ess"] > 0) and np.isfinite(f["mean"]).all()


def test_only_kept_iterations_count_and_a_census_rerun_counts_once(ngp, O):
    sched = (20, 4, 2)
    s = build(ngp, O, sched=sched, split=4)
    s.run(5)                                                   # burn-in 4, thin 2: iteration 6 is the first kept one
    assert s.diagnostics_stats() == 0 and s.diagnostics()["n"] == 0 and not s.diagnostics_state()["state"].any()
    s.run(1)
    assert s.diagnostics_stats() == 1 and s.diagnostics()["n"] == 1
    one = s.diagnostics_state()["state"]
    s.run(1)                                                   # iteration 7: thinned out
    assert s.diagnostics_stats() == 1 and np.array_equal(s.diagnostics_state()["state"], one)
    s.run(13)
    ref = s.diagnostics_state()
    assert ref["n"] == 8 == s.get_posterior_sums()["nKept"] and s.diagnostics_stats() == 8
    d = build(ngp, O, sched=sched, split=4)
    d.debug_fail_census(9)                                     # the sweep of iteration 9 ends at its census once; 10 is a kept one
    d.run(20)
    got = d.diagnostics_state()
    assert got["n"] == 8 and d.diagnostics_stats() == 8 and np.array_equal(got["state"], ref["state"])
    assert same(d.diagnostics(), s.diagnostics())


def test_diagnostics_change_nothing(ngp, O, tmp_path):
    """Chain state, posterior sums and the bytes of the sample file are the same with the diagnostics on and off; off launches nothing."""
    files = []
    chains = []
    for on in (True, False):
        s = build(ngp, O, sched=(30, 4, 2), diag=on)
        files.append(str(tmp_path / f"s{int(on)}.ngpsmp"))
        s.set_sample_file(files[-1]); s.run(30); s.set_sample_file(None)
        chains.append(s)
    assert same_everything(*chains)
    assert open(files[0], "rb").read() == open(files[1], "rb").read() and os.path.getsize(files[0]) > 13 * 8 * 193
    assert chains[0].diagnostics_stats() == 13 and chains[1].diagnostics_stats() == 0
    with pytest.raises(ngp.NextGPHipError, match="no convergence diagnostics"):
        chains[1].diagnostics()
    chains[0].enable_diagnostics(False)
    chains[0].run(4)
    assert chains[0].diagnostics_stats() == 0


def test_set_y_zeroes_and_resume(ngp, O, tmp_path):
    """ngp_set_y zeroes the state; state image + snapshot into a fresh handle, then on: the uninterrupted run, bit for bit."""
    sched = (40, 4, 2)
    a = build(ngp, O, sched=sched, split=9)
    a.run(40)
    ref = a.diagnostics_state()
    assert ref["n"] == 18
    b = build(ngp, O, sched=sched, split=9)
    b.run(22)
    mid = b.diagnostics_state()
    assert mid["n"] == 9
    b.save_snapshot(str(tmp_path / "snap"))
    G, y, v = make_codes(O, N, P)
    b.set_y(y)
    z = b.diagnostics_state()
    assert z["n"] == 0 and not z["state"].any() and b.diagnostics()["n"] == 0
    c = build(ngp, O, sched=sched, split=9)
    c.load_snapshot(str(tmp_path / "snap"))
    c.set_diagnostics_state(mid)
    assert c.diagnostics_layout()[3] == 9
    c.run(18)
    got = c.diagnostics_state()
    assert got["n"] == 18 and np.array_equal(got["state"], ref["state"]) and same(c.diagnostics(), a.diagnostics())
    assert same_everything(a, c)


def test_refusals(ngp, O):
    E = ngp.NextGPHipError
    s = ngp.Sampler(device=0, seed=1, chain=0)
    with pytest.raises(E, match="-2|need a model"):
        s.enable_diagnostics(True)
    s = build(ngp, O, diag=False)
    for bad in (0, 1, 7, 258, -2):
        with pytest.raises(E, match="lags must be even"):
            s.enable_diagnostics(True, bad, 0)
    with pytest.raises(E, match="split must be >= 0"):
        s.enable_diagnostics(True, 8, -1)
    with pytest.raises(E, match="no convergence diagnostics"):
        s.diagnostics_layout()
    s.enable_diagnostics(True, 4, 2)
    D, L, H, n, w = s.diagnostics_layout()
    assert (D, L, H, n, w) == (193, 4, 2, 0, 17 * 193)
    with pytest.raises(E, match="D = 193"):
        s._chk(s.L.ngp_get_diagnostics(s.h, None, None, None, None, None, None, None, None, 192, None))
    with pytest.raises(E, match="words"):
        s.set_diagnostics_state(dict(state=np.zeros(5), n=0))
    s.run(10)
    assert s.diagnostics()["n"] == 8
    s.add_fixed_set((np.arange(N) % 3).astype(np.float64))     # the model changes while draws are held: D would change
    with pytest.raises(E, match="model changed"):
        s.run(2)
    s.enable_diagnostics(True, 4, 2)                           # enabling again takes the new model
    assert s.diagnostics_layout()[0] == 194


def test_fused_chains_equal_chains_alone(ngp, O):
    """Four chains of one ngp_run_many: every chain launches its own update, and its state is bit for bit what it holds alone."""
    K, sched = 4, (24, 4, 2)
    first = ngp.Sampler(device=0, seed=1001, chain=0)
    ms = first.shards_for_pass(K)
    first.close()
    chains = [build(ngp, O, sched=sched, split=5, chain=0, shards=ms)]
    for c in range(1, K):
        chains.append(build(ngp, O, sched=sched, split=5, chain=c, share=chains[0], y_shift=0.01 * c))
    ngp.Sampler.run_many(chains, 24)
    for c in range(K):
        alone = build(ngp, O, sched=sched, split=5, chain=c, shards=ms, y_shift=0.01 * c)
        alone.run(24)
        a, f = alone.diagnostics_state(), chains[c].diagnostics_state()
        assert a["n"] == f["n"] == 10 and chains[c].diagnostics_stats() == 10
        assert np.array_equal(a["state"], f["state"]) and same(alone.diagnostics(), chains[c].diagnostics())
    assert not np.array_equal(chains[0].diagnostics_state()["state"], chains[1].diagnostics_state()["state"])


def lmem(ngp, problem, tmp_path, name, herd=False, **kw):
    """M1 BayesPR, M2 BayesC with pi estimated; herd: a (1|herd) term beside them and M2 BayesR instead."""
    G, y, v = problem
    np.save(tmp_path / "a.npy", G[:, :70]); np.save(tmp_path / "b.npy", G[:, 70:])
    f = f'y ~ 1 + {"(1|herd) + " if herd else ""}SNP(M1,"{tmp_path / "a.npy"}") + SNP(M2,"{tmp_path / "b.npy"}")'
    m2 = ngp.BayesR([0.85, 0.10, 0.04, 0.01], [0.0, 0.01, 0.1, 1.0], v, estimatePi=True) if herd else ngp.BayesC(0.1, v, estimatePi=True)
    vc = {"M1": ngp.BayesPR(9999, v), "M2": m2, "e": ngp.Random("I", 0.25 * y.var())}
    data = {"y": y}
    if herd:
        data["herd"] = np.array([f"h{i % 5}" for i in range(N)]); vc["1|herd"] = ngp.Random("I", 0.5)
    out = tmp_path / name
    return ngp.runLMEM(f, data, 44, 4, 2, VCV=vc, outFolder=str(out), seed=7, **kw), out


def stems_checked(folder, names):
    """Every *Out file of the folder that a name's stem points at has that stem's column headers, in order, as its header row."""
    checked = set()
    for stem in dict.fromkeys(nm.split(":", 1)[0] for nm in names):
        f = folder / f"{stem}Out"
        if f.exists():
            assert open(f).readline().rstrip("\n").split("\t") == [nm.split(":", 1)[1] for nm in names if nm.split(":", 1)[0] == stem], stem
            checked.add(stem)
    return checked


def test_runlmem_diagnostics_end_to_end(ngp, O, tmp_path):
    """runLMEM(chains=4, diagnostics=True): the pooled result is pool_diagnostics of the chains', convergence.txt round-trips, the names
    line up with the headers of the *Out files; diagnostics={"lags": 8} on one chain, and convergencyMCMC over its folder; a model with
    a (1|herd) term and a BayesR set for the names of u, varU and the class probabilities."""
    problem = make_codes(O, N, P)
    res, out = lmem(ngp, problem, tmp_path, "four", chains=4, diagnostics=True)
    dg = res["diagnostics"]
    D = len(dg["names"])
    assert len(dg["chains"]) == 4 and all(c["n"] == 20 and np.array_equal(c["half_n"], [10.0, 10.0]) for c in dg["chains"]) and dg["n"] == 80
    pooled = ngp.pool_diagnostics(dg["chains"])
    assert all(np.array_equal(dg[k], pooled[k], equal_nan=True) for k in ("mean", "sd", "mcse", "ess", "rhat", "truncated"))
    assert len(set(dg["names"])) == D and len(dg["worst"]["ess"]) == 10 and set(dg["worst"]["ess"]) <= set(dg["names"])
    assert np.isfinite(dg["rhat"][dg["names"].index("varE:e")]) and dg["ess"][dg["names"].index("varE:e")] <= 80
    cv = ngp.read_convergence_file(str(out / "convergence.txt"))
    assert cv["names"] == dg["names"] and all(np.array_equal(cv[k], dg[k], equal_nan=True) for k in ("mean", "sd", "mcse", "ess", "rhat", "truncated"))
    # the pooled mean is the posterior mean the sums give
    assert np.allclose(dg["mean"][dg["names"].index("varE:e")], res["varE"], rtol=1e-12, atol=0)
    assert {"varE", "b", "betaM1", "betaM2", "varM1", "varM2", "piM2"} <= stems_checked(out / "chain0", dg["names"])
    # one chain, a window of 8 lags
    one, out1 = lmem(ngp, problem, tmp_path, "one", diagnostics={"lags": 8})
    d1 = one["diagnostics"]
    assert d1["n"] == 20 and len(d1["chains"]) == 1 and d1["names"] == dg["names"]
    assert {"varE", "b", "betaM1", "betaM2", "varM1", "varM2", "piM2"} <= stems_checked(out1, d1["names"])
    assert np.array_equal(d1["ess"], d1["chains"][0]["ess"]) and np.isfinite(d1["rhat"][0])
    mean, rows = ngp.convergencyMCMC("betaM2", summary=True, outFolder=str(out1))
    assert rows["names"] == [f"M{j + 1}" for j in range(60)] and mean.shape == (1, 60)
    assert np.allclose(rows["mean"], mean[0], rtol=1e-9, atol=1e-300) and np.array_equal(ngp.convergencyMCMC("betaM2", outFolder=str(out1)), mean)
    assert np.allclose(rows["mean"], one["sets"]["M2"]["beta"], rtol=1e-9, atol=1e-300)
    # a (1|herd) term and a BayesR set: u in level order, varU, the class probabilities; piHat of a set that writes none has no file
    rnd, out2 = lmem(ngp, problem, tmp_path, "herd", herd=True, diagnostics={"lags": 8})
    d2 = rnd["diagnostics"]
    assert len(set(d2["names"])) == len(d2["names"]) == len(d2["mean"]) == len(d1["names"]) + 5 + 1 + 4
    assert {"varE", "b", "u1 | herd", "varU1 | herd", "betaM1", "betaM2", "varM1", "varM2", "piM2"} <= stems_checked(out2, d2["names"])
    assert [nm for nm in d2["names"] if nm.startswith("piM2:")] == ["piM2:pi1", "piM2:pi2", "piM2:pi3", "piM2:pi4"]
    for param, want in (("u1 | herd", rnd["random"]["1 | herd"]["u"]), ("piM2", rnd["sets"]["M2"]["pi"]), ("varU1 | herd", [rnd["random"]["1 | herd"]["varU"]])):
        mean, rows = ngp.convergencyMCMC(param, summary=True, outFolder=str(out2))
        assert np.allclose(rows["mean"], mean[0], rtol=1e-9, atol=1e-300) and np.allclose(rows["mean"], want, rtol=1e-9, atol=1e-300), param
