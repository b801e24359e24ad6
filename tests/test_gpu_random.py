"""(1|g) random-effect sets on the device (sampleZ! / sampleVarU, src/functions.jl:57-72, 92-97, 498-501).  Yardsticks: the blocked
restatement of the device's documented order (bit for bit) and the reference's order (RandomRefChain, to 1e-9 relative), both in
tests/ref_random.py."""
import os

import numpy as np
import pytest

import ref_random as RR
from conftest import add_sets, make_problem

pytestmark = pytest.mark.gpu


def _ped_K(q, seed=0):
    """A pedigree-like sparse precision: A^-1 of a random pedigree (Henderson's rules, parents before progeny)."""
    rng = np.random.default_rng(seed)
    K = np.zeros((q, q))
    for i in range(q):
        if i >= 4 and rng.random() < 0.8:
            s_, d_ = (int(x) for x in rng.choice(i, 2, replace=False))
            idx, c = [i, s_, d_], 2.0
            w = np.array([1.0, -0.5, -0.5])
        else:
            idx, c, w = [i], 1.0, np.array([1.0])
        K[np.ix_(idx, idx)] += c * np.outer(w, w)
    return K


def _Ks(q):
    rng = np.random.default_rng(9)
    A = rng.normal(size=(q, q))
    S = A @ A.T + q * np.eye(q)
    dense = np.linalg.inv(S)
    dense = (dense + dense.T) / 2
    return dict(identity=None, diagonal=np.diag(rng.uniform(0.5, 2.0, q)), pedigree=_ped_K(q), dense=dense)


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("kname", ["identity", "diagonal", "pedigree", "dense"])
def test_fine_seam_bit_exact_vs_blocked_restatement(ngp, O, kname, weighted):
    N, P, q = 300, 128, 23
    X, y, _, v = make_problem(O, N, P, seed=2)
    rng = np.random.default_rng(4)
    level = rng.integers(0, q - 2, size=N)                      # two levels without records
    w = rng.uniform(0.3, 3.0, N) if weighted else None
    K = _Ks(q)[kname]
    s = ngp.Sampler(device=0, seed=77, chain=2)
    if weighted:
        s.set_residual_weights(w)
    s.set_panel(X)
    rid = s.add_random_set(level, q, K=K, df=4.0, scale=0.4, varU0=0.8)
    s.add_random_set(rng.integers(0, 5, size=N), 5)             # a second set: keys carry the set id
    ycorr = y - y.mean()
    u = rng.normal(size=q)
    rs = np.sqrt(w) if weighted else None
    zpz = RR.zpz_of(level, q, w)
    varU = 0.8
    for it in (1, 2):                                           # the set's own call counter is the iteration of its draws
        yt_in = ycorr * rs if weighted else ycorr               # the device's residual: y~ = s ycorr under weights
        yt, u_ref, v_ref = RR.random_step_blocked(O, 77, 2, it, rid, yt_in, None if rs is None else list(rs), level, q, K, zpz, u, varU,
                                                  1.3, 4.0, 0.4)
        y_ref = np.array(yt) / rs if weighted else np.array(yt)
        varU = s.sample_random_set(rid, 1.3, ycorr, u, varU)   # ycorr, u updated in place
        assert np.array_equal(u, np.array(u_ref)), it
        assert varU == v_ref, it
        assert np.array_equal(ycorr, y_ref), it


SPEC = [(0, 192, "PR"), (192, 128, "B"), (320, 128, "R")]


def _random_problem(O, N=300, P=448, qh=12, seed=3, herd_sd=3.0):
    X, y, _, v = make_problem(O, N, P, seed=seed)
    rng = np.random.default_rng(seed + 50)
    herd = rng.integers(0, qh, size=N)
    uh = rng.normal(size=qh) * herd_sd * np.sqrt(y.var())
    y = y + uh[herd]
    qa = 40
    animal = rng.integers(0, qa, size=N)
    return X, y, v, herd, qh, animal, qa, uh


def test_chain_vs_reference_order(ngp, O):
    X, y, v, herd, qh, animal, qa, _ = _random_problem(O)
    Ka = _ped_K(qa, seed=3)
    s = ngp.Sampler(device=0, seed=31, chain=1)
    s.set_panel(X)
    ref = RR.RandomRefChain(O, X.astype(np.float64), y, seed=31, chain=1)
    ref.add_marker_set, ref.add_marker_set_r = ref.add_set, ref.add_set_r
    s.add_random_set(herd, qh, df=4.0, scale=1.0, varU0=2.0)
    s.add_random_set(animal, qa, K=Ka, df=4.0, scale=0.5, varU0=1.0)
    ref.add_random(herd, qh, None, df=4.0, scale=1.0, v=2.0)
    ref.add_random(animal, qa, Ka, df=4.0, scale=0.5, v=1.0)
    add_sets(s, SPEC, v); add_sets(ref, SPEC, v)
    s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var())
    ref.E_df, ref.E_scale = 4.0, 0.25 * y.var()
    tol = lambda a, b: np.abs(np.asarray(a) - np.asarray(b)).max() <= 1e-9 * max(1e-6, np.abs(np.asarray(b)).max())
    for it in range(4):
        s.run(1); ref.run(1)
        a, b = s.get_state(), ref.state()
        assert np.array_equal(a["delta"], b["delta"]), it
        for k in ("beta", "ycorr", "varBeta"):
            assert tol(a[k], b[k]), (it, k)
        for r in range(2):
            g = s.get_random(r)
            assert tol(g["u"], ref.u[r]), (it, r)
            assert abs(g["varU"] - ref.varU[r]) <= 1e-9 * ref.varU[r], (it, r)
        assert abs(a["varE"] - b["varE"]) <= 1e-9 * b["varE"]


def _full(ngp, X, y, v, herd, qh, animal, qa, seed, chain, w=None, share=None, max_shards=None):
    s = ngp.Sampler(device=0, seed=seed, chain=chain)
    if w is not None:
        s.set_residual_weights(w)
    if max_shards:
        s.set_max_shards(max_shards)
    if share is not None:
        s.share_panel(share)
    else:
        s.set_panel(X)
    s.add_fixed_set(np.linspace(-1, 1, len(y)))
    s.add_random_set(herd, qh, df=4.0, scale=1.0, varU0=2.0)
    s.add_random_set(animal, qa, K=_ped_K(qa, seed=3), df=4.0, scale=0.5, varU0=1.0)
    add_sets(s, SPEC, v)
    s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var()); s.set_schedule(12, 2, 2)
    return s


def _consistent(s, y, herd, animal):
    st = s.get_state()
    fx = s.get_fixed()["b"]
    u0, u1 = s.get_random(0)["u"], s.get_random(1)["u"]
    xf = np.linspace(-1, 1, len(y)) * fx[0]
    exp = y - st["b"] - xf - u0[herd] - u1[animal] - s.xbeta(st["beta"])
    assert np.abs(st["ycorr"] - exp).max() <= 1e-9 * np.abs(y).max()


@pytest.mark.parametrize("variant", ["fp32", "weighted", "u8"])
def test_state_holds_together(ngp, O, variant):
    X, y, v, herd, qh, animal, qa, _ = _random_problem(O, herd_sd=20.0)   # herd effects large against sqrt(varE): the range contract
    kw = {}
    if variant == "weighted":
        kw["w"] = np.random.default_rng(1).uniform(0.3, 3.0, len(y))
    if variant == "u8":
        G = np.rint(X.astype(np.float64) - X.min(axis=0)).astype(np.uint8)
        s = ngp.Sampler(device=0, seed=5, chain=0, storage=1)
        s.set_panel(np.asfortranarray(G), centre=True)
        s.add_fixed_set(np.linspace(-1, 1, len(y)))
        s.add_random_set(herd, qh, df=4.0, scale=1.0, varU0=2.0)
        s.add_random_set(animal, qa, K=_ped_K(qa, seed=3), df=4.0, scale=0.5, varU0=1.0)
        add_sets(s, SPEC, v)
        s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var()); s.set_schedule(12, 2, 2)
    else:
        s = _full(ngp, X, y, v, herd, qh, animal, qa, 5, 0, **kw)
    s.run(12)
    _consistent(s, y, herd, animal)


def _everything(s):
    st, ps = s.get_state(), s.get_posterior_sums()
    rr = [s.get_random(r) for r in range(2)]
    return st, ps, rr


def _same(a, b):
    (sa, pa, ra), (sb, pb, rb) = a, b
    for k in ("ycorr", "beta", "delta", "varBeta", "piHat"):
        assert np.array_equal(sa[k], sb[k]), k
    assert sa["varE"] == sb["varE"] and sa["b"] == sb["b"]
    for k in ("sum_beta", "sum_varBeta", "sum_pi"):
        assert np.array_equal(pa[k], pb[k]), k
    for x, z in zip(ra, rb):
        assert np.array_equal(x["u"], z["u"]) and np.array_equal(x["sum_u"], z["sum_u"])
        assert x["varU"] == z["varU"] and x["sum_varU"] == z["sum_varU"]


def test_run_many_equals_chains_alone(ngp, O):
    X, y, v, herd, qh, animal, qa, _ = _random_problem(O)
    K = 3
    first = ngp.Sampler(device=0, seed=11, chain=0)
    ms = first.shards_for_pass(K)
    first.close()
    chains = [_full(ngp, X, y, v, herd, qh, animal, qa, 11, 0, max_shards=ms)]
    for c in range(1, K):
        chains.append(_full(ngp, X, y + 0.01 * c, v, herd, qh, animal, qa, 11, c, max_shards=ms, share=chains[0]))
    ngp.Sampler.run_many(chains, 12)
    for c in range(K):
        alone = _full(ngp, X, y + 0.01 * c, v, herd, qh, animal, qa, 11, c, max_shards=ms)
        alone.run(12)
        _same(_everything(chains[c]), _everything(alone))


def test_snapshot_resume_and_sample_file(ngp, O, tmp_path):
    X, y, v, herd, qh, animal, qa, _ = _random_problem(O)
    a = _full(ngp, X, y, v, herd, qh, animal, qa, 21, 0)
    a.set_sample_file(str(tmp_path / "s.ngpsmp"))
    a.run(12)
    a.set_sample_file(None)
    S = ngp.read_sample_file(str(tmp_path / "s.ngpsmp"))
    last = a.get_random(0), a.get_random(1)
    assert len(S["u"]) == 2 and S["u"][0].shape == (5, qh) and S["varU"].shape == (5, 2)   # kept: 4, 6, 8, 10, 12
    assert np.array_equal(S["u"][0][-1], last[0]["u"]) and np.array_equal(S["u"][1][-1], last[1]["u"])
    assert S["varU"][-1, 0] == last[0]["varU"] and np.allclose(S["u"][0].sum(axis=0), last[0]["sum_u"], rtol=1e-12, atol=1e-12)
    assert np.array_equal(S["beta"][-1], a.get_state()["beta"])
    b = _full(ngp, X, y, v, herd, qh, animal, qa, 21, 0)
    b.run(5)
    b.save_snapshot(str(tmp_path / "snap"))
    c = _full(ngp, X, y, v, herd, qh, animal, qa, 21, 0)
    c.load_snapshot(str(tmp_path / "snap"))
    c.run(7)
    _same(_everything(a), _everything(c))
    d = _full(ngp, X, y, v, herd, qh, animal, qa, 21, 0)
    d.run(12)
    _same(_everything(a), _everything(d))
    e = ngp.Sampler(device=0, seed=21, chain=0)                 # a model with other random sets is refused
    e.set_panel(X); e.add_fixed_set(np.linspace(-1, 1, len(y)))
    e.add_random_set(herd, qh, df=4.0, scale=1.0, varU0=2.0)
    e.add_random_set(animal, qa, df=4.0, scale=0.5, varU0=1.0)  # identity instead of the pedigree K
    add_sets(e, SPEC, v); e.set_y(y)
    with pytest.raises(ngp.NextGPHipError, match="random-effect sets differ"):
        e.load_snapshot(str(tmp_path / "snap"))
    e.run(2)
    ncls = len(a.get_class_state(2)["piHat"])                   # the BayesR set's classes
    assert a.posterior_len() == 3 * 448 + a.nvb + 2 * 3 + ncls + 1 + (qh + qa + 2) + 3   # + sums of u and of varU


def test_refusals_leave_a_handle_that_runs(ngp, O):
    X, y, v, herd, qh, *_ = _random_problem(O)
    s = ngp.Sampler(device=0, seed=3, chain=0)
    s.set_panel(X)
    bad = herd.copy(); bad[5] = qh
    K = _ped_K(qh)
    Kns = K.copy(); Kns[0, 5] += 0.25
    Knd = K.copy(); Knd[3, 3] = 0.0
    Knf = K.copy(); Knf[2, 2] = np.nan
    for args, kw in (((bad, qh), {}), ((herd, qh), dict(K=Kns)), ((herd, qh), dict(K=Knd)), ((herd, qh), dict(K=Knf)),
                     ((herd, qh), dict(varU0=-1.0))):
        with pytest.raises(ngp.NextGPHipError):
            s.add_random_set(*args, **kw)
        s.rand_q = []
    rid = s.add_random_set(herd, qh, K=K, varU0=1.0)
    add_sets(s, SPEC, v); s.set_y(y); s.set_residual_prior(4.0, 1.0); s.run(3)
    assert np.all(np.isfinite(s.get_random(rid)["u"]))
    with pytest.raises(ngp.NextGPHipError):
        s.sample_random_set(rid, -1.0, y.copy(), np.zeros(qh), 1.0)
    s.run(1)


def test_runLMEM_writes_reference_files_and_recovers_herd_effects(ngp, O, tmp_path):
    from nextgp_jl_amd import api
    N, P, qh = 600, 256, 15
    X, y, _, v = make_problem(O, N, P, seed=8)
    rng = np.random.default_rng(8)
    herd_names = np.array([f"h{k:02d}" for k in rng.permutation(qh)])
    herd = herd_names[rng.integers(0, qh, size=N)]
    uh = {h: rng.normal() * 2.0 * np.sqrt(y.var()) for h in herd_names}
    y = y + np.array([uh[h] for h in herd])
    geno = str(tmp_path / "geno.npy")
    np.save(geno, X.astype(np.float64))
    data = dict(y=y, herd=herd)
    for K, sub in ((1, "one"), (4, "four")):
        out = str(tmp_path / sub)
        res = api.runLMEM(f'y ~ 1 + (1|herd) + SNP(M, "{geno}")', data, 60, 20, 2, outFolder=out,
                          VCV={"1|herd": api.Random("I", 1.0), "M": api.BayesPR(9999, v)}, chains=K)
        folder = out if K == 1 else os.path.join(out, "chain0")
        with open(os.path.join(folder, "u1 | herdOut")) as f:
            hdr = f.readline().rstrip("\n").split("\t")
        assert hdr == sorted(set(herd.tolist()))
        with open(os.path.join(folder, "varU1 | herdOut")) as f:
            assert f.readline().rstrip("\n") == "1herd"
        um = api.summaryMCMC("u1 | herd", outFolder=folder)[0]
        rr = res["random"]["1 | herd"] if K == 1 else res["chains"][0]["random"]["1 | herd"]
        assert np.allclose(um, rr["u"], rtol=1e-12, atol=1e-12)
        truth = np.array([uh[h] for h in rr["levels"]])
        assert np.corrcoef(res["random"]["1 | herd"]["u"], truth)[0, 1] > 0.95
        assert res["random"]["1 | herd"]["varU"] > 0
