"""BayesLV marker sets on the device (sampleBayesLV!, src/functions.jl:421-486).  Yardsticks: the blocked restatement of the device's
documented order of the variance step (bit for bit), a BayesPR set with one region per locus (the sweep, bit for bit) and the
reference's order (LVRefChain, to 1e-9 relative), the restatements in tests/ref_logvar.py."""
import math
import os

import numpy as np
import pytest

import ref_logvar as RL
from conftest import make_problem
from test_logvar_host import _inputs

pytestmark = pytest.mark.gpu


def test_det_exp_any_bit_exact(ngp, O):
    s = ngp.Sampler(device=0, seed=1, chain=0)
    rng = np.random.default_rng(0)
    mags = np.exp(rng.uniform(math.log(1e-300), math.log(720.0), 20000))
    x = np.concatenate([mags, -mags, [0.0, -0.0, -708.0, -708.5, -709.0, -745.2, -1e4, 708.0, 709.0, 709.5, 710.0, 1e4, math.inf, -math.inf, math.nan]])
    got = s.eval_math(4, x)
    exp = np.array([RL.det_exp_any(O, float(v)) for v in x])
    assert np.array_equal(got, exp, equal_nan=True)
    assert got[len(x) - 1] != got[len(x) - 1] and got[2 * len(mags)] == 1.0 and got[2 * len(mags) + 1] == 1.0


def _lv_sampler(ngp, O, P, C, vb0, varZeta0, mode, frac, zeta0, seed=21, chain=1, N=48, lhs0=None, rhs0=None, col0=0, extra=0):
    X, _ = O.generate_panel(N, P + extra, seed=5)
    s = ngp.Sampler(device=0, seed=seed, chain=chain)
    s.set_panel(X)
    if extra:
        s.add_marker_set(0, extra, 0, 4.0, 0.01, [(0, extra)], [0.02])
    sid = s.add_marker_set_lv(col0 + extra, P, vb0, C, varZeta0, est_mode=mode, est_fraction=frac, zeta0=zeta0, lhs0=lhs0, rhs0=rhs0)
    return s, sid, X


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["fixed", "var_zeta", "fraction"])
@pytest.mark.parametrize("ncov", [1, 3, 16])
@pytest.mark.parametrize("P", [64, 1000, 4099])
def test_fine_seam_variance_step_bit_exact(ngp, O, P, ncov, mode):
    """ngp_sweep_set on a BayesLV set = the sweep, then the variance step on the effects the sweep has left.  Summary-statistic terms pin
    those effects: an infinite lhs0 gives exactly 0, a large one with rhs0 = lhs0 * b an effect next to b (here |b| = 40 and 20 sd)."""
    C, vb, _, zeta = _inputs(P, ncov, 100 + P + ncov)
    lhs0 = np.zeros(P); rhs0 = np.zeros(P)
    big = np.arange(3, P, 11)
    zero = np.setdiff1d(np.arange(0, P, 7), big)
    lhs0[zero] = np.inf
    lhs0[big] = 1e12
    rhs0[big] = 1e12 * np.sqrt(vb[big]) * np.where(np.arange(len(big)) % 2 == 0, 40.0, -20.0)   # b^2 / (2 var) = 800: exp underflows; 200
    for given in (True, False):
        s, sid, X = _lv_sampler(ngp, O, P, C, 0.01, 0.7, mode, 0.3, zeta if given else None, lhs0=lhs0, rhs0=rhs0, extra=64)
        assert sid == 1
        st0 = s.lv_state(sid)
        z_in = zeta if given else RL.zeta_start(O, 21, 1, sid, P)
        assert np.array_equal(st0["zeta"], z_in) and st0["varZeta"] == 0.7 and np.all(st0["c"] == 0.0)
        assert np.allclose(st0["iCpC"], RL.icpc(C), rtol=1e-9, atol=0)
        rng = np.random.default_rng(3)
        ycorr = rng.normal(size=X.shape[0])
        beta = np.zeros(P)
        v = vb.copy()
        varZeta = 0.7
        for it in (1, 2):                                           # the set's own call counter keys the draws
            v_in = v.copy()
            s.sweep_set(sid, 1.1, ycorr, beta, v)
            if it == 1:
                assert np.all(beta[zero] == 0.0) and np.all(np.abs(beta[big]) > 19.0 * np.sqrt(vb[big]))
            v_ref, c_ref, z_ref, vz_ref, tr_ref = RL.lv_step_blocked(O, 21, 1, it, sid, beta, v_in, z_in, C, st0["iCpC"], varZeta, mode, 0.3)
            st = s.lv_state(sid)
            assert np.array_equal(v, v_ref), (given, it)
            assert np.array_equal(st["c"], c_ref) and np.array_equal(st["zeta"], z_ref), (given, it)
            assert st["varZeta"] == vz_ref and st["trapped"] == tr_ref, (given, it, st["varZeta"], vz_ref, st["trapped"], tr_ref)
            z_in, varZeta = z_ref, vz_ref


SWEEP_ENGINES = [(0, 1), (1, 1), (1, 2), (1, 3), (1, 4), (1, 6), (1, 8), (1, 5, 4), (1, 8, 4), (1, 3, 3, 2), (1, 4, 3, 2), (1, 5, 4, 2), (1, 6, 4, 2),
                 (1, 8, 2), (1, 6, 2, 2), (1, 6, 1, 2), (1, 8, 1)]    # tests/test_gpu_parity.py's engine list


def _identity(ngp, mk, X, y, P0, Pl, vbl, rng_seed=6):
    """The same fine-seam call on an LV set and on a BayesPR set with one region per locus: beta, delta, ycorr bit for bit."""
    out = []
    C = np.column_stack([np.ones(Pl), np.arange(Pl) % 2])
    for kind in ("lv", "pr"):
        s = mk()
        s.add_marker_set(0, P0, 1, 4.0, 0.01, [(j, j + 1) for j in range(P0)], [0.02] * P0, pi0=0.3)
        if kind == "lv":
            sid = s.add_marker_set_lv(P0, Pl, 0.01, C, 0.5, est_mode=1)
        else:
            sid = s.add_marker_set(P0, Pl, 0, 4.0, 0.005, [(j, j + 1) for j in range(Pl)], [0.01] * Pl)
        rng = np.random.default_rng(rng_seed)
        ycorr = y - y.mean()
        beta = rng.normal(size=Pl) * 0.05
        v = vbl.copy()
        delta = s.sweep_set(sid, 1.3, ycorr, beta, v)
        out.append((beta, delta, ycorr))
    for a, b in zip(*out):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("form", [0, 1], ids=["chain64", "tinv"])
@pytest.mark.parametrize("engine", SWEEP_ENGINES, ids=[str(e) for e in SWEEP_ENGINES])
def test_sweep_is_the_bayespr_sweep(ngp, O, engine, form):
    N, P0, Pl = 300, 64, 200
    X, y, _, _ = make_problem(O, N, P0 + Pl, seed=2)
    vbl = np.exp(np.random.default_rng(1).normal(-4.5, 1.0, Pl))

    def mk():
        s = ngp.Sampler(device=0, seed=9, chain=2, mode=engine[0], lag=engine[1], streamer=engine[3] if len(engine) > 3 else 1)
        s.set_chain_form(form)
        if len(engine) > 2:
            s.set_near(engine[2])
        s.set_panel(X)
        return s
    _identity(ngp, mk, X, y, P0, Pl, vbl)


@pytest.mark.parametrize("variant", ["compact", "weighted"])
def test_sweep_identity_compact_and_weighted(ngp, O, variant):
    N, P0, Pl = 300, 64, 200
    X, y, _, _ = make_problem(O, N, P0 + Pl, seed=2)
    vbl = np.exp(np.random.default_rng(1).normal(-4.5, 1.0, Pl))
    G = np.asfortranarray(np.rint(X.astype(np.float64) - X.min(axis=0)).astype(np.uint8))
    w = np.random.default_rng(8).uniform(0.3, 3.0, N)

    def mk():
        if variant == "compact":
            s = ngp.Sampler(device=0, seed=9, chain=2, storage=1)
            s.set_panel(G, centre=True)
        else:
            s = ngp.Sampler(device=0, seed=9, chain=2)
            s.set_residual_weights(w)
            s.set_panel(X)
        return s
    _identity(ngp, mk, X, y, P0, Pl, vbl)


def _chain_problem(O, N=300, Pl=192, Pp=128, seed=4):
    X, y, _, v = make_problem(O, N, Pl + Pp, seed=seed)
    rng = np.random.default_rng(seed + 1)
    a = rng.integers(0, 2, Pl).astype(float)
    bt = rng.normal(size=Pl) * np.where(a == 1, 0.5, 0.05)
    y = y + X[:, :Pl].astype(np.float64) @ bt
    C = np.column_stack([np.ones(Pl), a])
    return X, y, v, C, np.linspace(-1, 1, N)


def _full(ngp, X, y, v, C, cov, seed, chain, est=1, share=None, max_shards=None, with_r=False, storage=None):
    s = ngp.Sampler(device=0, seed=seed, chain=chain)
    if max_shards:
        s.set_max_shards(max_shards)
    if share is not None:
        s.share_panel(share)
    else:
        s.set_panel(X)
    Pl = C.shape[0]
    s.add_fixed_set(cov)
    s.add_marker_set_lv(0, Pl, v, C, 0.5, est_mode=est)
    Pp = X.shape[1] - Pl
    if with_r:
        s.add_marker_set_r(Pl, Pp, 4.0, v * 0.5, v, [0.0, 0.01, 0.1, 1.0], [0.85, 0.10, 0.04, 0.01], estPi=True)
    else:
        s.add_marker_set(Pl, Pp, 0, 4.0, v * 0.5, [(0, Pp)], [v])
    s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var()); s.set_schedule(12, 2, 2)
    return s


def test_chain_vs_reference_order(ngp, O):
    """An intercept, one covariate, a BayesLV set (varZeta estimated) and a BayesPR set, 30 iterations, against LVRefChain at the project's
    tolerance for reference-order comparisons (1e-9 relative, tests/test_gpu_random.py::test_chain_vs_reference_order).  Two reference-
    order chains that differ only in the rounding of the variance step stay within 7.9e-15 of each other over 30 iterations
    (tests/test_logvar_host.py::test_variance_step_chains_differ_by_rounding_only): the slice step does not amplify rounding, so the
    bound stays 1e-9."""
    X, y, v, C, cov = _chain_problem(O)
    s = _full(ngp, X, y, v, C, cov, 31, 1)
    ref = RL.LVRefChain(O, X.astype(np.float64), y, seed=31, chain=1)
    ref.add_fixed(cov)
    ref.add_set_lv(0, C.shape[0], v, C, 0.5, est=True)
    Pp = X.shape[1] - C.shape[0]
    ref.add_set(C.shape[0], Pp, 0, 4.0, v * 0.5, [(0, Pp)], [v])
    ref.E_df, ref.E_scale = 4.0, 0.25 * y.var()
    gap = lambda a, b: np.abs(np.asarray(a) - np.asarray(b)).max() / max(1e-6, np.abs(np.asarray(b)).max())
    worst = {}
    for it in range(30):
        s.run(1); ref.run(1)
        a, b, lv = s.get_state(), ref.state(), s.lv_state(0)
        g = dict(beta=gap(a["beta"], b["beta"]), ycorr=gap(a["ycorr"], b["ycorr"]), varBeta=gap(a["varBeta"], b["varBeta"]),
                 c=gap(lv["c"], ref.M[0]["c"]), zeta=gap(lv["zeta"], ref.M[0]["SNPVARRESID"]), varZeta=abs(lv["varZeta"] / ref.M[0]["varZeta"][0] - 1),
                 varE=abs(a["varE"] / b["varE"] - 1))
        for k, x in g.items():
            worst[k] = max(worst.get(k, 0.0), x)
        assert lv["trapped"] == ref.M[0]["trapped"], it
    print("chain against reference order, largest relative gaps over 30 iterations:", worst)
    for k, x in worst.items():
        assert x <= 1e-9, (k, x)
    assert np.array_equal(a["piHat"], b["piHat"])                  # the [0.5, 0.5] placeholder of a set without pi


def _everything(s):
    return s.get_state(), s.get_posterior_sums(), s.lv_state(1 - 1)


def _same(a, b):
    (sa, pa, la), (sb, pb, lb) = a, b
    for k in ("ycorr", "beta", "delta", "varBeta", "piHat"):
        assert np.array_equal(sa[k], sb[k]), k
    assert sa["varE"] == sb["varE"] and sa["b"] == sb["b"]
    for k in ("sum_beta", "sum_varBeta", "sum_pi"):
        assert np.array_equal(pa[k], pb[k]), k
    for k in ("c", "sum_c", "zeta"):
        assert np.array_equal(la[k], lb[k]), k
    assert la["varZeta"] == lb["varZeta"] and la["sum_varZeta"] == lb["sum_varZeta"] and la["trapped"] == lb["trapped"]


@pytest.mark.parametrize("with_r", [False, True], ids=["lv_pr", "lv_bayesr"])
def test_run_many_is_fused_and_equals_chains_alone(ngp, O, with_r):
    X, y, v, C, cov = _chain_problem(O)
    K = 3
    first = ngp.Sampler(device=0, seed=11, chain=0)
    ms = first.shards_for_pass(K)
    first.close()
    chains = [_full(ngp, X, y, v, C, cov, 11, 0, max_shards=ms, with_r=with_r)]
    for c in range(1, K):
        chains.append(_full(ngp, X, y + 0.01 * c, v, C, cov, 11, c, max_shards=ms, share=chains[0], with_r=with_r))
    ngp.Sampler.run_many(chains, 12)
    assert chains[0].get_timing()["sweep_launches"] == 12          # one fused launch per iteration
    for c in range(K):
        alone = _full(ngp, X, y + 0.01 * c, v, C, cov, 11, c, max_shards=ms, with_r=with_r)
        alone.run(12)
        _same(_everything(chains[c]), _everything(alone))


def test_state_resume_snapshot_and_sample_file(ngp, O, tmp_path):
    X, y, v, C, cov = _chain_problem(O)
    a = _full(ngp, X, y, v, C, cov, 21, 0)
    a.set_sample_file(str(tmp_path / "s.ngpsmp"))
    kept = {}
    for it in range(1, 13):                                         # kept: 4, 6, 8, 10, 12
        a.run(1)
        if it >= 4 and it % 2 == 0:
            kept[it] = a.lv_state(0)
    a.set_sample_file(None)
    S = ngp.read_sample_file(str(tmp_path / "s.ngpsmp"))
    assert S["lv_c"][0].shape == (5, 2) and S["lv_varZeta"].shape == (5, 1) and [int(i) for i in S["iter"]] == sorted(kept)
    for r, it in enumerate(sorted(kept)):
        assert np.array_equal(S["lv_c"][0][r], kept[it]["c"]) and S["lv_varZeta"][r, 0] == kept[it]["varZeta"]
    assert np.array_equal(S["varBeta"][-1], a.get_state()["varBeta"]) and np.array_equal(S["beta"][-1], a.get_state()["beta"])
    assert S["sets"][0]["method"] == 5
    last = a.lv_state(0)
    assert np.allclose(S["lv_c"][0].sum(axis=0), last["sum_c"], rtol=1e-12, atol=1e-12) and np.isclose(S["lv_varZeta"].sum(), last["sum_varZeta"], rtol=1e-12)
    d = _full(ngp, X, y, v, C, cov, 21, 0)                          # the uninterrupted run in one call
    d.run(12)
    _same(_everything(a), _everything(d))
    b = _full(ngp, X, y, v, C, cov, 21, 0)                          # snapshot / resume
    b.run(5)
    b.save_snapshot(str(tmp_path / "snap"))
    c = _full(ngp, X, y, v, C, cov, 21, 0)
    c.load_snapshot(str(tmp_path / "snap"))
    c.run(7)
    _same(_everything(a), _everything(c))
    e = _full(ngp, X, y, v, C, cov, 21, 0, est=0)                   # the signature covers the mode ...
    with pytest.raises(ngp.NextGPHipError, match="does not match"):
        e.load_snapshot(str(tmp_path / "snap"))
    e.run(2)
    f = _full(ngp, X, y, v, np.column_stack([C, np.arange(C.shape[0]) % 3]), cov, 21, 0)   # ... and ncov
    with pytest.raises(ngp.NextGPHipError, match="does not match"):
        f.load_snapshot(str(tmp_path / "snap"))
    g = _full(ngp, X, y, v, C, cov, 21, 0)                          # get_state -> set_state + set_lv_state + set_posterior_sums
    g.run(5)
    st, ps, lv, fx = g.get_state(), g.get_posterior_sums(), g.lv_state(0), g.get_fixed()
    h = _full(ngp, X, y, v, C, cov, 21, 0)
    h.set_state(st); h.set_lv_state(0, lv); h.set_posterior_sums(ps); h.set_fixed(fx["b"], fx["sum_b"])
    h.run(7)
    _same(_everything(a), _everything(h))
    h.set_y(y)                                                      # set_y resets zeta, c and varZeta
    fresh = _full(ngp, X, y, v, C, cov, 21, 0)
    r0, r1 = h.lv_state(0), fresh.lv_state(0)
    assert np.array_equal(r0["zeta"], r1["zeta"]) and np.array_equal(r0["zeta"], RL.zeta_start(O, 21, 0, 0, C.shape[0]))
    assert np.all(r0["c"] == 0) and np.all(r0["sum_c"] == 0) and r0["varZeta"] == 0.5 and r0["sum_varZeta"] == 0.0
    h.run(12)
    _same(_everything(a), _everything(h))


def test_snapshot_and_sample_file_of_a_model_with_every_component(ngp, O, tmp_path):
    """Every component that travels in a snapshot and in a sample record at once: a Tuple set, BayesPR, BayesB, a BayesR set with four
    classes, a BayesLV set with three covariates, a two-column fixed set, a diagonal random-effect set and one with a sparse K, residual
    weights.  Snapshot after 5 of 12 iterations, loaded into a fresh handle, 7 more: everything equals the uninterrupted chain; the
    sample file's last record is the chain's state."""
    rng = np.random.default_rng(12)
    N, v, off = 200, 0.01, 64
    X, y, _, _ = make_problem(O, N, off + 400, seed=8)
    w = rng.uniform(0.5, 2.0, N)
    Z, lev6, lev5 = rng.normal(size=(N, 2)), rng.integers(0, 6, size=N), rng.integers(0, 5, size=N)
    K5 = 2.0 * np.eye(5) - 0.5 * (np.eye(5, k=1) + np.eye(5, k=-1))
    Cm = np.column_stack([np.ones(100), np.arange(100) % 2, rng.normal(size=100)])
    vm = v * (0.6 * np.eye(2) + 0.4 * np.ones((2, 2)))

    def mk():
        s = ngp.Sampler(device=0, seed=13, chain=1)
        s.set_residual_weights(w)
        s.set_panel(X)
        s.add_marker_set_tuple(0, 32, 2, 5.0, vm * 2.0, [(0, 15), (15, 32)], vm)
        s.add_marker_set(off, 100, 0, 4.0, v * 0.5, [(0, 50), (50, 100)], [v, v])
        s.add_marker_set(off + 100, 100, 1, 4.0, v * 0.5, [(j, j + 1) for j in range(100)], [v] * 100, pi0=0.1, estPi=True)
        s.add_marker_set_r(off + 200, 100, 4.0, v * 0.5, v, [0.0, 0.01, 0.1, 1.0], [0.85, 0.10, 0.04, 0.01], estPi=True)
        s.add_fixed_set(Z)
        s.add_random_set(lev6, 6, varU0=0.5)
        s.add_random_set(lev5, 5, K=K5, varU0=0.3)
        s.add_marker_set_lv(off + 300, 100, v, Cm, 0.5, est_mode=1)
        s.set_y(y); s.set_residual_prior(4.0, 0.5); s.set_schedule(12, 2, 2)
        return s

    def everything(s):
        out = [s.get_state(), s.get_posterior_sums(), s.get_fixed(), s.get_random(0), s.get_random(1), s.get_class_state(3), s.lv_state(4)]
        return {f"{i}.{k}": np.asarray(x) for i, d in enumerate(out) for k, x in d.items()}

    a = mk()
    a.set_sample_file(str(tmp_path / "s.ngpsmp"))
    a.run(12)
    a.set_sample_file(None)
    b = mk()
    b.run(5)
    b.save_snapshot(str(tmp_path / "snap"))
    c = mk()
    c.load_snapshot(str(tmp_path / "snap"))
    c.run(7)
    ea, ec = everything(a), everything(c)
    assert sorted(ea) == sorted(ec)
    for k in ea:
        assert np.array_equal(ea[k], ec[k]), k
    assert open(tmp_path / "s.ngpsmp", "rb").read(8) == b"NGPSMP03"
    S = ngp.read_sample_file(str(tmp_path / "s.ngpsmp"))
    st, lv = a.get_state(), a.lv_state(4)
    assert [int(i) for i in S["iter"]] == [4, 6, 8, 10, 12] and S["varE"][-1] == st["varE"] and S["b"][-1] == st["b"]
    for k in ("beta", "varBeta", "piHat", "delta"):
        assert np.array_equal(S[k][-1], st[k]), k
    assert np.array_equal(S["b_fixed"][-1], a.get_fixed()["b"]) and np.array_equal(S["class_pi"][-1], a.get_class_state(3)["piHat"])
    for r in (0, 1):
        assert np.array_equal(S["u"][r][-1], a.get_random(r)["u"]) and S["varU"][-1, r] == a.get_random(r)["varU"]
    assert np.array_equal(S["lv_c"][0][-1], lv["c"]) and S["lv_varZeta"][-1, 0] == lv["varZeta"]
    assert a.posterior_len() == 3 * a.P + a.nvb + 2 * 5 + 4 + 2 + (6 + 5 + 2) + 17 + 3


def test_posterior_len_and_pooled_sums(ngp, O):
    X, y, v, C, cov = _chain_problem(O)
    chains = [_full(ngp, X, y + 0.01 * c, v, C, cov, 5, c) for c in range(4)]
    for s in chains:
        s.run(12)
    assert chains[0].posterior_len() == 3 * X.shape[1] + chains[0].nvb + 2 * 2 + 1 + 17 + 3   # + sums of c (16 words) and of varZeta
    own = [s.lv_state(0) for s in chains]
    ps = [s.get_posterior_sums() for s in chains]
    for vd in ((None,) * 4, (0, 1, 0, 2)):                          # one device; the multi-device branch under virtual devices
        again = [_full(ngp, X, y + 0.01 * c, v, C, cov, 5, c) for c in range(4)]
        for s, d in zip(again, vd):
            s.run(12)
            if d is not None:
                s.debug_set_virtual_device(d)
        ngp.Sampler.allreduce_posterior(again)
        for s in again:
            lv = s.lv_state(0)
            assert np.allclose(lv["sum_c"], sum(o["sum_c"] for o in own), rtol=1e-12, atol=0)
            assert np.isclose(lv["sum_varZeta"], sum(o["sum_varZeta"] for o in own), rtol=1e-12)
            assert np.allclose(s.get_posterior_sums()["sum_varBeta"], sum(p["sum_varBeta"] for p in ps), rtol=1e-12, atol=0)
            assert s.get_posterior_sums()["nKept"] == 20


def test_refusals_leave_a_handle_that_runs(ngp, O):
    X, y, v, C, cov = _chain_problem(O)
    Pl = C.shape[0]
    s = ngp.Sampler(device=0, seed=3, chain=0)
    s.set_panel(X)
    nan_c = C.copy(); nan_c[5, 1] = np.nan
    singular = np.column_stack([C[:, 1], -C[:, 1]]) * 0.0
    bad = [dict(C=np.ones((Pl, 17))), dict(C=nan_c), dict(vb0=0.0), dict(vb0=-1.0), dict(vz=0.0), dict(vz=-2.0),
           dict(mode=3), dict(mode=-1), dict(mode=2, frac=0.0), dict(mode=2, frac=-0.5), dict(C=singular), dict(zeta0=np.full(Pl, np.inf))]
    for kw in bad:
        with pytest.raises(ngp.NextGPHipError, match="BayesLV"):
            s.add_marker_set_lv(0, Pl, kw.get("vb0", v), kw.get("C", C), kw.get("vz", 0.5), est_mode=kw.get("mode", 0), est_fraction=kw.get("frac", 0.0),
                                zeta0=kw.get("zeta0"))
    with pytest.raises(ngp.NextGPHipError, match="two loci"):
        s.add_marker_set_lv(0, 1, v, np.ones((1, 1)), 0.5, est_mode=1)
    assert s.nsets == 0
    sid = s.add_marker_set_lv(0, Pl, v, C, 0.5, est_mode=1)
    assert sid == 0
    with pytest.raises(ngp.NextGPHipError, match="overlap"):
        s.add_marker_set_lv(10, 20, v, C[:20], 0.5)
    Pp = X.shape[1] - Pl
    s.add_marker_set(Pl, Pp, 0, 4.0, v * 0.5, [(0, Pp)], [v])
    s.set_y(y); s.set_residual_prior(4.0, 1.0); s.run(3)
    with pytest.raises(ngp.NextGPHipError):
        s.set_lv_state(sid, dict(varZeta=-1.0))
    with pytest.raises(ngp.NextGPHipError):
        s._chk(s.L.ngp_get_lv_state(s.h, 1, None, None, None, None, None, None, None))   # set 1 is the BayesPR set
    s.run(1)
    lv = s.lv_state(sid)
    assert np.all(np.isfinite(lv["c"])) and lv["varZeta"] > 0 and np.all(s.get_state()["varBeta"] > 0)


def test_runLMEM_end_to_end(ngp, O, tmp_path):
    """A simulated panel whose true effect variance is larger for the SNPs with a binary covariate = 1.  The files exist with the pinned
    headers; the posterior means of c and varZeta are judged against LVRefChain on the same data and draws, at the tolerance of
    test_chain_vs_reference_order (1e-9 relative)."""
    from nextgp_jl_amd import api
    N, P = 256, 192                                                 # N a power of two: codes minus their mean are exact in fp32 tiles
    X, y, _, v = make_problem(O, N, P, seed=8)
    X = np.rint(X.astype(np.float64) - X.min(axis=0))                # genotype codes 0 / 1 / 2
    rng = np.random.default_rng(8)
    a = rng.integers(0, 2, P)
    bt = rng.normal(size=P) * np.where(a == 1, 0.6, 0.05)
    y = 5.0 + X.astype(np.float64) @ bt + rng.normal(size=N)
    geno = str(tmp_path / "geno.npy")
    np.save(geno, X.astype(np.float64))
    cov = dict(annot=a)
    nChain, nBurn, nThin = 40, 10, 2
    prior = api.BayesLV(v, "0 ~ annot", cov, 0.5, estimateVarZeta=True)
    out = str(tmp_path / "one")
    res = api.runLMEM(f'y ~ 1 + SNP(M, "{geno}")', dict(y=y), nChain, nBurn, nThin, outFolder=out, VCV={"M": prior, "e": api.Random("I", 1.0)}, seed=13)
    head = lambda n: open(os.path.join(out, n)).readline().rstrip("\n").split("\t")
    assert head("cMOut") == ["c1", "c2"] and head("varZetaMOut") == ["varZeta"] and head("varMOut") == [f"reg_{j + 1}" for j in range(P)]
    cm = api.summaryMCMC("cM", outFolder=out)[0]
    assert np.allclose(cm, res["sets"]["M"]["c"], rtol=1e-12, atol=1e-12)
    assert np.isclose(api.summaryMCMC("varZetaM", outFolder=out)[0, 0], res["sets"]["M"]["varZeta"], rtol=1e-12)
    # the reference-order chain on the same data (centred in Float64 as runLMEM centres, src/prepMatVec.jl:129) and draws
    Xc = X.astype(np.float64); Xc = Xc - Xc.mean(axis=0)
    ref = RL.LVRefChain(O, Xc, y, seed=13, chain=0)
    Cm, _ = api.lv_design_matrix(prior.f, cov)
    ref.add_set_lv(0, P, v, Cm, 0.5, est=True)
    ref.E_df, ref.E_scale = 4.0, 1.0 * 2.0 / 4.0
    sc, sv, n = np.zeros(2), 0.0, 0
    for it in range(1, nChain + 1):
        ref.run(1)
        if it >= nBurn + nThin and (it - nBurn) % nThin == 0:
            sc += ref.M[0]["c"]; sv += ref.M[0]["varZeta"][0]; n += 1
    g = max(np.abs(res["sets"]["M"]["c"] - sc / n).max() / np.abs(sc / n).max(), abs(res["sets"]["M"]["varZeta"] / (sv / n) - 1))
    print("runLMEM against LVRefChain: posterior means of c", res["sets"]["M"]["c"], sc / n, "varZeta", res["sets"]["M"]["varZeta"], sv / n, "gap", g)
    assert n == res["nKept"] and g <= 1e-9
    res3 = api.runLMEM(f'y ~ 1 + SNP(M, "{geno}")', dict(y=y), nChain, nBurn, nThin, outFolder=str(tmp_path / "three"),
                       VCV={"M": prior, "e": api.Random("I", 1.0)}, seed=13, chains=3)
    assert os.path.exists(os.path.join(str(tmp_path / "three"), "chain0", "cMOut")) and res3["sets"]["M"]["c"].shape == (2,)
    assert len(res3["chains"]) == 3 and np.all(np.isfinite(res3["sets"]["M"]["c"])) and res3["sets"]["M"]["varZeta"] > 0
