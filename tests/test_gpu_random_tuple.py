"""Correlated (Tuple) random-effect sets on the device (ngp_random_tuple.h): the fine seam under both Gauss-Seidel engines against the
restatement of the documented order, bit for bit; k = 1 against ngp_add_random_set; whole chains against the reference's lines with
the one documented change (ref_random_tuple.TupleRefChain) and, where no record links two levels, against the literal lines; state,
snapshots, sample files, fused chains per pass and runLMEM.  Nothing here times anything."""
import os

import numpy as np
import pytest

import ref_pedigree as RP
import ref_random_tuple as RT
from conftest import make_problem

pytestmark = pytest.mark.gpu

SHAPES = {"ped14": (RP.pblup_sire_dam, 10), "ped3000": (lambda: RP.random_pedigree(3000, 2000), 600),
          "ped21000": (lambda: RP.random_pedigree(21000, 4000), 800)}
_cache = {}


def _shape(ngp, name):
    if name not in _cache:
        s, d = SHAPES[name][0]()
        _, K = ngp.pedigree_ainv(s, d)
        rows = RP.csr_rows(*K)
        _cache[name] = dict(n=len(s), K=K, rows=rows, dam=d.astype(np.int64) - 1, sire=s.astype(np.int64) - 1)
    return _cache[name]


def _levels(sh, name, nrec, k, rng):
    """(ID, Dam[, Sire]) of nrec records; founders among the animals give -1 in the second component."""
    n = sh["n"]
    animal = np.arange(4, 14) if name == "ped14" else rng.integers(n // 3, n, size=nrec)
    if name == "ped14":
        animal[0] = 1                                                         # a founder: its dam is unknown
    else:
        animal[:8] = np.arange(8)                                             # founders
    comps = [animal, sh["dam"][animal], sh["sire"][animal]][:k]
    assert (comps[1] < 0).any() and (comps[1] >= 0).any()
    return np.stack(comps)


CASES = [(n, k) for n in ("ped14", "ped3000") for k in (2, 3)] + [("ped21000", 2)]


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("name,k", CASES, ids=[f"{n}-k{k}" for n, k in CASES])
def test_fine_seam_serial_equals_scheduled_equals_restatement(ngp, O, name, k, weighted):
    sh = _shape(ngp, name)
    n, nrec = sh["n"], SHAPES[name][1]
    rng = np.random.default_rng(4)
    levels = _levels(sh, name, nrec, k, rng)
    w = rng.uniform(0.3, 3.0, nrec) if weighted else None
    rs = np.sqrt(w) if weighted else None
    setup = RT.tuple_setup(levels, n, w)
    dep = RT.union_depths(sh["rows"], setup[2])
    order, dptr = RT.schedule_of(dep)
    plan = RP.plan(dptr)
    kinds = [p[0] for p in plan]
    if name == "ped14":
        assert kinds == ["fused"]
    elif name == "ped3000":
        assert max(np.diff(dptr)) > 1024 and kinds[0] == "wide" and kinds[-1] == "fused"
    else:
        assert 8 * n * k > 160 * 1024
    A = rng.normal(size=(k, k))
    V0 = A @ A.T + k * np.eye(k)
    V0 = (V0 + V0.T) / 2
    scale = V0 * 0.5
    df = 3.0 + k
    y0, u0 = rng.normal(size=nrec), rng.normal(size=(n, k))
    out = {}
    for mode in (1, 2):
        s = ngp.Sampler(device=0, seed=77, chain=2)
        if weighted:
            s.set_residual_weights(w)
        s.set_records(nrec)
        rid = s.add_random_set_tuple(levels, n, K=sh["K"], df=df, scale=scale, varU0=V0)
        s.set_random_schedule(rid, mode)
        assert s.get_random_schedule(rid) == dict(engine=mode, depths=len(dptr) - 1, launches=1 if mode == 1 else len(plan))
        ycorr, u, varU, calls = y0.copy(), u0.copy(), V0.copy(), []
        for _ in range(5):
            s.sample_random_set_tuple(rid, 1.3, ycorr, u, varU)
            calls.append((ycorr.copy(), u.copy(), varU.copy()))
        out[mode] = calls
        s.close()
    for it, (a, b) in enumerate(zip(out[1], out[2])):
        assert all(np.array_equal(x, z) for x, z in zip(a, b)), it
    assert np.all(np.isfinite(out[1][-1][1])) and np.all(np.isfinite(out[1][-1][2]))
    ycorr, u, varU = y0, u0, V0
    for it in range(1 if name == "ped21000" else 5):
        yt_in = ycorr * rs if weighted else ycorr
        yt, u_ref, v_ref = RT.tuple_step_blocked(O, 77, 2, it + 1, 0, yt_in, None if rs is None else list(rs), levels, n, sh["rows"], setup, u, varU,
                                                 1.3, df, scale)
        ycorr, u, varU = (np.array(yt) / rs if weighted else np.array(yt)), np.array(u_ref), np.array(v_ref).reshape(k, k)
        got = out[1][it]
        print(name, k, weighted, it, np.abs(got[1] - u).max(), np.abs(got[2] - varU).max(), np.abs(got[0] - ycorr).max())
        assert np.array_equal(got[1], u) and np.array_equal(got[2], varU) and np.array_equal(got[0], ycorr), it


def test_k1_is_the_scalar_set(ngp):
    sh = _shape(ngp, "ped3000")
    n, nrec = sh["n"], 600
    rng = np.random.default_rng(9)
    level = rng.integers(n // 3, n, size=nrec)
    y0, u0 = rng.normal(size=nrec), rng.normal(size=n)
    df, scale, v0 = 4.0, 0.4, 0.8
    a = ngp.Sampler(device=0, seed=5, chain=1); a.set_records(nrec)
    ra = a.add_random_set(level, n, K=sh["K"], df=df, scale=scale, varU0=v0)
    b = ngp.Sampler(device=0, seed=5, chain=1); b.set_records(nrec)
    rb = b.add_random_set_tuple(level[None, :], n, K=sh["K"], df=df, scale=[[scale * df]], varU0=[[v0]])
    ya, ua, va = y0.copy(), u0.copy(), v0
    yb, ub, vb = y0.copy(), u0.copy().reshape(n, 1), np.array([[v0]])
    for it in range(5):
        va = a.sample_random_set(ra, 1.3, ya, ua, va)
        b.sample_random_set_tuple(rb, 1.3, yb, ub, vb)
        assert np.array_equal(ua, ub[:, 0]) and np.array_equal(ya, yb) and va == vb[0, 0], it
    assert np.abs(ua - u0).max() > 0
    g = b.get_random_tuple(rb)
    assert g["u"].shape == (n, 1) and np.array_equal(g["u"][:, 0], ua) and g["varU"][0, 0] == va
    assert np.array_equal(a.get_random_tuple(ra)["u"][:, 0], a.get_random(ra)["u"])


def _chain_problem(ngp, O, same_levels=False):
    X, y, _, v = make_problem(O, 200, 256, seed=5)
    s_, d_ = RP.random_pedigree(300, 60, seed=3)
    _, K = ngp.pedigree_ainv(s_, d_)
    rng = np.random.default_rng(6)
    animal = rng.integers(40, 300, size=200)                                   # some founders: unknown dams
    dam = d_[animal].astype(np.int64) - 1
    levels = np.stack([animal, animal if same_levels else dam])
    assert same_levels or ((dam < 0).any() and (dam >= 0).any())
    sd = np.sqrt(y.var())
    y = y + rng.normal(size=300)[animal] * sd + np.where(dam >= 0, rng.normal(size=300)[dam], 0.0) * 0.5 * sd
    V = np.array([[0.5, -0.1], [-0.1, 0.3]]) * y.var()
    return X, y, v, levels, K, V


def _chain(ngp, X, y, v, levels, K, V, mode=0, chain=0, share=None, max_shards=None, w=None, storage=None, nchain=30):
    s = ngp.Sampler(device=0, seed=13, chain=chain, **({} if storage is None else dict(storage=storage)))
    if w is not None:
        s.set_residual_weights(w)
    if max_shards:
        s.set_max_shards(max_shards)
    if share is not None:
        s.share_panel(share)
    elif storage is not None:
        s.set_panel(np.asfortranarray(np.rint(X.astype(np.float64) - X.min(axis=0)).astype(np.uint8)), centre=True)
    else:
        s.set_panel(X)
    rid = s.add_random_set_tuple(levels, 300, K=K, varU0=V)                    # df = 3 + k, scale = V (df - k - 1)
    if mode:
        s.set_random_schedule(rid, mode)
    s.add_marker_set(0, 256, 0, 4.0, v * 0.5, [(0, 256)], [v])
    s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var()); s.set_schedule(nchain, 10, 2)
    return s


def _tol(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    err = np.abs(a - b).max() / max(1e-300, np.abs(b).max())
    print("rel", err)
    return err <= 1e-9


@pytest.mark.parametrize("same_levels", [False, True], ids=["id_dam-changed", "one_level_vector-literal"])
def test_whole_chain_against_the_reference_lines(ngp, O, same_levels):
    """(ID, Dam): the reference's lines with the one documented change.  Both components on one level vector: the reference's own
    lines, unchanged -- there the two coincide, which pins the build to the reference."""
    X, y, v, levels, K, V = _chain_problem(ngp, O, same_levels)
    s = _chain(ngp, X, y, v, levels, K, V)
    ref = RT.TupleRefChain(O, X.astype(np.float64), y, seed=13, chain=0, literal=same_levels)
    ref.add_random_tuple(levels, 300, RP.csr_dense(*K), v=V)
    ref.add_set(0, 256, 0, 4.0, v * 0.5, [(0, 256)], [v])
    ref.E_df, ref.E_scale = 4.0, 0.25 * y.var()
    s.run(30); ref.run(30)
    a, g, b = s.get_state(), s.get_random_tuple(0), ref.state()
    assert _tol(g["u"], ref.u[0]) and _tol(g["varU"], ref.varU[0])
    assert _tol(a["beta"], b["beta"]) and abs(a["varE"] - b["varE"]) <= 1e-9 * b["varE"] and _tol(a["ycorr"], b["ycorr"])
    if not same_levels:                                                        # the literal lines are another chain here
        lit = RT.TupleRefChain(O, X.astype(np.float64), y, seed=13, chain=0, literal=True)
        lit.add_random_tuple(levels, 300, RP.csr_dense(*K), v=V)
        lit.add_set(0, 256, 0, 4.0, v * 0.5, [(0, 256)], [v])
        lit.E_df, lit.E_scale = 4.0, 0.25 * y.var()
        lit.run(3)
        ref3 = RT.TupleRefChain(O, X.astype(np.float64), y, seed=13, chain=0)
        ref3.add_random_tuple(levels, 300, RP.csr_dense(*K), v=V)
        ref3.add_set(0, 256, 0, 4.0, v * 0.5, [(0, 256)], [v])
        ref3.E_df, ref3.E_scale = 4.0, 0.25 * y.var()
        ref3.run(3)
        assert np.abs(lit.u[0] - ref3.u[0]).max() > 1e-6 * np.abs(ref3.u[0]).max()


@pytest.mark.parametrize("variant", ["fp32", "weighted", "u8"])
def test_state_holds_together(ngp, O, variant):
    X, y, v, levels, K, V = _chain_problem(ngp, O)
    kw = {}
    if variant == "weighted":
        kw["w"] = np.random.default_rng(1).uniform(0.3, 3.0, len(y))
    if variant == "u8":
        kw["storage"] = 1
    s = _chain(ngp, X, y, v, levels, K, V, nchain=50, **kw)
    s.run(50)
    st, u = s.get_state(), s.get_random_tuple(0)["u"]
    zu = sum(np.where(levels[m] >= 0, u[np.maximum(levels[m], 0), m], 0.0) for m in range(2))
    exp = y - st["b"] - zu - s.xbeta(st["beta"])
    err = np.abs(st["ycorr"] - exp).max() / np.abs(y).max()
    print("ycorr rel", err)
    assert err <= 1e-9 and np.abs(u).max() > 0


def _everything(s):
    import torch
    n = s.posterior_len()
    buf = torch.zeros(n, device="cuda", dtype=torch.float64)
    s.export_posterior_device(buf.data_ptr(), n)
    torch.cuda.synchronize()
    return buf.cpu().numpy(), s.get_state(), s.get_random_tuple(0)


def _same(a, b):
    assert np.array_equal(a[0], b[0])
    for k in ("ycorr", "beta", "varBeta"):
        assert np.array_equal(a[1][k], b[1][k]), k
    assert a[1]["varE"] == b[1]["varE"] and a[1]["b"] == b[1]["b"]
    for k in ("u", "sum_u", "varU", "sum_varU"):
        assert np.array_equal(a[2][k], b[2][k]), k


def test_snapshot_sample_file_and_packed_posterior(ngp, O, tmp_path):
    X, y, v, levels, K, V = _chain_problem(ngp, O)
    a = _chain(ngp, X, y, v, levels, K, V, mode=1)
    a.set_sample_file(str(tmp_path / "s.ngpsmp"))
    a.run(30)
    a.set_sample_file(None)
    ea = _everything(a)
    S = ngp.read_sample_file(str(tmp_path / "s.ngpsmp"))                       # kept: 12, 14, .., 30
    assert S["u"][0].shape == (10, 600) and S["varU"].shape == (10, 4)
    assert np.array_equal(S["u"][0][-1].reshape(300, 2), ea[2]["u"]) and np.array_equal(S["varU"][-1].reshape(2, 2), ea[2]["varU"])
    assert np.allclose(S["u"][0].sum(axis=0).reshape(300, 2), ea[2]["sum_u"], rtol=1e-12, atol=1e-12)
    assert np.allclose(S["varU"].sum(axis=0).reshape(2, 2), ea[2]["sum_varU"], rtol=1e-12)
    assert np.array_equal(S["beta"][-1], ea[1]["beta"])
    # the packed posterior: ... | sum_u (q k) | sum_varU (k k) | sum_varE | sum_b | nKept
    assert a.posterior_len() == 3 * 256 + a.nvb + 2 + (600 + 4) + 3
    assert np.array_equal(ea[0][-3 - 4 - 600:-3 - 4].reshape(300, 2), ea[2]["sum_u"]) and np.array_equal(ea[0][-7:-3].reshape(2, 2), ea[2]["sum_varU"])
    b = _chain(ngp, X, y, v, levels, K, V, mode=2)                             # resume mid-chain, under the other engine
    b.run(13)
    b.save_snapshot(str(tmp_path / "snap"))
    c = _chain(ngp, X, y, v, levels, K, V, mode=1)
    c.load_snapshot(str(tmp_path / "snap"))
    c.run(17)
    _same(ea, _everything(c))
    other = levels.copy(); other[1, 0] = -1 if other[1, 0] >= 0 else 0
    d = _chain(ngp, X, y, v, other, K, V)                                      # other levels
    with pytest.raises(ngp.NextGPHipError, match="random-effect sets differ"):
        d.load_snapshot(str(tmp_path / "snap"))
    d.run(2)
    e = ngp.Sampler(device=0, seed=13, chain=0)                                # another k: a scalar set over the first component
    e.set_panel(X); e.add_random_set(levels[0], 300, K=K, varU0=V[0, 0])
    e.add_marker_set(0, 256, 0, 4.0, v * 0.5, [(0, 256)], [v]); e.set_y(y)
    with pytest.raises(ngp.NextGPHipError, match="random-effect sets differ"):
        e.load_snapshot(str(tmp_path / "snap"))
    e.run(2)
    # set_random_tuple restores what get_random_tuple gave; set_y resets u = 0, varU = varU0
    g = c.get_random_tuple(0)
    c.set_random_tuple(0, u=g["u"] * 0 + 1.5, varU=V)
    g2 = c.get_random_tuple(0)
    assert np.all(g2["u"] == 1.5) and np.array_equal(g2["varU"], V) and np.array_equal(g2["sum_u"], g["sum_u"])
    with pytest.raises(ngp.NextGPHipError, match="positive definite"):
        c.set_random_tuple(0, varU=np.array([[1.0, 2.0], [2.0, 1.0]]))
    with pytest.raises(ngp.NextGPHipError, match="k-fold"):
        c.get_random(0)
    c.set_y(y)
    g3 = c.get_random_tuple(0)
    assert not g3["u"].any() and not g3["sum_u"].any() and np.array_equal(g3["varU"], V) and not g3["sum_varU"].any()


def test_two_fused_chains_per_pass(ngp, O):
    X, y, v, levels, K, V = _chain_problem(ngp, O)
    first = ngp.Sampler(device=0, seed=13, chain=0)
    ms = first.shards_for_pass(2)
    first.close()
    c0 = _chain(ngp, X, y, v, levels, K, V, chain=0, max_shards=ms)
    c1 = _chain(ngp, X, y + 0.01, v, levels, K, V, chain=1, share=c0, max_shards=ms)
    c0.get_timing()
    ngp.Sampler.run_many([c0, c1], 30)
    assert c0.get_timing()["sweep_launches"] == 30                             # ONE fused sweep launch per iteration for both chains
    for cid, c, yy in ((0, c0, y), (1, c1, y + 0.01)):
        alone = _chain(ngp, X, yy, v, levels, K, V, chain=cid, max_shards=ms)
        alone.run(30)
        _same(_everything(c), _everything(alone))


def test_refusals_leave_a_handle_that_runs(ngp, O):
    X, y, v, levels, K, V = _chain_problem(ngp, O)
    s = ngp.Sampler(device=0, seed=3, chain=0)
    s.set_panel(X)
    bad = levels.copy(); bad[1, 3] = 300
    low = levels.copy(); low[0, 3] = -2
    for lv, kw in ((bad, {}), (low, {}), (levels, dict(varU0=np.array([[1.0, 2.0], [2.0, 1.0]]))), (levels, dict(varU0=np.array([[1.0, 0.2], [0.3, 1.0]]))),
                   (levels, dict(scale=np.array([[1.0, 0.0], [0.0, -1.0]]))), (np.stack([levels[0]] * 5), dict(varU0=np.eye(5)))):
        kw = dict(dict(varU0=V), **kw)
        with pytest.raises((ngp.NextGPHipError, ValueError)):
            s.add_random_set_tuple(lv, 300, K=K, **kw)
        s.rand_q = []
    with pytest.raises(ngp.NextGPHipError, match="outside 0..q-1"):
        s.add_random_set(levels[1], 300, K=K)                                  # the scalar entry point keeps refusing -1
    s.rand_q = []
    rid = s.add_random_set_tuple(levels, 300, K=K, varU0=V)
    s.add_marker_set(0, 256, 0, 4.0, v * 0.5, [(0, 256)], [v]); s.set_y(y); s.set_residual_prior(4.0, 1.0); s.run(3)
    assert np.all(np.isfinite(s.get_random_tuple(rid)["u"]))
    with pytest.raises(ngp.NextGPHipError):
        s.sample_random_set_tuple(rid, -1.0, y.copy(), np.zeros((300, 2)), V.copy())
    with pytest.raises(ngp.NextGPHipError, match="k-fold"):
        s.sample_random_set(rid, 1.0, y.copy(), np.zeros(300), 1.0)
    s.run(1)


def _pblup_data():
    D = RP.PBLUP_DATA
    return dict(ID=np.array([r[0] for r in D]), Dam=np.array([r[2] for r in D]), BW=np.array([r[5] for r in D]))


@pytest.mark.parametrize("snp", [False, True], ids=["ped_only", "ped_plus_snp"])
def test_runLMEM_direct_maternal_model(ngp, O, tmp_path, snp):
    from nextgp_jl_amd import api
    data = _pblup_data()
    V = np.array([[150.0, -40.0], [-40.0, 90.0]])
    VCV = {("ID", "Dam"): api.Random("A", V), "e": api.Random("I", 350.0)}
    formula = "BW ~ 1 + PED(ID) + PED(Dam)"
    P, vm = 64, 0.5
    if snp:
        rng = np.random.default_rng(2)
        M = np.column_stack([rng.permutation([0, 0, 0, 1, 1, 1, 1, 2, 2, 2]) for _ in range(P)]).astype(np.float64)
        np.save(str(tmp_path / "g.npy"), M)
        formula += ' + SNP(M1, "%s")' % str(tmp_path / "g.npy")
        VCV["M1"] = api.BayesPR(9999, vm)
    out = str(tmp_path / "out")
    res = api.runLMEM(formula, data, 8, 2, 2, outFolder=out, VCV=VCV, userPedData=RP.PBLUP_PED, seed=1)
    ids = [r[0] for r in RP.PBLUP_PED]
    for nm in ("uIDOut", "uDamOut"):
        with open(os.path.join(out, nm)) as f:
            lines = f.read().rstrip("\n").split("\n")
        assert lines[0].split("\t") == ids and len(lines) == 1 + 3
    with open(os.path.join(out, "varU(:ID, :Dam)Out")) as f:
        lines = f.read().rstrip("\n").split("\n")
    assert lines[0].split("\t") == ["ID_Dam_1", "ID_Dam_2", "ID_Dam_3", "ID_Dam_4"] and len(lines) == 1 + 3
    rr = res["random"][("ID", "Dam")]
    assert rr["levels"] == ids and rr["u"].shape == (2, 14) and rr["varU"].shape == (2, 2)
    assert np.allclose(api.summaryMCMC("uID", outFolder=out)[0], rr["u"][0], rtol=1e-12, atol=1e-12)
    assert np.allclose(api.summaryMCMC("uDam", outFolder=out)[0], rr["u"][1], rtol=1e-12, atol=1e-12)
    assert np.allclose(api.summaryMCMC("varU(:ID, :Dam)", outFolder=out)[0], rr["varU"].T.ravel(), rtol=1e-12)
    # the reference's lines with the one documented change, the same K
    _, Kc = ngp.pedigree_ainv(*RP.pblup_sire_dam())
    levels = np.array([[ids.index(a) for a in data["ID"]], [ids.index(a) for a in data["Dam"]]])
    ref = RT.TupleRefChain(O, (M - 1.0) if snp else np.zeros((10, 1)), data["BW"], seed=1, chain=0)
    ref.add_random_tuple(levels, 14, RP.csr_dense(*Kc), v=V)
    if snp:
        ref.add_set(0, P, 0, 4.0, vm * 0.5, [(0, P)], [vm])
    ref.E_df, ref.E_scale = 4.0, 175.0
    ref.run(8)
    smp = res["sampler"]
    a, g = smp.get_state(), smp.get_random_tuple(0)
    assert _tol(g["u"], ref.u[0]) and _tol(g["varU"], ref.varU[0]) and _tol(a["ycorr"], ref.ycorr)
    assert abs(a["varE"] - ref.varE) <= 1e-9 * ref.varE and abs(a["b"] - ref.b[0]) <= 1e-9 * abs(ref.b[0])
    if snp:
        assert _tol(a["beta"][:P], ref.state()["beta"]) and sorted(res["sets"]) == ["M1"]
