"""Pedigree BLUP on the device: the level-scheduled Gauss-Seidel engine of CSR random-effect sets (k_rand_sched_*) against the serial one
(k_rand_gs), bit for bit, on A^-1 of pedigrees (ngp_pedigree_ainv); whole chains under both engines; runLMEM with PED terms.
Yardsticks: ref_random.random_step_blocked (the device's documented order, bit for bit) and ref_random.RandomRefChain (the reference's
order, to 1e-9 relative).  Nothing here times anything."""
import os

import numpy as np
import pytest

import ref_pedigree as RP
import ref_random as RR
from conftest import make_problem

pytestmark = pytest.mark.gpu

# shape -> (sire, dam) and the number of records; the first third of the animals has no record in any of them
SHAPES = {"ped14": (RP.pblup_sire_dam, 10), "ped3000": (lambda: RP.random_pedigree(3000, 2000), 600),
          "ped21000": (lambda: RP.random_pedigree(21000, 4000), 800)}
_cache = {}


def _shape(ngp, name):
    if name not in _cache:
        s, d = SHAPES[name][0]()
        _, K = ngp.pedigree_ainv(s, d)
        rows = RP.csr_rows(*K)
        order, dptr = RP.schedule(rows)
        _cache[name] = dict(n=len(s), K=K, rows=rows, dptr=dptr, plan=RP.plan(dptr))
    return _cache[name]


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_fine_seam_scheduled_equals_serial_equals_restatement(ngp, O, name, weighted, monkeypatch):
    """ped14: one fused single-workgroup launch; ped3000: a multi-workgroup launch followed by a fused one; ped21000: more levels than
    the serial engine holds in LDS (it reads u from global memory), wide and fused launches in turn.  The restatement is compared on
    every call of the two small shapes and on the first call of the large one (a Python loop over 21,000 levels per call)."""
    sh = _shape(ngp, name)
    n, nrec = sh["n"], SHAPES[name][1]
    kinds = [k for k, _, _ in sh["plan"]]
    if name == "ped14":
        assert sh["plan"] == [("fused", 0, 7)] and max(np.diff(sh["dptr"])) <= 3
    elif name == "ped3000":
        assert kinds[0] == "wide" and kinds[-1] == "fused" and max(np.diff(sh["dptr"])) > 1024
    else:
        assert n * 8 > 160 * 1024 and "wide" in kinds and "fused" in kinds
    rng = np.random.default_rng(4)
    level = np.arange(4, 14) if name == "ped14" else rng.integers(n // 3, n, size=nrec)
    w = rng.uniform(0.3, 3.0, nrec) if weighted else None
    rs = np.sqrt(w) if weighted else None
    y0, u0 = rng.normal(size=nrec), rng.normal(size=n)
    out = {}
    for mode in (1, 2):
        s = ngp.Sampler(device=0, seed=77, chain=2)
        if weighted:
            s.set_residual_weights(w)
        s.set_records(nrec)
        rid = s.add_random_set(level, n, K=sh["K"], df=4.0, scale=0.4, varU0=0.8)
        assert s.get_random_schedule(rid)["engine"] in (1, 2)                           # (automatic: whichever the rule picks)
        s.set_random_schedule(rid, mode)
        info = s.get_random_schedule(rid)
        assert info == dict(engine=mode, depths=len(sh["dptr"]) - 1, launches=1 if mode == 1 else len(sh["plan"]))
        ycorr, u, varU, calls = y0.copy(), u0.copy(), 0.8, []
        for _ in range(5):
            varU = s.sample_random_set(rid, 1.3, ycorr, u, varU)
            calls.append((ycorr.copy(), u.copy(), varU))
        out[mode] = calls
        s.close()
    for it, (a, b) in enumerate(zip(out[1], out[2])):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2], it
    monkeypatch.setattr(RR, "csr_of", lambda K, q: sh["rows"])     # the CSR rows as they are (not through a dense n x n array)
    zpz = RR.zpz_of(level, n, w)
    ycorr, u, varU = y0, u0, 0.8
    for it in range(1 if name == "ped21000" else 5):
        yt_in = ycorr * rs if weighted else ycorr
        yt, u_ref, v_ref = RR.random_step_blocked(O, 77, 2, it + 1, 0, yt_in, None if rs is None else list(rs), level, n, None, zpz, u, varU,
                                                  1.3, 4.0, 0.4)
        ycorr, u, varU = (np.array(yt) / rs if weighted else np.array(yt)), np.array(u_ref), v_ref
        assert np.array_equal(out[1][it][1], u) and out[1][it][2] == varU and np.array_equal(out[1][it][0], ycorr), it


def _chain_problem(ngp, O):
    X, y, _, v = make_problem(O, 200, 256, seed=5)
    s_, d_ = RP.random_pedigree(300, 60, seed=3)
    _, K = ngp.pedigree_ainv(s_, d_)
    rng = np.random.default_rng(6)
    animal = rng.integers(100, 300, size=200)
    return X, y + rng.normal(size=300)[animal] * np.sqrt(y.var()), v, animal, K


def _chain(ngp, X, y, v, animal, K, mode, chain=0, share=None, max_shards=None):
    s = ngp.Sampler(device=0, seed=13, chain=chain)
    if max_shards:
        s.set_max_shards(max_shards)
    if share is not None:
        s.share_panel(share)
    else:
        s.set_panel(X)
    rid = s.add_random_set(animal, 300, K=K, df=4.0, scale=0.5 * y.var() * 0.5, varU0=0.5 * y.var())
    s.set_random_schedule(rid, mode)
    s.add_marker_set(0, 256, 0, 4.0, v * 0.5, [(0, 256)], [v])
    s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var()); s.set_schedule(30, 10, 2)
    return s


def _packed(s):
    import torch
    n = s.posterior_len()
    buf = torch.zeros(n, device="cuda", dtype=torch.float64)
    s.export_posterior_device(buf.data_ptr(), n)
    torch.cuda.synchronize()
    r = s.get_random(0)
    return buf.cpu().numpy(), s.get_state()["ycorr"], r["u"], r["varU"]


def _same(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and a[3] == b[3]


def test_chains_under_both_engines_are_the_same_chain(ngp, O, tmp_path):
    X, y, v, animal, K = _chain_problem(ngp, O)
    ser = _chain(ngp, X, y, v, animal, K, 1); ser.run(30)
    sch = _chain(ngp, X, y, v, animal, K, 2); sch.run(30)
    assert sch.get_random_schedule(0)["engine"] == 2 and ser.get_random_schedule(0)["engine"] == 1
    ref = _packed(ser)
    assert np.abs(ref[2]).max() > 0
    _same(ref, _packed(sch))
    # run_many of two chains under each engine
    first = ngp.Sampler(device=0, seed=13, chain=0)
    ms = first.shards_for_pass(2)
    first.close()
    many = {}
    for mode in (1, 2):
        c0 = _chain(ngp, X, y, v, animal, K, mode, 0, max_shards=ms)
        c1 = _chain(ngp, X, y + 0.01, v, animal, K, mode, 1, share=c0, max_shards=ms)
        ngp.Sampler.run_many([c0, c1], 30)
        many[mode] = (_packed(c0), _packed(c1))
    _same(many[1][0], many[2][0]); _same(many[1][1], many[2][1])
    # a snapshot taken under one engine loads under the other: the signature does not depend on the schedule
    for m_save, m_load in ((1, 2), (2, 1)):
        a = _chain(ngp, X, y, v, animal, K, m_save); a.run(12)
        a.save_snapshot(str(tmp_path / f"snap{m_save}"))
        b = _chain(ngp, X, y, v, animal, K, m_load)
        b.load_snapshot(str(tmp_path / f"snap{m_save}"))
        b.run(18)
        _same(ref, _packed(b))


def _pblup_data():
    D = RP.PBLUP_DATA
    return dict(ID=np.array([r[0] for r in D]), Dam=np.array([r[2] for r in D]), BW=np.array([r[5] for r in D]))


@pytest.mark.parametrize("snp", [False, True], ids=["pblup", "ped_plus_snp"])
def test_runLMEM_on_the_documentation_example(ngp, O, tmp_path, snp):
    from nextgp_jl_amd import api
    data = _pblup_data()
    ped = tmp_path / "pedigreeBase.txt"
    ped.write_text("#Pedigree for the above example\n" + "\n".join(" ".join(r) for r in RP.PBLUP_PED) + "\n")
    VCV = {"ID": api.Random("A", 150.0), "e": api.Random("I", 350.0)}
    formula = "BW ~ 1 + PED(ID)"
    P, vm = 64, 0.5
    if snp:   # every column a permutation of 0 0 0 1 1 1 1 2 2 2: its mean is 1, the centred codes are exact in fp32
        rng = np.random.default_rng(2)
        M = np.column_stack([rng.permutation([0, 0, 0, 1, 1, 1, 1, 2, 2, 2]) for _ in range(P)]).astype(np.float64)
        np.save(str(tmp_path / "g.npy"), M)
        formula += ' + SNP(M1, "%s")' % str(tmp_path / "g.npy")
        VCV["M1"] = api.BayesPR(9999, vm)
    out = str(tmp_path / "out")
    res = api.runLMEM(formula, data, 8, 2, 2, outFolder=out, VCV=VCV, userPedData=str(ped), seed=1)
    ids = [r[0] for r in RP.PBLUP_PED]
    with open(os.path.join(out, "uIDOut")) as f:
        lines = f.read().rstrip("\n").split("\n")
    assert lines[0].split("\t") == ids and len(lines) == 1 + 3
    with open(os.path.join(out, "varUIDOut")) as f:
        assert f.readline().rstrip("\n") == "ID"
    rr = res["random"]["ID"]
    assert rr["levels"] == ids and len(rr["u"]) == 14
    assert np.allclose(api.summaryMCMC("uID", outFolder=out)[0], rr["u"], rtol=1e-12, atol=1e-12)
    assert np.allclose(api.summaryMCMC("varUID", outFolder=out)[0, 0], rr["varU"], rtol=1e-12)
    # the reference's order of operations with the same K
    _, Kc = ngp.pedigree_ainv(*RP.pblup_sire_dam())
    level = np.array([ids.index(a) for a in data["ID"]])
    ref = RR.RandomRefChain(O, (M - 1.0) if snp else np.zeros((10, 1)), data["BW"], seed=1, chain=0)
    ref.add_random(level, 14, RP.csr_dense(*Kc), df=4.0, scale=75.0, v=150.0)
    if snp:
        ref.add_set(0, P, 0, 4.0, vm * 0.5, [(0, P)], [vm])
    ref.E_df, ref.E_scale = 4.0, 175.0
    ref.run(8)
    smp = res["sampler"]
    tol = lambda a, b: np.abs(np.asarray(a) - np.asarray(b)).max() <= 1e-9 * max(1e-6, np.abs(np.asarray(b)).max())
    a, g = smp.get_state(), smp.get_random(0)
    assert tol(g["u"], ref.u[0]) and abs(g["varU"] - ref.varU[0]) <= 1e-9 * ref.varU[0]
    assert tol(a["ycorr"], ref.ycorr) and abs(a["varE"] - ref.varE) <= 1e-9 * ref.varE and abs(a["b"] - ref.b[0]) <= 1e-9 * abs(ref.b[0])
    if snp:
        assert tol(a["beta"][:P], ref.state()["beta"]) and sorted(res["sets"]) == ["M1"]
    else:
        assert not [f for f in os.listdir(out) if f.startswith(("beta", "delta"))]


def test_runLMEM_two_ped_terms_and_chains(ngp, tmp_path):
    """PED(ID) + PED(Dam) + (1|Dam) of the documentation: two sets over the same A^-1, every dam a known animal; two chains."""
    from nextgp_jl_amd import api
    VCV = {"ID": api.Random("A", 150.0), "Dam": api.Random("A", 90.0), "1|Dam": api.Random("I", 40.0), "e": api.Random("I", 350.0)}
    res = api.runLMEM("BW ~ 1 + PED(ID) + PED(Dam) + (1|Dam)", _pblup_data(), 10, 2, 2, outFolder=str(tmp_path / "o"), VCV=VCV,
                      userPedData=RP.PBLUP_PED, chains=2)
    assert sorted(res["random"]) == ["1 | Dam", "Dam", "ID"]
    assert len(res["random"]["Dam"]["u"]) == 14 and len(res["random"]["1 | Dam"]["u"]) == 4
    for c in (0, 1):
        assert os.path.exists(os.path.join(str(tmp_path / "o"), f"chain{c}", "uDamOut"))
    assert not np.array_equal(res["chains"][0]["random"]["ID"]["u"], res["chains"][1]["random"]["ID"]["u"])


def test_refusals_leave_things_running(ngp, O, tmp_path):
    from nextgp_jl_amd import api
    X, y, v, animal, K = _chain_problem(ngp, O)
    s = _chain(ngp, X, y, v, animal, K, 0)
    for bad in (3, -1):
        with pytest.raises(ngp.NextGPHipError, match="0 automatic, 1 serial"):
            s.set_random_schedule(0, bad)
    with pytest.raises(ngp.NextGPHipError, match="unknown random-effect set"):
        s.set_random_schedule(1, 2)
    assert s.get_random_schedule(0)["engine"] in (1, 2)                 # the refused calls left the automatic choice in force
    s.run(3)
    d = ngp.Sampler(device=0, seed=1, chain=0)
    d.set_records(200)
    did = d.add_random_set(animal, 300)                                 # the identity: no Gauss-Seidel to schedule
    with pytest.raises(ngp.NextGPHipError, match="off-diagonal"):
        d.set_random_schedule(did, 2)
    assert d.get_random_schedule(did) == dict(engine=0, depths=1, launches=0)
    d.set_y(y); d.run(2)
    data = _pblup_data()
    with pytest.raises(ValueError, match="userPedData"):
        api.runLMEM("BW ~ 1 + PED(ID)", data, 6, 2, 2, outFolder=str(tmp_path / "a"))
    with pytest.raises(ValueError, match="needs a pedigree"):
        api.runLMEM('BW ~ 1 + (1|Dam) + SNP(M, "%s")' % _npy(tmp_path, np.random.default_rng(1).integers(0, 3, size=(10, 64)).astype(np.float64)), data, 6, 2, 2, outFolder=str(tmp_path / "b"),
                    VCV={"1|Dam": api.Random("A", 1.0)})
    unknown = dict(data, ID=np.array(["0"] + list(data["ID"][1:])))
    with pytest.raises(NotImplementedError, match="all-zero row"):
        api.runLMEM("BW ~ 1 + PED(ID)", unknown, 6, 2, 2, outFolder=str(tmp_path / "c"), userPedData=RP.PBLUP_PED)
    res = api.runLMEM("BW ~ 1 + PED(ID)", data, 6, 2, 2, outFolder=str(tmp_path / "d"), userPedData=RP.PBLUP_PED,
                      VCV={"ID": api.Random("A", 150.0)})
    assert res["nKept"] == 2 and np.all(np.isfinite(res["random"]["ID"]["u"]))
    s.run(1)


def _npy(tmp_path, M):
    p = str(tmp_path / "geno.npy")
    np.save(p, M)
    return p
