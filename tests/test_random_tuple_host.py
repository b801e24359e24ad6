"""Correlated (Tuple) random-effect sets without a device: the changed restatement is the Gibbs conditional of the model it writes
down (and the reference's literal lines are not), the level schedule over the union pattern, the draw keys, and runLMEM's
handling of a tuple key (refusals, file names, headers) over a stand-in for the sampler."""
import os

import numpy as np
import pytest

import ref_pedigree as RP
import ref_random as RR
import ref_random_tuple as RT

VARE = 1.7
VARU = np.array([[0.9, -0.25], [-0.25, 0.6]])


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.fixture(scope="module")
def ped14(ngp):
    """The 14 animals of the documentation: records of QGG5 .. QGG14 and of two founders (unknown dams), components (ID, Dam)."""
    s, d = RP.pblup_sire_dam()
    _, K = ngp.pedigree_ainv(s, d)
    animal = np.array([0, 2] + list(range(4, 14)))
    levels = np.stack([animal, d[animal].astype(np.int64) - 1])                # dam 0 (unknown) -> -1
    assert (levels[1] < 0).sum() == 2 and (levels[1] >= 0).sum() == 10
    rng = np.random.default_rng(11)
    return dict(q=14, K=RP.csr_dense(*K), rows=RP.csr_rows(*K), levels=levels, u=rng.normal(size=(14, 2)), ycorr=rng.normal(size=12))


def _dense_conditional(l, levels, q, K, u, ycorr):
    """Level l's conditional from the dense mixed-model matrix C = Z'Z / varE + kron(K, inv(varU)), Z = [Z_ID Z_Dam] with column l k + m."""
    k, N = levels.shape
    Z = np.zeros((N, q * k))
    for m in range(k):
        for i in range(N):
            if levels[m, i] >= 0:
                Z[i, levels[m, i] * k + m] = 1.0
    C = Z.T @ Z / VARE + np.kron(K, np.linalg.inv(VARU))
    rhs = Z.T @ (ycorr + Z @ u.ravel()) / VARE                                  # right-hand side of the whole system: Z'y* / varE
    blk = slice(l * k, l * k + k)
    others = np.ones(q * k, dtype=bool)
    others[blk] = False
    cov = np.linalg.inv(C[blk, blk])
    return cov @ (rhs[blk] - C[blk][:, others] @ u.ravel()[others]), cov


def test_the_changed_restatement_is_the_gibbs_conditional(ped14):
    P = ped14
    worst_literal = 0.0
    for l in range(P["q"]):
        mean, cov = _dense_conditional(l, P["levels"], P["q"], P["K"], P["u"], P["ycorr"])
        m1, c1 = RT.conditional_of_level(l, P["levels"], P["q"], P["K"], P["u"], VARU, VARE, P["ycorr"])
        assert _rel(m1, mean) <= 1e-9 and _rel(c1, cov) <= 1e-9, l
        m2, c2 = RT.conditional_of_level(l, P["levels"], P["q"], P["K"], P["u"], VARU, VARE, P["ycorr"], literal=True)
        assert _rel(c2, cov) <= 1e-9
        worst_literal = max(worst_literal, _rel(m2, mean))
    assert worst_literal > 1e-3                                                 # the reference's lines are NOT that conditional here
    same = np.stack([P["levels"][0], P["levels"][0]])                           # ... and are when no record links two levels
    for l in range(P["q"]):
        mean, cov = _dense_conditional(l, same, P["q"], P["K"], P["u"], P["ycorr"])
        m2, c2 = RT.conditional_of_level(l, same, P["q"], P["K"], P["u"], VARU, VARE, P["ycorr"], literal=True)
        m1, _ = RT.conditional_of_level(l, same, P["q"], P["K"], P["u"], VARU, VARE, P["ycorr"])
        assert _rel(m2, mean) <= 1e-9 and _rel(c2, cov) <= 1e-9 and _rel(m1, m2) <= 1e-9, l


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
def test_the_blocked_step_is_a_gauss_seidel_sweep_of_that_conditional(O, ped14, weighted):
    """tuple_step_blocked (the device's order) against a sweep that takes every level's mean and covariance from the dense matrix
    of the (weighted) model and the same keyed normals: 1e-9 relative, two orders of the same arithmetic."""
    P = ped14
    k, q, levels = 2, P["q"], P["levels"]
    N = levels.shape[1]
    w = np.random.default_rng(3).uniform(0.4, 2.5, N) if weighted else np.ones(N)
    rs = np.sqrt(w)
    setup = RT.tuple_setup(levels, q, w if weighted else None)
    yt, u_new, varU_new = RT.tuple_step_blocked(O, 5, 1, 3, 2, P["ycorr"] * rs if weighted else P["ycorr"], list(rs) if weighted else None, levels, q,
                                                P["rows"], setup, P["u"], VARU, VARE, 5.0, VARU * 2.0)
    Z = np.zeros((N, q * k))
    for m in range(k):
        for i in range(N):
            if levels[m, i] >= 0:
                Z[i, levels[m, i] * k + m] = 1.0
    C = Z.T @ (w[:, None] * Z) / VARE + np.kron(P["K"], np.linalg.inv(VARU))
    rhs = Z.T @ (w * (P["ycorr"] + Z @ P["u"].ravel())) / VARE
    u = P["u"].ravel().copy()
    for l in range(q):
        blk = slice(l * k, l * k + k)
        others = np.ones(q * k, dtype=bool)
        others[blk] = False
        cov = np.linalg.inv(C[blk, blk])
        z = np.array([RR.draw(O, 5, 1, 3, RR.KIND_U_NORMAL, (2 << 40) | (l * k + m), 1) for m in range(k)])
        u[blk] = cov @ (rhs[blk] - C[blk][:, others] @ u[others]) + np.linalg.cholesky(cov) @ z
    assert _rel(np.array(u_new).ravel(), u) <= 1e-9
    ycorr_new = np.array(yt) / rs if weighted else np.array(yt)
    assert _rel(ycorr_new, P["ycorr"] + Z @ P["u"].ravel() - Z @ u) <= 1e-9
    V = np.array(varU_new).reshape(k, k)
    assert np.array_equal(V, V.T) or _rel(V, V.T) <= 1e-12
    assert np.all(np.linalg.eigvalsh((V + V.T) / 2) > 0)


def test_depths_come_from_the_union_of_the_patterns(O, ped14):
    P = ped14
    _, _, Wrows = setup = RT.tuple_setup(P["levels"], P["q"])
    assert any(Wrows)                                                           # records do link animals to their dams ...
    dep = RT.union_depths(P["rows"], Wrows)
    assert dep == RP.depths(P["rows"])                                          # ... along entries Henderson's rules put into K already
    assert RT.schedule_of(dep) == tuple(RP.schedule(P["rows"]))
    # K = I: the schedule of K alone is one depth; the record links make it deeper
    q = 9
    rowsI = RR.csr_of(None, q)
    levels = np.array([[3, 4, 5, 6, 7, 8, 8], [0, 1, 3, 3, 6, -1, 7]])
    setupI = RT.tuple_setup(levels, q)
    depI = RT.union_depths(rowsI, setupI[2])
    assert RP.depths(rowsI) == [0] * q and depI == [0, 0, 0, 1, 1, 2, 2, 3, 4]
    rng = np.random.default_rng(2)
    for rows, lv, st, d, qq in ((P["rows"], P["levels"], setup, dep, P["q"]), (rowsI, levels, setupI, depI, q)):
        y0, u0 = rng.normal(size=lv.shape[1]), rng.normal(size=(qq, 2))
        a = RT.tuple_step_blocked(O, 1, 0, 1, 0, y0, None, lv, qq, rows, st, u0, VARU, VARE, 5.0, VARU * 2.0)
        b = RT.tuple_step_blocked(O, 1, 0, 1, 0, y0, None, lv, qq, rows, st, u0, VARU, VARE, 5.0, VARU * 2.0, dep=d)
        assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2]                   # bit for bit: the reordering is exact
        assert np.abs(np.array(a[1]) - u0).max() > 0


def test_every_draw_key_of_a_set_is_distinct():
    k, q, r = 4, 1000, 0
    keys = [(RR.KIND_U_NORMAL, (r << 40) | (l * k + m)) for l in range(q) for m in range(k)]
    keys += [((RR.KIND_U_CHI2, r) if i == 0 else (RT.KIND_U_WISHART, (r << 40) | (i << 4) | j)) for i in range(4) for j in range(i + 1)]
    assert len(keys) == q * k + 10 and len(set(keys)) == len(keys)
    other = 1                                                                   # a scalar set and a tuple set under another id
    scalar = [(RR.KIND_U_NORMAL, (other << 40) | l) for l in range(q * k)] + [(RR.KIND_U_CHI2, other)]
    scalar += [(RT.KIND_U_WISHART, (other << 40) | (i << 4) | j) for i in range(1, 4) for j in range(i + 1)]
    assert not set(keys) & set(scalar) and len(set(scalar)) == len(scalar)
    assert RT.KIND_U_WISHART not in (RR.KIND_U_NORMAL, RR.KIND_U_CHI2) and RT.KIND_U_WISHART > 16   # (kinds 1 .. 16 are taken)
    assert max(i for _, i in keys if i < (1 << 40)) == q * k - 1 < (1 << 40)


class _StandIn:
    """What runLMEM calls on a Sampler, recorded; no library, no device."""
    made = []

    def __init__(self, **kw):
        self.calls, self.randoms, self.N = [], [], 0
        _StandIn.made.append(self)

    def set_records(self, N):
        self.N = N

    def add_random_set_tuple(self, levels, q, K=None, df=None, scale=None, varU0=None):
        self.calls.append(("tuple", np.array(levels), q, K, df, np.array(scale), np.array(varU0)))
        self.tq, self.tk = q, len(levels)
        return len(self.calls) - 1

    def add_random_set(self, level, q, K=None, df=4.0, scale=None, varU0=100.0):
        self.calls.append(("scalar", np.array(level), q))
        return len(self.calls) - 1

    def get_random_tuple(self, set_id):
        q, k = self.tq, self.tk
        return dict(u=np.arange(q * k, dtype=np.float64).reshape(q, k), sum_u=np.ones((q, k)), varU=np.array([[1.0, 2.0], [3.0, 4.0]]),
                    sum_varU=np.eye(k))

    def get_state(self):
        return dict(b=1.0, varE=2.0, beta=np.zeros(0), delta=np.zeros(0), varBeta=np.zeros(0), piHat=np.zeros(0))

    def get_posterior_sums(self):
        return dict(nKept=1, sum_b=1.0, sum_varE=2.0, sum_beta=np.zeros(0), sum_delta=np.zeros(0), sum_varBeta=np.zeros(0), sum_pi=np.zeros(0))

    def __getattr__(self, name):
        return lambda *a, **kw: None


def _data():
    D = RP.PBLUP_DATA
    return dict(ID=np.array([r[0] for r in D]), Dam=np.array([r[2] for r in D]), BW=np.array([r[5] for r in D]))


def test_runLMEM_takes_a_tuple_of_ped_terms(ngp, tmp_path, monkeypatch):
    from nextgp_jl_amd import api
    monkeypatch.setattr(api, "Sampler", _StandIn)
    _StandIn.made.clear()
    V = np.array([[150.0, -40.0], [-40.0, 90.0]])
    data = _data()
    data["Dam"] = np.array(["0"] + list(data["Dam"][1:]))                       # an unknown dam: level -1 in the second component
    out = str(tmp_path / "o")
    res = api.runLMEM("BW ~ 1 + PED(ID) + PED(Dam)", data, 4, 2, 2, outFolder=out, VCV={("ID", "Dam"): api.Random("A", V), "e": api.Random("I", 350.0)},
                      userPedData=RP.PBLUP_PED, samples="text-sync")
    (kind, levels, q, K, df, scale, varU0), = _StandIn.made[0].calls            # ONE set for the two terms
    ids = [r[0] for r in RP.PBLUP_PED]
    assert kind == "tuple" and q == 14 and K is not None and df == 5.0
    assert np.array_equal(scale, V * 2.0) and np.array_equal(varU0, V)          # scale = v (df - k - 1), src/mme.jl:271
    assert levels.shape == (2, 10) and levels[1, 0] == -1 and levels[0].tolist() == [ids.index(a) for a in data["ID"]]
    assert levels[1, 1:].tolist() == [ids.index(a) for a in data["Dam"][1:]]
    files = sorted(os.listdir(out))
    assert files == sorted(["bOut", "varEOut", "uIDOut", "uDamOut", "varU(:ID, :Dam)Out"])
    for nm, col in (("uIDOut", 0), ("uDamOut", 1)):
        lines = open(os.path.join(out, nm)).read().rstrip("\n").split("\n")
        assert lines[0].split("\t") == ids and len(lines) == 1 + 1
        assert [float(x) for x in lines[1].split("\t")] == [float(2 * l + col) for l in range(14)]
    lines = open(os.path.join(out, "varU(:ID, :Dam)Out")).read().rstrip("\n").split("\n")
    assert lines[0].split("\t") == ["ID_Dam_1", "ID_Dam_2", "ID_Dam_3", "ID_Dam_4"]
    assert [float(x) for x in lines[1].split("\t")] == [1.0, 3.0, 2.0, 4.0]     # column by column (src/samplers.jl:74)
    rr = res["random"][("ID", "Dam")]
    assert rr["u"].shape == (2, 14) and rr["varU"].shape == (2, 2) and rr["levels"] == ids
    # "I" keeps the identity over the pedigree's levels
    _StandIn.made.clear()
    api.runLMEM("BW ~ 1 + PED(ID) + PED(Dam)", _data(), 2, 0, 1, outFolder=str(tmp_path / "i"), VCV={("ID", "Dam"): api.Random("I", V)},
                userPedData=RP.PBLUP_PED, samples="none")
    assert _StandIn.made[0].calls[0][3] is None


def test_runLMEM_refusals_for_tuples(ngp, tmp_path, monkeypatch):
    from nextgp_jl_amd import api
    monkeypatch.setattr(api, "Sampler", _StandIn)
    V = np.array([[150.0, -40.0], [-40.0, 90.0]])
    data = _data()
    g = str(tmp_path / "g.npy")
    np.save(g, np.random.default_rng(1).integers(0, 3, size=(10, 64)).astype(np.float64))
    n = [0]

    def run(formula, VCV, **kw):
        n[0] += 1
        return api.runLMEM(formula, data, 4, 2, 2, outFolder=str(tmp_path / f"r{n[0]}"), VCV=VCV, userPedData=RP.PBLUP_PED, samples="none", **kw)

    with pytest.raises(NotImplementedError, match="GBLUP term M"):             # a dense K inside a tuple
        run(f'BW ~ 1 + PED(ID) + SNP(M, "{g}")', {("ID", "M"): api.Random("A", V), "M": api.Random("G", 1.0)})
    with pytest.raises(ValueError, match="Not available to use summary statistics in correlated effects"):
        run("BW ~ 1 + PED(ID) + PED(Dam)", {("ID", "Dam"): api.Random("A", V)}, summaryStat={("ID", "Dam"): (np.zeros(2), np.ones(2))})
    with pytest.raises(NotImplementedError, match="Symbols only"):
        run("BW ~ 1 + PED(ID) + (1|Dam)", {("ID", "1|Dam"): api.Random("A", V)})
    with pytest.raises(ValueError, match="2 x 2 covariance"):
        run("BW ~ 1 + PED(ID) + PED(Dam)", {("ID", "Dam"): api.Random("A", 150.0)})
    with pytest.raises(ValueError, match="needs its PED"):
        run("BW ~ 1 + PED(ID)", {("ID", "Dam"): api.Random("A", V)})
    with pytest.raises(ValueError, match="one or the other"):
        run("BW ~ 1 + PED(ID) + PED(Dam)", {("ID", "Dam"): api.Random("A", V), "Dam": api.Random("A", 90.0)})
    unknown = dict(data, ID=np.array(["0"] + list(data["ID"][1:])))             # outside a tuple a 0 stays refused, with the existing message
    with pytest.raises(NotImplementedError, match="all-zero row"):
        api.runLMEM("BW ~ 1 + PED(ID)", unknown, 4, 2, 2, outFolder=str(tmp_path / "z"), userPedData=RP.PBLUP_PED)
