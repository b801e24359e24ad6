"""APY GBLUP on the device: the column-panel builder (ngp_grm_begin_apy, ngp_grm_apy), the pieces, and the random-effect set whose
non-core levels are drawn in one pass over P (ngp_add_random_set_apy, k_apy_tail).  Yardstick: tests/ref_apy.py, plain fp64 with
derived forward-error bounds; comparisons to rounding use RA.TOL x the bound."""
import numpy as np
import pytest

import ref_apy as RA
import ref_gblup as RG
import ref_random as RR

pytestmark = pytest.mark.gpu

NSNP = 300


def _apy_set(ngp, M, nc, method=1, w=None, seed=77, chain=2):
    N = M.shape[0]
    s = ngp.Sampler(device=0, seed=seed, chain=chain)
    if w is not None:
        s.set_residual_weights(w)
    s.set_records(N)
    s.grm_begin_apy(N, nc, method); s.grm_columns(M); s.grm_end(); s.grm_apy()
    form = s.grm_get_apy()
    rid = s.add_random_set_apy(None, N, nc, df=4.0, scale=0.4, varU0=0.8)
    return s, rid, form


def _chain(s, y):
    s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var()); s.set_schedule(6, 0, 1)
    return s


def _same(a, b):
    ga, gb = a.get_random(0), b.get_random(0)
    assert np.array_equal(ga["u"], gb["u"]) and ga["varU"] == gb["varU"]
    assert np.array_equal(a.get_state()["ycorr"], b.get_state()["ycorr"])


@pytest.mark.parametrize("N", [64, 130])
def test_all_core_is_the_dense_set(ngp, O, N):
    """nc = N, an empty tail: the seeded chain and the variance step give the bits of the dense set over ngp_grm_invert of the same G."""
    M = RG.hw_genotypes(O, N, NSNP, seed=N)
    y = np.random.default_rng(N).normal(size=N) * 2.0 + 5.0
    a = _chain(_apy_set(ngp, M, N, seed=31, chain=1)[0], y)
    b = ngp.Sampler(device=0, seed=31, chain=1)
    b.set_records(N)
    b.grm_begin(N, 1); b.grm_columns(M); b.grm_end(); b.grm_invert()
    b.add_random_set_dense(None, N, df=4.0, scale=0.4, varU0=0.8)
    _chain(b, y)
    a.run(6); b.run(6)
    _same(a, b)
    a.close(); b.close()


@pytest.mark.parametrize("N,nc,method,twin", [(70, 64, 1, False), (70, 64, 2, False), (200, 64, 1, False), (200, 130, 1, False), (1100, 192, 1, False),
                                              (2120, 2049, 1, False), (200, 64, 1, True)])
def test_one_step_against_ref_apy(ngp, O, N, nc, method, twin):
    """One step from a non-zero u against ref_apy.step on the device's own pieces; the step repeated on a fresh handle gives the same bits.
    The pieces themselves are checked against ref_apy.pieces by test_pieces, at (200, 130) and (1100, 192): here they are exact inputs, so a
    wrong P would show only through s and u_n.
    (2120, 2049): the instantiation of k_apy_tail for cores above 2,048.  twin: weighted residuals, and a dense set over the assembled K_APY
    with the same seed and set id draws the same u to rounding (the sum of the two sets' bounds)."""
    M = RG.hw_genotypes(O, N, NSNP, seed=N + nc)
    rng = np.random.default_rng(N + method)
    w = rng.uniform(0.3, 3.0, N) if twin else None
    rs = np.sqrt(w) if twin else None
    y0, u0 = rng.normal(size=N) * 3.0, rng.normal(size=N)
    zpz = RR.zpz_of(np.arange(N), N, w)
    out = []
    for rep in range(2):
        s, rid, pc = _apy_set(ngp, M, nc, method, w)
        ycorr, u = y0.copy(), u0.copy()
        varU = s.sample_random_set(rid, 1.3, ycorr, u, 0.8)
        out.append((ycorr, u, varU, s.grm_get_apy("s", rid), s.grm_get_apy("uKu", rid)))
        s.close()
    for x, z in zip(out[0], out[1]):
        assert np.array_equal(x, z)
    ycorr, u, varU, sd, uKu = out[0]
    ref = RA.step(O, 77, 2, 1, rid, y0 * rs if twin else y0, rs, None, pc, zpz, u0, 0.8, 1.3, 4.0, 0.4)
    yref, byt = (ref["yt"] / rs, ref["byt"] / rs) if twin else (ref["yt"], ref["byt"])
    for name, got, want, b in (("u_c", u[:nc], ref["u"][:nc], ref["bu"][:nc]), ("u_n", u[nc:], ref["u"][nc:], ref["bu"][nc:]), ("s", sd, ref["s"], ref["bs"]),
                               ("uKu", uKu, ref["uKu"], ref["buKu"]), ("ycorr", ycorr, yref, byt), ("varU", varU, ref["varU"], ref["bvarU"])):
        r = np.max(np.abs(got - want) / b)
        print(f"apy step N={N} nc={nc} method={method} {name}: max err / bound = {r:.3e}")
        assert r <= RA.TOL, name
    if twin:
        t = ngp.Sampler(device=0, seed=77, chain=2)
        t.set_residual_weights(w); t.set_records(N)
        assert t.add_random_set_dense(None, N, K=RA.assemble(pc), df=4.0, scale=0.4, varU0=0.8) == rid
        yd, ud = y0.copy(), u0.copy()
        t.sample_random_set(rid, 1.3, yd, ud, 0.8)
        r = np.max(np.abs(ud - u) / (2.0 * ref["bu"]))
        print(f"apy against the dense set over K_APY: max |du| / (sum of bounds) = {r:.3e}")
        assert r <= RA.TOL
        t.close()


@pytest.mark.parametrize("N,nc", [(200, 130), (1100, 192)])
def test_pieces(ngp, O, N, nc):
    """(1100, 192): more than one 64-row tile of non-core rows in the two matrix-core products."""
    M = RG.hw_genotypes(O, N, NSNP, seed=9)
    s, _, got = _apy_set(ngp, M, nc)
    ref = RA.pieces(M, nc)
    for k in ("P", "m", "Kcc"):
        r = np.max(np.abs(got[k] - ref[k]) / ref["b" + k])
        print(f"apy pieces {k}: max err / bound = {r:.3e}")
        assert r <= RA.TOL, k
    assert np.array_equal(got["Kcc"], got["Kcc"].T)
    s.close()
    # a non-core copy of a core animal: m = r (2 a + r) / (a + r) < 2 r given that animal alone (r the 0.001 ridge, a = G_00 - r), and
    # conditioning on the rest of the core only lowers it -- positive because of the ridge, which must be enough
    M2 = M.copy(); M2[N - 1] = M2[0]
    s, _, got = _apy_set(ngp, M2, nc)
    assert 0.0 < got["m"][-1] < 0.002
    s.close()


@pytest.mark.parametrize("shared", [False, True], ids=["own_form", "shared_form"])
def test_state_round_trip(ngp, O, shared):
    """3 iterations, the state through ngp_get_random / ngp_set_random into a fresh handle, 3 more: the bits of 6 uninterrupted ones (the
    seed s is derived state and must follow u).  shared_form: the fresh handle takes the form of the first chain's set by reference."""
    N, nc = 200, 64
    M = RG.hw_genotypes(O, N, NSNP, seed=4)
    y = np.random.default_rng(8).normal(size=N) * 2.0 + 5.0
    a = _chain(_apy_set(ngp, M, nc, seed=31, chain=1)[0], y); a.run(6)
    b = _chain(_apy_set(ngp, M, nc, seed=31, chain=1)[0], y); b.run(3)
    if shared:
        c = ngp.Sampler(device=0, seed=31, chain=1)
        c.set_records(N)
        c.add_random_set_apy(None, N, nc, K=(a, 0), df=4.0, scale=0.4, varU0=0.8)
        _chain(c, y)
    else:
        c = _chain(_apy_set(ngp, M, nc, seed=31, chain=1)[0], y)
    c.set_state(b.get_state()); c.set_random(0, **b.get_random(0)); c.run(3)
    _same(a, c)
    for s in (a, b, c):
        s.close()


def test_makeG_core(ngp, O):
    """api.makeG(M, core=[...]): the pieces over the renumbered animals reassemble to ref_apy's K_APY of the permuted genotypes."""
    N, core = 90, [70, 3, 41, 8, 55]
    M = RG.hw_genotypes(O, N, NSNP, seed=6)
    got = ngp.makeG(M, core=core)
    assert got["nc"] == 5 and got["order"][:5].tolist() == core
    ref = RA.pieces(M[got["order"]], 5)
    Kref, K = RA.assemble(ref), RA.assemble(got)
    bd = ref["bm"] / ref["m"] ** 2 + RA.EPS * ref["d"]
    aP, ad = np.abs(ref["P"]), ref["d"]
    boff = bd[:, None] * aP + ad[:, None] * ref["bP"] + RA.EPS * ad[:, None] * aP
    bound = np.block([[ref["bKcc"], boff.T], [boff, np.diag(bd) + (1 - np.eye(N - 5))]])   # (off the diagonal of D both are exact zeros)
    assert np.all(np.abs(K - Kref) <= RA.TOL * bound)


def test_runLMEM_apy(ngp, O, tmp_path):
    """runLMEM(..., apy={"M1": core}): the levels are renumbered core first, the files and res carry the records' names in that order, and
    the chain is the one built by hand over the permuted genotypes."""
    import os
    N, core = 90, [70, 3, 41, 8, 55]
    M = RG.hw_genotypes(O, N, NSNP, seed=6)
    y = np.random.default_rng(5).normal(size=N) + 10.0
    v = ve = 0.5 * y.var()
    np.save(str(tmp_path / "g.npy"), M)
    out = str(tmp_path / "o")
    res = ngp.runLMEM('y ~ 1 + SNP(M1, "%s")' % (tmp_path / "g.npy"), dict(y=y), 20, 4, 2, outFolder=out, seed=1,
                      VCV={"M1": ngp.Random("G", v), "e": ngp.Random("I", ve)}, apy={"M1": core})
    order, nc = ngp.api.apy_order(N, core)
    names = [f"Ind{i + 1}" for i in order]
    assert res["random"]["M1"]["levels"] == names and names[:5] == ["Ind71", "Ind4", "Ind42", "Ind9", "Ind56"]
    with open(os.path.join(out, "uM1Out")) as f:
        assert f.readline().rstrip("\n").split("\t") == names
    s = ngp.Sampler(device=0, seed=1, chain=0)
    s.set_records(N); s.set_residual_prior(4.0, ve * 2.0 / 4.0)
    s.grm_begin_apy(N, nc, 1); s.grm_columns(M[order]); s.grm_end(); s.grm_apy()
    level = np.empty(N, dtype=np.int32); level[order] = np.arange(N)
    s.add_random_set_apy(level, N, nc, df=4.0, scale=v * 2.0 / 4.0, varU0=v)
    s.set_y(y); s.set_schedule(20, 4, 2); s.run(20)
    assert np.array_equal(s.get_random(0)["sum_u"] / 8, res["random"]["M1"]["u"])
    s.close()
