"""Pedigree BLUP on the host side: A^-1 by Henderson's rules (ngp_pedigree_ainv) against the dense tabular route, makePed, PED terms of
the formula, and the level schedule restated in Python (tests/ref_pedigree.py) against the serial restatement, bit for bit.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ngp_pkg import load_pkg  # noqa: E402

ngp = load_pkg()
from nextgp_jl_amd import api  # noqa: E402

import ref_pedigree as RP  # noqa: E402
import ref_random as RR  # noqa: E402


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


PEDS = {"pblup14": RP.pblup_sire_dam, "inbred60": RP.inbred_pedigree}


@pytest.mark.parametrize("name", list(PEDS))
def test_ainv_against_the_dense_route(name):
    s, d = PEDS[name]()
    n = len(s)
    F, (kp, kc, kv) = ngp.pedigree_ainv(s, d)
    A = api.makeA(s, d)
    K = RP.csr_dense(kp, kc, kv)
    atol = 1e-10 * np.abs(K).max()
    assert np.abs(K - np.linalg.inv(A)).max() <= atol
    assert np.abs(K @ A - np.eye(n)).max() <= atol
    assert np.abs(F - (np.diag(A) - 1.0)).max() <= 1e-12
    assert np.array_equal(K, K.T)                                       # exactly symmetric
    assert kp[0] == 0 and kp.dtype == np.int64 and kc.dtype == np.int32
    for l in range(n):
        assert np.all(np.diff(kc[kp[l]:kp[l + 1]]) > 0)                 # columns ascending, none repeated
    if name == "inbred60":
        assert F.max() > 0.9 and np.any((s == d) & (s > 0))             # heavily inbred, with selfings


def test_ainv_count_then_fill_and_refusals():
    import ctypes as C
    lib = ngp.load()
    f = lib.ngp_pedigree_ainv
    s, d = RP.pblup_sire_dam()
    n = len(s)
    p32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    nnz = C.c_int64(-1)
    kp = np.empty(n + 1, dtype=np.int64)
    rc = f(C.c_int64(n), p32(s), p32(d), None, kp.ctypes.data_as(C.POINTER(C.c_int64)), None, None, C.c_int64(0), C.byref(nnz))
    assert rc == -1 and nnz.value == kp[n] > n and "cap" in lib.ngp_last_error(None).decode()
    bad = s.copy(); bad[0] = 5                                          # a parent behind its offspring
    own = s.copy(); own[6] = 7                                          # its own parent
    out = s.copy(); out[8] = n + 1                                      # outside the list
    for sire in (bad, own, out):
        assert f(C.c_int64(n), p32(sire), p32(d), None, None, None, None, C.c_int64(0), C.byref(nnz)) == -1
        with pytest.raises(ngp.NextGPHipError):
            ngp.pedigree_ainv(sire, d)
    assert f(C.c_int64(0), p32(s), p32(d), None, None, None, None, C.c_int64(0), None) == -1


def test_makePed_orders_parents_first(tmp_path):
    rows = list(RP.PBLUP_PED)
    rng = np.random.default_rng(3)
    shuffled = [rows[k] for k in rng.permutation(len(rows))]
    path = tmp_path / "ped.txt"
    path.write_text("#Pedigree for the example\n" + "\n".join("  ".join(r) for r in shuffled) + "\n\n")
    table, (kp, kc, kv) = api.makePed(str(path), [r[0] for r in RP.PBLUP_DATA])
    ids = table["origID"]
    assert sorted(ids) == sorted(r[0] for r in rows) and table["ID"].tolist() == list(range(1, 15))
    byid = {r[0]: r for r in rows}
    for i, a in enumerate(ids):
        for col, p in (("Sire", byid[a][1]), ("Dam", byid[a][2])):
            assert table[col][i] == (0 if p == "0" else ids.index(p) + 1) and table[col][i] <= i
    # stable: an animal whose parents stand in front of it in the file keeps its place among such animals
    filepos = {r[0]: k for k, r in enumerate(shuffled)}
    kept = [a for a in ids if all(p == "0" or filepos[p] < filepos[a] for p in byid[a][1:])]
    assert len(kept) >= 4
    # the file in pedigree order already: nothing moves, and Ainv is the one of the plain list
    t2, (kp2, kc2, kv2) = api.makePed(rows)
    assert t2["origID"] == [r[0] for r in rows]
    F, (kp3, kc3, kv3) = ngp.pedigree_ainv(*RP.pblup_sire_dam())
    assert np.array_equal(kp2, kp3) and np.array_equal(kc2, kc3) and np.array_equal(kv2, kv3) and np.array_equal(t2["F"], F)
    # the shuffled file gives the same matrix up to the permutation of the animals
    K, K2 = RP.csr_dense(kp, kc, kv), RP.csr_dense(kp2, kc2, kv2)
    perm = [t2["pos"][a] for a in ids]
    assert np.allclose(K, K2[np.ix_(perm, perm)], rtol=0, atol=1e-12)
    # an animal moves only because a parent came later: C (parents A, B) in front of them
    t3, _ = api.makePed([("C", "A", "B"), ("A", "0", "0"), ("D", "0", "0"), ("B", "0", "0")])
    assert t3["origID"] == ["A", "B", "C", "D"]


def test_makePed_refusals():
    rows = list(RP.PBLUP_PED)
    with pytest.raises(ValueError, match="phenotyed individuals are not a subset of pedigree"):
        api.makePed(rows, ["QGG5", "QGG99"])
    with pytest.raises(ValueError, match="listed twice"):
        api.makePed(rows + [("QGG5", "0", "0")])
    with pytest.raises(ValueError, match="not listed"):
        api.makePed(rows + [("QGG15", "QGG77", "0")])
    with pytest.raises(ValueError, match="cycle"):
        api.makePed([("A", "B", "0"), ("B", "C", "0"), ("C", "A", "0")])
    with pytest.raises(ValueError, match="cycle"):
        api.makePed([("A", "A", "0")])


def test_parse_formula_takes_ped_terms_with_the_flag():
    p = api.parse_formula('BW ~ 1 + Herds + PED(ID) + (1|Dam) + PED( Dam ) + SNP(M1, "g.txt")', random_effects=True, pedigree=True)
    assert p.ped == ["ID", "Dam"] and p.random == ["Dam"] and p.covariates == ["Herds"]
    assert p.order == [("ped", "ID"), ("1|", "Dam"), ("ped", "Dam"), ("snp", "M1")]
    assert [t.name for t in p[2]] == ["M1"] and p[0] == "BW" and p[1] is True
    assert api.parse_formula("y ~ 1 + x", random_effects=True, pedigree=True).ped == []
    with pytest.raises(NotImplementedError, match="PedigreeBase"):      # without the flag: the refusals as they were
        api.parse_formula("y ~ 1 + PED(ID)", random_effects=True)
    with pytest.raises(NotImplementedError, match="PedigreeBase"):
        api.parse_formula('y ~ 1 + PED(ID) + SNP(M,"g")')
    with pytest.raises(NotImplementedError, match="random_effects=True"):
        api.parse_formula('y ~ 1 + (1|herd) + SNP(M, "g.txt")', pedigree=True)
    with pytest.raises(NotImplementedError):                            # not a column name
        api.parse_formula("y ~ 1 + PED(ID, Dam)", random_effects=True, pedigree=True)


def test_runLMEM_pedigree_refusals_before_any_device(tmp_path):
    data = dict(BW=np.array([r[5] for r in RP.PBLUP_DATA]), ID=np.array([r[0] for r in RP.PBLUP_DATA]))
    with pytest.raises(ValueError, match="userPedData"):
        api.runLMEM("BW ~ 1 + PED(ID)", data, 10, 2, 2, outFolder=str(tmp_path / "a"))
    with pytest.raises(ValueError, match="at least one SNP"):
        api.runLMEM("BW ~ 1", data, 10, 2, 2, outFolder=str(tmp_path / "b"), userPedData=RP.PBLUP_PED)
    unknown = dict(data, ID=np.array(["0"] + [r[0] for r in RP.PBLUP_DATA][1:]))
    with pytest.raises(NotImplementedError, match="all-zero row"):
        api.runLMEM("BW ~ 1 + PED(ID)", unknown, 10, 2, 2, outFolder=str(tmp_path / "c"), userPedData=RP.PBLUP_PED)
    outside = dict(data, ID=np.array(["QGG99"] + [r[0] for r in RP.PBLUP_DATA][1:]))
    with pytest.raises(ValueError, match="not a subset of pedigree"):
        api.runLMEM("BW ~ 1 + PED(ID)", outside, 10, 2, 2, outFolder=str(tmp_path / "d"), userPedData=RP.PBLUP_PED)


def test_schedule_depths_order_plan():
    # a hand-made K: row 3 depends on 1, row 4 on 3, row 2 on 0 -> depths 0 0 1 1 2
    rows = [[(0, 2.0), (2, -1.0)], [(1, 2.0), (3, -1.0)], [(0, -1.0), (2, 2.0)], [(1, -1.0), (3, 2.0), (4, -0.5)], [(3, -0.5), (4, 2.0)]]
    assert RP.depths(rows) == [0, 0, 1, 1, 2]
    order, dptr = RP.schedule(rows)
    assert order == [0, 1, 2, 3, 4] and dptr == [0, 2, 4, 5]
    assert RP.plan(dptr) == [("fused", 0, 3)]
    assert RP.plan([0, 10, 1500, 1510, 1520, 4000, 6000, 6001]) == [("fused", 0, 1), ("wide", 1, 2), ("fused", 2, 4), ("wide", 4, 5),
                                                                    ("wide", 5, 6), ("fused", 6, 7)]
    assert RP.plan([0, 1024]) == [("fused", 0, 1)] and RP.plan([0, 1025]) == [("wide", 0, 1)]
    s, d = RP.pblup_sire_dam()
    _, (kp, kc, kv) = ngp.pedigree_ainv(s, d)
    rr = RP.csr_rows(kp, kc, kv)
    order, dptr = RP.schedule(rr)
    dep = RP.depths(rr)
    assert RP.depths(rr) == [0, 1, 2, 0, 3, 3, 4, 5, 4, 3, 5, 6, 5, 4] and max(np.diff(dptr)) <= 3   # worked by hand: 7 depths
    for l, row in enumerate(rr):                                        # the property the schedule rests on
        assert all(dep[c] < dep[l] for c, _ in row if c < l)
    assert sorted(order) == list(range(14))


def _problem(s, d, nrec, seed):
    n = len(s)
    _, (kp, kc, kv) = ngp.pedigree_ainv(s, d)
    rng = np.random.default_rng(seed)
    level = rng.integers(n // 3, n, size=nrec)                          # the first third of the animals has no records
    return (kp, kc, kv), level, rng.normal(size=nrec), rng.normal(size=n), rng.uniform(0.3, 3.0, nrec)


@pytest.mark.parametrize("name,weighted", [("pblup14", False), ("pblup14", True), ("inbred60", False), ("ped3000", True)])
def test_scheduled_restatement_equals_the_serial_one_bit_for_bit(O, name, weighted, monkeypatch):
    s, d = RP.random_pedigree(3000, 2000) if name == "ped3000" else PEDS[name]()
    n = len(s)
    (kp, kc, kv), level, y, u, w = _problem(s, d, 40 if n < 100 else 600, 7)
    rows = RP.csr_rows(kp, kc, kv)
    if name == "ped3000":
        pl = RP.plan(RP.schedule(rows)[1])
        assert pl[0][0] == "wide" and pl[-1][0] == "fused"              # a multi-workgroup launch followed by fused ones
        monkeypatch.setattr(RR, "csr_of", lambda K, q: rows)            # (the rows as they are, instead of a 3000 x 3000 array)
        K = None
    else:
        K = RP.csr_dense(kp, kc, kv)
    rs = list(np.sqrt(w)) if weighted else None
    zpz = RR.zpz_of(level, n, w if weighted else None)
    yt = y * np.sqrt(w) if weighted else y
    varU = 0.7
    for it in (1, 2):
        a = RR.random_step_blocked(O, 5, 1, it, 0, yt, rs, level, n, K, zpz, u, varU, 1.3, 4.0, 0.4)
        b = RP.random_step_scheduled(O, 5, 1, it, 0, yt, rs, level, n, rows, zpz, u, varU, 1.3, 4.0, 0.4)
        assert a[0] == b[0] and a[1] == b[1] and a[2] == b[2], it
        yt, u, varU = np.array(a[0]), np.array(a[1]), a[2]
