"""Single-step GBLUP on the host side: A22 by Colleau's method (ngp_pedigree_a22) against the dense tabular route, the level renumbering
and the permuted A^-1, the hybrid step restated in Python (tests/ref_singlestep.py) against the dense restatement on the embedded K,
runLMEM's refusals, and the ABI.  No GPU."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from ngp_pkg import load_pkg  # noqa: E402

ngp = load_pkg()
from nextgp_jl_amd import api  # noqa: E402

import ref_gblup as RG  # noqa: E402
import ref_pedigree as RP  # noqa: E402
import ref_random as RR  # noqa: E402
import ref_singlestep as RS  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _built():
    import __graft_entry__ as g
    g.build()


PEDS = {"inbred60": lambda: RP.inbred_pedigree(60), "random300": lambda: RP.random_pedigree(300, 20)}
_dense = {}


def _ped(name):
    if name not in _dense:
        s, d = PEDS[name]()
        _dense[name] = (s, d, api.makeA(s, d), ngp.pedigree_ainv(s, d))
    return _dense[name]


@pytest.mark.parametrize("subset", [1, 7, "all"])
@pytest.mark.parametrize("name", list(PEDS))
def test_a22_against_the_dense_route(name, subset):
    """The entries of A are dyadic rationals that both methods represent exactly at these depths; 1e-12 covers the order of sums."""
    s, d, A, (F, _) = _ped(name)
    n = len(s)
    rng = np.random.default_rng(5)
    idx = np.arange(n) if subset == "all" else rng.choice(n, size=subset, replace=False)   # (not sorted: any order is allowed)
    A22 = ngp.pedigree_a22(s, d, F, idx)
    err = np.abs(A22 - A[np.ix_(idx, idx)]).max()
    print(f"{name} subset {subset}: max |A22 - A[idx, idx]| = {err:.3e}")
    assert err <= 1e-12
    assert np.array_equal(A22, A22.T)
    if subset != "all":
        assert np.abs(RS.colleau_a22(s, d, F, idx) - A22).max() <= 1e-12       # the plain restatement of the method


def test_a22_refusals():
    s, d, _, (F, _) = _ped("inbred60")
    with pytest.raises(ngp.NextGPHipError, match="outside"):
        ngp.pedigree_a22(s, d, F, [3, 60])
    bad = s.copy(); bad[0] = 5
    with pytest.raises(ngp.NextGPHipError, match="in front of"):
        ngp.pedigree_a22(bad, d, F, [3])
    with pytest.raises(ValueError):
        ngp.pedigree_a22(s, d, F, [])


@pytest.mark.parametrize("name", list(PEDS))
def test_renumbering_and_the_permuted_csr(name):
    s, d, A, (F, Ainv) = _ped(name)
    n = len(s)
    gpos = np.random.default_rng(8).choice(n, size=11, replace=False)          # in the genotypes' row order, not sorted
    perm = api.single_step_order(n, gpos)
    assert sorted(perm.tolist()) == list(range(n))
    assert perm[n - 11:].tolist() == gpos.tolist()                              # the genotyped animals last, in ids order
    head = perm[:n - 11]
    assert np.all(np.diff(head) > 0) and not set(head.tolist()) & set(gpos.tolist())   # the others first, in pedigree order
    assert np.array_equal(perm, RS.renumber(n, gpos))
    kp, kc, kv = api.permute_csr(Ainv, perm)
    assert kp[0] == 0 and kp[-1] == Ainv[0][-1]
    for l in range(n):
        assert np.all(np.diff(kc[kp[l]:kp[l + 1]]) > 0)                         # columns ascending
    K, K0 = RP.csr_dense(kp, kc, kv), RP.csr_dense(*Ainv)
    assert np.array_equal(K, K.T)
    P = np.zeros((n, n)); P[np.arange(n), perm] = 1.0
    assert np.array_equal(K, P @ K0 @ P.T)                                      # (a permutation moves values, it rounds nothing)


def _hybrid_problem(hd, nd, nrec, seed, weighted):
    """A pedigree's A^-1 over q = hd + nd animals with the last nd `genotyped`, and a D of the size G_w^-1 - A22^-1 has."""
    q = hd + nd
    rng = np.random.default_rng(seed)
    s, d = RP.random_pedigree(q, max(2, q // 6), seed=seed)
    F, Ainv = ngp.pedigree_ainv(s, d)
    gpos = np.sort(rng.choice(q, size=nd, replace=False))
    perm = api.single_step_order(q, gpos)
    S = api.permute_csr(Ainv, perm)
    B = rng.normal(size=(nd, nd + 3))
    Gw = B @ B.T / (nd + 3) + 0.05 * np.eye(nd)
    A22 = ngp.pedigree_a22(s, d, F, gpos)
    D = np.linalg.inv(0.9 * Gw + 0.1 * A22) - np.linalg.inv(A22)
    D = (D + D.T) / 2.0
    level = rng.integers(0, q, size=nrec)
    w = rng.uniform(0.3, 3.0, nrec) if weighted else None
    return q, S, D, level, w, rng.normal(size=nrec) * 3.0, rng.normal(size=q)


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("hd,nd", [(1, 1), (5, 63), (70, 65)])
def test_hybrid_restatement_against_the_dense_one(O, hd, nd, weighted):
    """Same level order, same draw keys, hence the same chain as the dense engine on K = S + embed(D): 1e-9 relative over 3 steps."""
    q, S, D, level, w, y, u = _hybrid_problem(hd, nd, 90, 3 + hd, weighted)
    rows = RP.csr_rows(*S)
    K = RS.embed(rows, q, nd, D)
    assert np.array_equal(K, K.T)
    rs = np.sqrt(w) if weighted else None
    zpz = RR.zpz_of(level, q, w)
    ya, ua, va = (y * rs if weighted else y), u, 0.8
    yb, ub, vb = ya, ua, va
    for it in (1, 2, 3):
        ya, ua, va = RS.hybrid_step(O, 77, 2, it, 1, ya, None if rs is None else list(rs), level, q, rows, nd, D, zpz, ua, va, 1.3, 4.0, 0.4)
        yb, ub, vb = RG.dense_step_blocked(O, 77, 2, it, 1, yb, rs, level, q, K, zpz, ub, vb, 1.3, 4.0, 0.4)
        eu, ev, ey = np.abs(ua - ub).max() / np.abs(ub).max(), abs(va - vb) / vb, np.abs(ya - yb).max() / np.abs(yb).max()
        print(f"hd={hd} nd={nd} it={it}: rel err u {eu:.2e} varU {ev:.2e} ycorr {ey:.2e}")
        assert eu <= 1e-9 and ev <= 1e-9 and ey <= 1e-9


def test_hybrid_restatement_without_a_head_is_the_dense_one_bit_for_bit(O):
    nd = 70
    rng = np.random.default_rng(2)
    B = rng.normal(size=(nd, 2 * nd))
    T = np.linalg.inv(B @ B.T / nd); T = (T + T.T) / 2.0
    level = rng.integers(0, nd, size=50)
    zpz = RR.zpz_of(level, nd, None)
    y, u = rng.normal(size=50), rng.normal(size=nd)
    a = RS.hybrid_step(O, 5, 0, 1, 0, y, None, level, nd, [[] for _ in range(nd)], nd, T, zpz, u, 0.7, 1.1, 4.0, 0.3)
    b = RG.dense_step_blocked(O, 5, 0, 1, 0, y, None, level, nd, T, zpz, u, 0.7, 1.1, 4.0, 0.3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_h_inverse_is_the_inverse_of_h():
    """H = [A11 + A12 A22^-1 (G_w - A22) A22^-1 A21, A12 A22^-1 G_w; ., G_w] (Legarra et al. 2009): ref_singlestep.h_inverse inverts it."""
    s, d, A, _ = _ped("inbred60")
    n = len(s)
    idx = np.array([50, 7, 33, 58, 21])
    rng = np.random.default_rng(1)
    B = rng.normal(size=(5, 40))
    G = B @ B.T / 40 + 0.001 * np.eye(5)
    w = 0.05
    A22 = A[np.ix_(idx, idx)]
    Gw = (1 - w) * G + w * A22
    rest = np.array([i for i in range(n) if i not in set(idx.tolist())])
    A12, iA22 = A[np.ix_(rest, idx)], np.linalg.inv(A22)
    H = np.zeros((n, n))
    H[np.ix_(rest, rest)] = A[np.ix_(rest, rest)] + A12 @ iA22 @ (Gw - A22) @ iA22 @ A12.T
    H[np.ix_(rest, idx)] = A12 @ iA22 @ Gw
    H[np.ix_(idx, rest)] = H[np.ix_(rest, idx)].T
    H[np.ix_(idx, idx)] = Gw
    Hi = RS.h_inverse(A, G, idx, w)
    assert np.abs(Hi @ H - np.eye(n)).max() <= 1e-8


def _pblup_data():
    D = RP.PBLUP_DATA
    return dict(ID=np.array([r[0] for r in D]), Dam=np.array([r[2] for r in D]), BW=np.array([r[5] for r in D]))


def test_runLMEM_single_step_refusals_before_any_device(tmp_path):
    data = _pblup_data()
    geno = np.random.default_rng(1).integers(0, 3, size=(3, 40)).astype(np.uint8)
    ss = {"ID": {"geno": geno, "ids": ["QGG5", "QGG9", "QGG12"], "w": 0.05}}
    H = {"ID": api.Random("H", 150.0)}
    run = lambda sub, formula="BW ~ 1 + PED(ID)", **kw: api.runLMEM(formula, data, 6, 2, 2, outFolder=str(tmp_path / sub), userPedData=RP.PBLUP_PED, **kw)
    with pytest.raises(ValueError, match="needs singleStep"):
        run("a", VCV=H)
    with pytest.raises(ValueError, match="needs singleStep"):
        run("a2", VCV=H, singleStep={})
    with pytest.raises(ValueError, match="is not Random"):
        run("b", VCV={"ID": api.Random("A", 150.0)}, singleStep=ss)
    with pytest.raises(ValueError, match="is not Random"):
        run("b2", singleStep=ss)
    with pytest.raises(ValueError, match="no PED"):
        run("b3", VCV=H, singleStep=dict(ss, Sire=ss["ID"]))
    with pytest.raises(ValueError, match="QGG99 is not in the pedigree"):
        run("c", VCV=H, singleStep={"ID": dict(ss["ID"], ids=["QGG5", "QGG99", "QGG12"])})
    with pytest.raises(ValueError, match="QGG5 is listed twice"):
        run("d", VCV=H, singleStep={"ID": dict(ss["ID"], ids=["QGG5", "QGG9", "QGG5"])})
    with pytest.raises(ValueError, match="rows for 2 ids"):
        run("e", VCV=H, singleStep={"ID": dict(ss["ID"], ids=["QGG5", "QGG9"])})
    for w in (-0.1, 1.0, float("nan")):
        with pytest.raises(ValueError, match=r"\[0, 1\)"):
            run("f", VCV=H, singleStep={"ID": dict(ss["ID"], w=w)})
    with pytest.raises(ValueError, match="valid method"):
        run("g", VCV={"ID": api.Random("H", 150.0, type=3)}, singleStep=ss)
    with pytest.raises(NotImplementedError, match="Tuple"):
        run("h", formula="BW ~ 1 + PED(ID) + PED(Dam)", VCV={("ID", "Dam"): api.Random("H", np.array([[2.0, 0.5], [0.5, 1.0]]))})
    with pytest.raises(NotImplementedError, match="summaryStat"):
        run("i", VCV=H, singleStep=ss, summaryStat={"ID": ([0.0], [1.0])})
    assert not [p for p in os.listdir(str(tmp_path)) if os.listdir(str(tmp_path / p))]     # nothing was written


def test_symbols_header_and_abi_version():
    new = ["ngp_pedigree_a22", "ngp_grm_single_step", "ngp_add_random_set_hybrid"]
    with open(os.path.join(ROOT, "include", "nextgp_hip.h")) as f:
        hdr = f.read()
    lib = ngp.load()
    for s in new:
        assert s in ngp.SYMBOLS and re.search(r"\bint32_t\s+%s\s*\(" % s, hdr) and hasattr(lib, s)
    assert re.search(r"#define\s+NGP_ABI_VERSION\s+4\b", hdr) and lib.ngp_abi_version() == 4
    for s in ("single_step_order", "permute_csr", "single_step_terms", "pedigree_a22"):
        assert hasattr(ngp, s)
    assert hasattr(ngp.Sampler, "add_random_set_hybrid") and hasattr(ngp.Sampler, "grm_single_step")
