"""Adding marker sets (include/nextgp_hip.h ngp_add_marker_set*, DESIGN.md "how a marker set is registered"): one model that goes through
every adder -- BayesPR with two regions, a Tuple set, BayesR, BayesRCpi, BayesLV, BayesB -- on N = 200, P = 256 (fp32 tiles).  A refused
call must leave no trace in the handle, a set must start the way ngp_set_y restarts it, and the cap of 16 sets must hold for every adder."""
import numpy as np
import pytest

from conftest import make_problem

pytestmark = pytest.mark.gpu

N, P = 200, 256
VC4, PI4 = [0.0, 0.01, 0.1, 1.0], [0.85, 0.10, 0.04, 0.01]      # BayesR on 128..159
VC3, PI3 = [0.0, 0.1, 1.0], [0.8, 0.15, 0.05]                   # BayesRCpi on 160..199, A = 2
ARG = "error -1: "                                               # NGP_ERR_ARG as Sampler._chk words it


def rc_annot(ncol=40):
    an = np.zeros((ncol, 2), dtype=np.int32)
    an[0::3, 0] = 1; an[1::3, 1] = 1; an[2::3, :] = 1           # first, second, both annotations
    return an


def lv_cov(ncol=30):
    rng = np.random.default_rng(8)
    return np.column_stack([np.ones(ncol), rng.normal(size=ncol)])


class Adders:
    """The five adders with the arguments of this model's sets, at any place in the panel."""

    def __init__(self, ngp, s, v):
        self.error, self.s, self.v, self.vm = ngp.NextGPHipError, s, v, v * (0.7 * np.eye(2) + 0.3)

    def pr(self, col0, ncol, regions=None):
        regions = regions or [(0, ncol)]
        return self.s.add_marker_set(col0, ncol, 0, 4.0, self.v * 0.5, regions, [self.v] * len(regions))

    def b(self, col0, ncol):
        return self.s.add_marker_set(col0, ncol, 1, 4.0, self.v * 0.5, [(j, j + 1) for j in range(ncol)], [self.v] * ncol, pi0=0.1, estPi=True)

    def tuple(self, col0, nloc, regions=None):
        return self.s.add_marker_set_tuple(col0, nloc, 2, 5.0, self.vm * 2, regions or [(0, nloc)], self.vm)

    def r(self, col0, ncol, pi=PI4):
        return self.s.add_marker_set_r(col0, ncol, 4.0, self.v * 0.5, self.v, VC4, pi, estPi=True)

    def rc(self, col0, ncol, annot=None):
        return self.s.add_marker_set_rc(col0, ncol, 4.0, self.v * 0.5, self.v, VC3, PI3, rc_annot(ncol) if annot is None else annot, estPi=True)

    def lv(self, col0, ncol, cov=None):
        return self.s.add_marker_set_lv(col0, ncol, self.v, lv_cov(ncol) if cov is None else cov, 0.5, est_mode=1)

    def refused(self, code, match, call):
        with pytest.raises(self.error, match=code + ".*" + match):
            call()

    def refused_by_each(self, col0, ncol, tuple_col0, tuple_nloc, code, match):
        """One refused call per adder: columns col0 .. col0 + ncol - 1, and tuple_nloc pairs of columns from tuple_col0 on."""
        for call in (lambda: self.pr(col0, ncol), lambda: self.tuple(tuple_col0, tuple_nloc), lambda: self.r(col0, ncol),
                     lambda: self.rc(col0, ncol), lambda: self.lv(col0, ncol)):
            self.refused(code, match, call)


def build(ngp, X, v, with_refusals):
    """The model of this file on a fresh handle; with_refusals: one refused call per case between the valid ones."""
    s = ngp.Sampler(device=0, seed=17, chain=2)
    s.set_panel(X)
    a = Adders(ngp, s, v)
    R = with_refusals
    ids = {}
    if R:
        a.refused_by_each(P - 16, 32, 192, 40, ARG, "outside the panel")           # past the end of the panel, before any set exists
        a.refused(ARG, "added with ngp_add_marker_set_r", lambda: s.add_marker_set(0, 64, 3, 4.0, v * 0.5, [(0, 64)], [v]))
    ids["pr"] = a.pr(0, 64, [(0, 40), (40, 64)])
    if R:
        a.refused_by_each(32, 64, 0, 32, ARG, "marker sets overlap")               # columns 32..95; the tuple set: block 0
        a.refused(ARG, "block boundary", lambda: a.tuple(70, 20))
        a.refused(ARG, "regions must cover all loci of the set", lambda: a.tuple(64, 32, [(0, 10), (10, 30)]))
    ids["tuple"] = a.tuple(64, 32)
    if R:
        a.refused(ARG, "BayesR: class probabilities must sum to 1", lambda: a.r(128, 32, pi=[0.75, 0.10, 0.04, 0.01]))
    ids["r"] = a.r(128, 32)
    if R:
        an = rc_annot()
        an[-1, :] = 0
        a.refused(ARG, "BayesRCpi: locus 39 has no annotation", lambda: a.rc(160, 40, an))
        an = rc_annot()
        an[7, 1] = 2
        a.refused(ARG, r"BayesRCpi: annotation entries must be 0 or 1 \(locus 7\)", lambda: a.rc(160, 40, an))
    ids["rc"] = a.rc(160, 40)
    if R:
        cov = lv_cov()
        cov[:, 1] = 0.0                                                            # ridge = min_i |(C'C)_ii| / 10000 = 0: C'C is singular
        a.refused(ARG, "BayesLV: C'C .. ridge. is not positive definite", lambda: a.lv(200, 30, cov))
    ids["lv"] = a.lv(200, 30)
    if R:
        a.refused_by_each(210, 30, 192, 15, ARG, "marker sets overlap")            # the BayesLV set; the tuple set: block 3, the BayesRCpi set
    ids["b"] = a.b(230, 26)
    if R:
        a.refused_by_each(P - 16, 32, 192, 40, ARG, "outside the panel")           # past the end again, with every kind of set in the handle
    return s, ids


def results(s, ids):
    return dict(state=s.get_state(), r=s.get_class_state(ids["r"]), rc_classes=s.get_class_state(ids["rc"]), rc=s.rc_state(ids["rc"]),
                lv=s.lv_state(ids["lv"]), post=s.get_posterior_sums())


def assert_same(a, b, path=""):
    """Bit for bit: np.array_equal on arrays, == on scalars."""
    assert type(a) is type(b), path
    if isinstance(a, dict):
        assert a.keys() == b.keys(), path
        for k in a:
            assert_same(a[k], b[k], path + "/" + k)
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and np.array_equal(a, b), path
    else:
        assert a == b, path


def start_and_run(s, y, niter=4):
    s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var()); s.set_schedule(4, 1, 1)
    s.run(niter)


@pytest.fixture(scope="module")
def problem(O):
    X, y, bt, v = make_problem(O, N, P, seed=4)
    return X, y, v


@pytest.fixture(scope="module")
def clean_run(ngp, problem):
    """Handle B: the valid calls only, then 4 iterations."""
    X, y, v = problem
    s, ids = build(ngp, X, v, with_refusals=False)
    start_and_run(s, y)
    return s, ids, results(s, ids)


def test_refused_calls_leave_no_trace(ngp, problem, clean_run):
    """Handle A gets a refused call per case between the valid ones -- overlap and past-the-end through each adder, and each adder's own
    refusals -- and must then draw the chain of handle B, which never saw them, bit for bit; the set ids are the same too."""
    X, y, v = problem
    _, ids_b, res_b = clean_run
    s, ids_a = build(ngp, X, v, with_refusals=True)
    assert ids_a == ids_b == dict(pr=0, tuple=1, r=2, rc=3, lv=4, b=5)
    start_and_run(s, y)
    res_a = results(s, ids_a)
    assert res_a["state"]["iter"] == 4
    assert len(np.unique(res_a["state"]["delta"][128:200])) >= 2        # the class sets sample
    assert_same(res_a, res_b)


def test_a_set_starts_the_way_it_restarts(problem, clean_run):
    """ngp_set_y on handle B again, with the same y, and the same 4 iterations: the results of the first run, bit for bit."""
    X, y, v = problem
    s, ids, res_first = clean_run
    start_and_run(s, y)
    assert_same(results(s, ids), res_first)


def test_the_cap_holds_for_every_adder(ngp, O):
    """Sixteen one-column BayesPR sets on a P = 64 panel: every adder refuses a seventeenth, and the handle still runs."""
    X, y, bt, v = make_problem(O, N, 64, seed=4)
    s = ngp.Sampler(device=0, seed=17, chain=2)
    s.set_panel(X)
    a = Adders(ngp, s, v)
    for c in range(16):
        assert a.pr(c, 1) == c
    a.refused_by_each(16, 4, 0, 2, ARG, "at most 16 marker sets")
    s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var()); s.set_schedule(2, 0, 1)
    s.run(2)
    st = s.get_state()
    assert st["iter"] == 2 and np.isfinite(st["beta"]).all() and np.any(st["beta"][:16] != 0.0) and not np.any(st["beta"][16:] != 0.0)
