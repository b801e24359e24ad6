"""What a handle carries from one call to the next.  Almost every other GPU test builds a fresh handle, configures it once, runs it and
compares; a host drives ONE long-lived handle through many calls.  Here a handle is used the second way:

1. settings changed between the runs of one chain -- the form of the block chain (ngp_set_chain_form), fine-seam calls between runs,
   the Gauss-Seidel engine of a random-effect set, observers (traced loci, the sample file, genomic variance, the prediction panel)
   switched on, off or replaced -- leave the chain the one the setting in force describes, and observers leave it alone;
2. a second chain on a used handle (ngp_set_y again) is the chain of a fresh handle: the bytes of its snapshot, and every getter the
   snapshot does not carry.

Every comparison is bit for bit.  The builders are those of the other test modules."""
import os

import numpy as np
import pytest

import ref_pedigree as RP
from conftest import add_sets, make_problem
from test_gpu_bayesrc import PI4, VC4, make_annot
from test_gpu_compact import make_codes
from test_gpu_direct_quads import KNOB_WITHHELD, N_TALL, P_TALL, _direct_as_reported
from test_gpu_gblup import _spd_K
from test_gpu_pedigree import _chain as ped_chain, _chain_problem as ped_problem
from test_gpu_sampler_waits import _device as _device_w
from test_gpu_singlestep import _chain as hybrid_chain, _problem as hybrid_problem
from test_gpu_threshold import classes_of
from test_gpu_tuple import ENGINES, oracle_like
from test_gpu_warm_helper import KNOB_NO_WARMER, _warmer_as_placed
from test_tuple_main_oracle import add_tuple, tuple_problem

pytestmark = pytest.mark.gpu

KNOB_GRAM_MFMA = 1 << 10   # ngp_debug_set_knob: the Gram window on the matrix cores (read when a panel is built)
SEG = 4          # iterations per segment; every schedule here is (n_total, 2, 2): kept draws fall into every segment
_made = {}


def _eq(a, b, what=None):
    """every entry of dict a, bit for bit, in dict b (the oracle may pad an array beyond the sampler's)"""
    for k, x in a.items():
        x, z = np.asarray(x), np.asarray(b[k])
        if x.ndim == 1 and z.ndim == 1 and len(z) > len(x):
            z = z[:len(x)]
        assert x.shape == z.shape and np.array_equal(x, z), (what, k)


def _same_bytes(pa, pb):
    with open(pa, "rb") as f:
        a = f.read()
    with open(pb, "rb") as f:
        b = f.read()
    if a != b:
        n = min(len(a), len(b))
        first = next((i for i in range(n) if a[i] != b[i]), n)
        raise AssertionError(f"files differ: {len(a)} and {len(b)} bytes, first difference at byte {first}")


# ---- 1a. the form of the block chain, switched between the runs of one chain ---------------------------------------------------------
FORM_ENGINES = {"blocklaunch": (dict(mode=0, lag=1), 0), "persist_lag4": (dict(mode=1, lag=4), 0), "rows_lag4": ENGINES["rows_lag4"]}
SEQUENCES = {"1_0_1": (1, 0, 1), "0_1_0": (0, 1, 0), "1_0_0_1": (1, 0, 0, 1)}
FORM_MODELS = ["all_pr", "pr_b_r", "tuple_b", "lv_pr"]


def _form_model(O, ngp, name):
    """(panel, y, add(m)): all_pr -- every block linear (lin_all); pr_b_r -- linear blocks beside stepping ones, one block shared by two
    sets and a partial last block; tuple_b -- a Tuple set's blocks (linear, one step per locus) and a BayesB set; lv_pr -- a BayesLV set
    (its sweep is BayesPR's) sharing a block with a BayesPR set.  The C oracle carries the first three."""
    if name not in _made:
        if name == "tuple_b":
            X, y, vm, v, span, off = tuple_problem(O, ngp, 300, 75, 2, extra=40)

            def add(m):
                add_tuple(m, 75, 2, vm, [(0, 25), (25, 75)])
                add_sets(m, [(off, 40, "B")], v)
        else:
            X, y, _, v = make_problem(O, 300, {"all_pr": 200, "pr_b_r": 328, "lv_pr": 250}[name], seed=4)
            if name == "lv_pr":
                cov = np.column_stack([np.ones(150), np.arange(150) % 2])

                def add(m):
                    m.add_marker_set_lv(0, 150, v, cov, 0.5, est_mode=1)
                    add_sets(m, [(150, 100, "PR")], v)
            else:
                spec = [(0, 120, "PR"), (120, 80, ("PRw", 16))] if name == "all_pr" else [(0, 128, "PR"), (128, 100, "B"), (228, 100, "R")]

                def add(m):
                    add_sets(m, spec, v)
        _made[name] = (X, y, add)
    return _made[name]


@pytest.mark.parametrize("seq", list(SEQUENCES))
@pytest.mark.parametrize("model", FORM_MODELS)
@pytest.mark.parametrize("engine", list(FORM_ENGINES))
def test_chain_form_switched_between_runs(ngp, O, tmp_path, engine, model, seq):
    """ngp_set_chain_form between two ngp_run calls: every segment runs the form in force, and ngp_get_chain_form says which.  Expected:
    the blocked oracle given Oracle.set_tform at the same iterations; for the BayesLV model (the oracle has none) fresh handles, one per
    segment, built under that segment's form and joined by snapshots."""
    forms = SEQUENCES[seq]
    n = SEG * len(forms)
    X, y, add = _form_model(O, ngp, model)
    kw, shards = FORM_ENGINES[engine]

    def start(form):
        s = ngp.Sampler(device=0, seed=21, chain=0, **kw)
        s.set_chain_form(form)
        if shards:
            s.set_max_shards(shards)
        s.set_panel(X)
        add(s)
        s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var()); s.set_schedule(n, 2, 2)
        return s

    a = start(forms[0])
    lv = model == "lv_pr"
    if not lv:
        e = oracle_like(O, a, X)
        add(e)
        e.set_y(y); e.set_residual_prior(4.0, 0.25 * y.var()); e.set_schedule(n, 2, 2)
    snap = None
    for i, f in enumerate(forms):
        a.set_chain_form(f)
        assert a.chain_form() == f
        if lv:
            e = start(f)
            if snap:
                e.load_snapshot(snap)
            e.run(SEG)
            snap = os.fspath(tmp_path / f"seg{i}.snap")
            e.save_snapshot(snap)
        else:
            e.set_tform(f)
            e.run(SEG)
        a.run(SEG)
        assert a.chain_form() == f
        _eq(a.get_state(), e.get_state(), (i, f))
        if lv:
            _eq(a.lv_state(0), e.lv_state(0), (i, f))
    assert a.get_state()["iter"] == n
    _eq(a.get_posterior_sums(), e.get_posterior_sums(), "sums")


def test_chain_form_switched_between_fused_runs(ngp, O, tmp_path):
    """Two chains over one panel in ONE fused launch per iteration (ngp_run_many; the fused launch passes the inverse-form table through
    an expression of its own), the form switched 1 -> 0 -> 1 on both: each is the chain of fresh handles, one per segment, joined by
    snapshots."""
    N, P, shards, forms = 408, 512, 6, (1, 0, 1)
    X, y, _, v = make_problem(O, N, P, seed=5)
    n = SEG * len(forms)

    def start(c, form, owner=None):
        s = ngp.Sampler(device=0, seed=1001 + c, chain=c, mode=1, lag=6, streamer=2)
        s.set_chain_form(form)
        if owner is None:
            s.set_max_shards(shards)
            s.set_panel(X)
        else:
            s.share_panel(owner)
        add_sets(s, [(0, 256, "PR"), (256, 256, "B")], v)
        s.set_y(y + 0.01 * c); s.set_residual_prior(4.0, 0.25 * y.var()); s.set_schedule(n, 2, 2)
        return s

    first = start(0, forms[0])
    fused = [first, start(1, forms[0], owner=first)]
    S = first.layout()[1]
    snaps, alone = [None, None], [None, None]
    for i, f in enumerate(forms):
        for s in fused:
            s.set_chain_form(f)
        ngp.Sampler.run_many(fused, SEG)
        assert first.census()["grid"] == 2 * (1 + (S + 31) // 32) + S      # one grid for both chains
        for c in range(2):
            e = start(c, f)
            assert e.layout() == first.layout()
            if snaps[c]:
                e.load_snapshot(snaps[c])
            e.run(SEG)
            snaps[c] = os.fspath(tmp_path / f"c{c}_seg{i}.snap")
            e.save_snapshot(snaps[c])
            assert fused[c].chain_form() == f
            _eq(fused[c].get_state(), e.get_state(), (i, f, c))
            alone[c] = e
    for c in range(2):
        _eq(fused[c].get_posterior_sums(), alone[c].get_posterior_sums(), ("sums", c))


# ---- 1b. fine-seam calls between the runs of a chain --------------------------------------------------------------------------------
@pytest.mark.parametrize("dev", [False, True], ids=["host_arrays", "device_arrays"])
def test_fine_seam_calls_between_runs(ngp, O, dev):
    """Handle A runs a chain under form 1 and, between its runs, sweeps set 0 and set 1 over the caller's arrays (ngp_sweep_set,
    ngp_sweep_set_dev): the table of linear blocks is rebuilt for set 0, for set 1 and for the whole model in turn.  What the calls
    return is what they return on a handle that makes nothing but these calls, in the same order.  The fine seam works in the handle's
    own chain arrays (docs/HISTORY.md, open finding), so A takes ngp_get_state in front of the calls and puts it back with
    ngp_set_state behind them, as include/nextgp_hip.h advises: with that, every segment of A's chain and its posterior sums are those
    of a handle that never made a fine-seam call -- which also needs the run behind the calls to rebuild the table for the whole model
    (left at set 0, where the lanes of set 1 count as inactive, the BayesB blocks would take the inverse form)."""
    N, spec = 300, [(0, 128, "PR"), (128, 100, "B")]
    X, y, _, v = make_problem(O, N, 228, seed=4)

    def start():
        s = ngp.Sampler(device=0, seed=21, chain=0)
        s.set_chain_form(1)
        s.set_panel(X)
        add_sets(s, spec, v)
        s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var()); s.set_schedule(4 * SEG, 2, 2)
        return s

    def arrays(s):
        return dict(ycorr=y - y.mean(), beta=[np.zeros(128), np.zeros(100)], varBeta=[np.full(1, v), np.full(100, v)],
                    piHat=[None, s.get_state()["piHat"][2:4].copy()])

    def fine(s, w, sid):
        if not dev:
            delta = s.sweep_set(sid, 1.3, w["ycorr"], w["beta"][sid], w["varBeta"][sid], w["piHat"][sid])
            return dict(ycorr=w["ycorr"].copy(), beta=w["beta"][sid].copy(), varBeta=w["varBeta"][sid].copy(), delta=delta)
        import torch
        t = {k: torch.tensor(x, device="cuda", dtype=torch.float64) for k, x in (("ycorr", w["ycorr"]), ("beta", w["beta"][sid]), ("varBeta", w["varBeta"][sid]))}
        d = torch.zeros(len(w["beta"][sid]), device="cuda", dtype=torch.int64)
        p = None if w["piHat"][sid] is None else torch.tensor(w["piHat"][sid], device="cuda", dtype=torch.float64)
        torch.cuda.synchronize()
        s.sweep_set_dev(sid, 1.3, t["ycorr"].data_ptr(), t["beta"].data_ptr(), t["varBeta"].data_ptr(), d.data_ptr(), 0 if p is None else p.data_ptr())
        w["ycorr"][:] = t["ycorr"].cpu().numpy(); w["beta"][sid][:] = t["beta"].cpu().numpy(); w["varBeta"][sid][:] = t["varBeta"].cpu().numpy()
        if p is not None:
            w["piHat"][sid][:] = p.cpu().numpy()
        return dict(ycorr=w["ycorr"].copy(), beta=w["beta"][sid].copy(), varBeta=w["varBeta"][sid].copy(), delta=d.cpu().numpy())

    a, only, plain = start(), start(), start()
    wa, wo = arrays(a), arrays(only)
    for seg, order in enumerate(((0, 1), (1, 0), (0, 1), ())):
        a.run(SEG); plain.run(SEG)           # (after the calls of the segment before: the table built for one set has to go)
        keep = a.get_state()
        _eq(keep, plain.get_state(), ("chain", seg))
        for sid in order:
            ra, ro = fine(a, wa, sid), fine(only, wo, sid)
            assert np.abs(ra["beta"]).max() > 0
            _eq(ra, ro, (seg, sid))
            if wa["piHat"][sid] is not None:
                assert np.array_equal(wa["piHat"][sid], wo["piHat"][sid]), (seg, sid)
        if order:
            assert a.get_state()["varE"] == 1.3          # the calls worked in the handle's chain arrays ...
            a.set_state(keep)                            # ... and ngp_set_state puts the chain back
    _eq(a.get_posterior_sums(), plain.get_posterior_sums(), "sums")
    assert a.chain_form() == 1 and a.get_state()["iter"] == 4 * SEG


# ---- 1c. the Gauss-Seidel engine of a random-effect set, switched mid-chain -----------------------------------------------------------
def _random_everything(s):
    out = {"st_" + k: x for k, x in s.get_state().items()}
    out.update({"rnd_" + k: x for k, x in s.get_random(0).items()})
    out.update({"ps_" + k: x for k, x in s.get_posterior_sums().items()})
    return out


@pytest.mark.parametrize("kind", ["csr_pedigree", "hybrid_70_65"])
def test_random_engine_switched_between_runs(ngp, O, kind):
    """ngp_set_random_schedule 1 -> 2 -> 1 between the runs of one chain: the serial and the level-scheduled engine draw the same bits,
    so the chain is the one that stayed on the serial engine."""
    if kind == "csr_pedigree":
        X, y, v, animal, K = ped_problem(ngp, O)

        def start():
            return ped_chain(ngp, X, y, v, animal, K, 1)
    else:
        pr = hybrid_problem(ngp, O, 70, 65)
        rng = np.random.default_rng(2)
        level = rng.integers(0, pr["q"], size=160)
        y = rng.normal(size=160) * 2.0 + 3.0

        def start():
            s = hybrid_chain(ngp, pr, level, y, pr["D"])
            s.set_random_schedule(0, 1)
            return s
    a, stay = start(), start()
    for s in (a, stay):
        s.set_schedule(3 * SEG, 2, 2)
    for seg, mode in enumerate((1, 2, 1)):
        a.set_random_schedule(0, mode)
        assert a.get_random_schedule(0)["engine"] == mode and stay.get_random_schedule(0)["engine"] == 1
        a.run(SEG); stay.run(SEG)
        _eq(_random_everything(a), _random_everything(stay), (seg, mode))
    assert np.abs(a.get_random(0)["u"]).max() > 0 and a.get_posterior_sums()["nKept"] == (3 * SEG - 2) // 2


# ---- 1d. knobs that change timing only, toggled between the runs of one chain ----------------------------------------------------------
def test_timing_knobs_toggled_between_runs(ngp, O):
    """225 shards of 160 rows on the row-owning streamer: the smallest shape of this suite at which the library, with no knob set, lets
    the row waves load quads themselves and offers the warmer role (tests/test_gpu_direct_quads.py, tests/test_gpu_warm_helper.py).
    Between the runs of handle A the knob goes 0 -> direct quads withheld -> warmer withheld -> 0, and bit 10 (the Gram window on the
    matrix cores, which A's panel was built under) is cleared and set again; the census of every segment says whether the feature was
    on.  The chain is the one of the handle that never had a knob.  (One engine: beside the phase streamer and byte tiles neither
    feature is offered, and a knob that selects nothing tests nothing.)"""
    nb = P_TALL // 64
    a = _device_w(ngp, O, N_TALL, P_TALL, 6, 225, None, "PR", knob=KNOB_GRAM_MFMA)
    plain = _device_w(ngp, O, N_TALL, P_TALL, 6, 225, None, "PR")
    assert a.layout() == plain.layout() == (160, 225, nb) and a.streamer() == (2, 7)
    for s in (a, plain):
        s.set_schedule(4 * SEG, 2, 2)
    for seg, knob in enumerate((0, KNOB_WITHHELD, KNOB_NO_WARMER | KNOB_GRAM_MFMA, 0)):
        a.debug_set_knob(knob)
        a.run(SEG); plain.run(SEG)
        _direct_as_reported(a, not (knob & KNOB_WITHHELD), nb=nb)
        _warmer_as_placed(a, candidate=not (knob & KNOB_NO_WARMER), nb=nb)
        _direct_as_reported(plain, True, nb=nb)
        _eq(a.get_state(), plain.get_state(), (seg, knob))
    _eq(a.get_posterior_sums(), plain.get_posterior_sums(), "sums")


# ---- 1e. observers switched on, off or replaced mid-chain -----------------------------------------------------------------------------
def test_observers_switched_mid_chain_leave_the_chain_alone(ngp, O, tmp_path):
    """Traced loci, the sample file, genomic variance (its windows replaced while it is off) and the prediction panel (replaced by one of
    another row count) come and go between the runs of handle A; its chain and marker posterior sums are those of a handle that never
    had an observer.  What the observers report after being switched back on is what include/nextgp_hip.h says: traces and sample
    records cover the runs that follow the call; enabling genomic variance zeroes its sums; a prediction panel loaded mid-chain, and one
    that replaces it, start the prediction sums at zero while nKept stays the chain's count."""
    N, P, n = 300, 328, 4 * SEG
    spec = [(0, 100, "PR"), (100, 92, "B"), (256, 72, "R")]
    G, y, v = make_codes(O, N, P)
    Gp1, Gp2 = make_codes(O, 37, P)[0], make_codes(O, 50, P)[0]
    W1, W2 = [(0, 1), (60, 70), (90, 100)], [(5, 40), (64, 100)]

    def start():
        s = ngp.Sampler(device=0, seed=1001, chain=0)
        s.set_panel(G, centre=True)
        add_sets(s, spec, v)
        return s

    def begin(s):
        s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var()); s.set_schedule(n, 2, 2)

    a, plain = start(), start()
    a.set_variance_windows(0, W1); a.enable_genomic_variance(True, 0.05, 8)
    a.set_trace_loci([3, 150, 300], 2)
    f1, f2 = os.fspath(tmp_path / "one.ngpsmp"), os.fspath(tmp_path / "two.ngpsmp")
    a.set_sample_file(f1)
    begin(a); begin(plain)

    def segment(niter, what):
        a.run(niter); plain.run(niter)
        st = a.get_state()
        _eq(st, plain.get_state(), what)
        return st

    # segment 1 (iterations 1-4, kept: 4): everything on
    st = segment(SEG, "seg1")
    tr = a.get_trace_ext(SEG)
    assert np.array_equal(tr["beta"][-1], st["beta"][[3, 150, 300]]) and np.array_equal(tr["varBeta"][-1], st["varBeta"][:2])
    assert a.genomic_variance_sums()["nKept"] == 1
    # segment 2 (5-8, kept: 6, 8): other loci, the file closed, genomic variance off, a first prediction panel (the chain has a kept draw)
    a.set_trace_loci([7, 200], 0)
    a.set_sample_file(None)
    a.enable_genomic_variance(False)
    a.set_prediction_panel(Gp1, centre=True)
    smp = ngp.read_sample_file(f1)
    assert smp["iter"].tolist() == [4] and np.array_equal(smp["beta"][0], st["beta"])

    def one_draw_since_the_panel_came(rows, nkept):
        ps, last = a.prediction_sums(), a.prediction_last()
        assert ps["sum"].shape == (4, rows) and ps["nKept"] == nkept == a.get_posterior_sums()["nKept"]   # (nKept: the chain's, not the panel's)
        assert np.abs(last).max() > 0 and np.array_equal(ps["sum"], last) and np.array_equal(ps["sum2"], last * last)
        return last

    st = segment(2, "seg2a")
    last = one_draw_since_the_panel_came(37, 2)
    st = segment(2, "seg2b")
    tr = a.get_trace_ext(2)
    assert tr["beta"].shape == (2, 2) and np.array_equal(tr["beta"][-1], st["beta"][[7, 200]])
    assert np.array_equal(a.prediction_sums()["sum"], last + a.prediction_last())
    assert ngp.read_sample_file(f1)["iter"].tolist() == [4]               # the closed file stays closed
    # segment 3 (9-12, kept: 10, 12): no traced loci, a new file, genomic variance on again with other windows, another prediction panel
    a.set_trace_loci([], 0)
    a.set_variance_windows(0, W2)
    a.enable_genomic_variance(True, 0.05, 8)
    a.set_sample_file(f2)
    a.set_prediction_panel(Gp2, centre=True)
    segment(2, "seg3a")
    one_draw_since_the_panel_came(50, 4)
    st = segment(2, "seg3b")
    gs = a.genomic_variance_sums()
    Vt, rt = a.genomic_variance_trace()
    assert gs["nKept"] == 2 and Vt.shape == (2, len(W2) + 3 + 1)           # enabling zeroed the sums: the draws of this segment only
    assert np.array_equal(gs["sumV"], Vt[0] + Vt[1]) and np.array_equal(gs["last"], Vt[1]) and gs["ratio"][0] == rt[0] + rt[1]
    # ... and they are the draws 10 and 12 of a chain that had these windows from the start
    w2 = start()
    w2.set_variance_windows(0, W2); w2.enable_genomic_variance(True, 0.05, 8)
    begin(w2)
    w2.run(3 * SEG)
    V2, r2 = w2.genomic_variance_trace()
    assert V2.shape[0] == 5 and np.array_equal(Vt, V2[3:5]) and np.array_equal(rt, r2[3:5])
    # segment 4 (13-16): everything off
    a.set_sample_file(None)
    a.enable_genomic_variance(False)
    smp = ngp.read_sample_file(f2)
    assert smp["iter"].tolist() == [10, 12] and np.array_equal(smp["beta"][-1], st["beta"]) and np.array_equal(smp["delta"][-1], st["delta"])
    segment(SEG, "seg4")
    _eq(a.get_posterior_sums(), plain.get_posterior_sums(), "sums")
    assert a.get_posterior_sums()["nKept"] == 7


# ---- 2. a second chain on a used handle ----------------------------------------------------------------------------------------------
SCHED = (12, 4, 2)
ZERO = ("sum", "nkept", "n_fit", "count", "ratio", "iter", "traced", "tries", "accepted")   # names of sums and counters in everything()


class ModelG:
    """Gaussian trait with markers: a Tuple set (k = 2), BayesPR, BayesB, BayesR with 12 classes, a BayesLV and a BayesRCpi set; a
    fixed-effect set of two columns; an identity, a pedigree (CSR) and a correlated (Tuple) random-effect set; a hold-out set; a
    prediction panel, traced loci and a sample file; and either residual weights or genomic variance with windows (the library
    refuses the two together)."""
    N, NLOC, reads_y = 300, 40, True

    def __init__(self, O, ngp, variant):
        self.ngp, self.variant = ngp, variant
        key = "model_g"
        if key not in _made:
            X, y, vm, v, span, off = tuple_problem(O, ngp, self.N, self.NLOC, 2, extra=284)
            rng = np.random.default_rng(12)
            s_, d_ = RP.random_pedigree(300, 60, seed=3)
            _, K = ngp.pedigree_ainv(s_, d_)
            animal = rng.integers(40, 300, size=self.N)
            dam = d_[animal].astype(np.int64) - 1
            _made[key] = dict(X=X, y=y, vm=vm, v=v, off=off, Xf=rng.normal(size=(self.N, 2)), herd=rng.integers(0, 12, size=self.N), animal=animal,
                              levels=np.stack([animal, dam]), K=K, V=np.array([[0.5, -0.1], [-0.1, 0.3]]) * y.var(), w=rng.uniform(0.3, 3.0, self.N),
                              H=np.arange(5, self.N, 9).astype(np.int64), Xp=np.asfortranarray(X[::7][:37]),
                              cov=np.column_stack([np.ones(70), np.arange(70) % 2]), annot=make_annot(64, 3, seed=9))
        self.d = _made[key]
        self.y1 = self.d["y"]
        self.y2 = self.d["y"][::-1] * 1.1 + 0.5
        self.prior = (4.0, 0.25 * float(self.d["y"].var()))

    def build(self, tmp_path, tag):
        d, ngp, off, v = self.d, self.ngp, self.d["off"], self.d["v"]
        s = ngp.Sampler(device=0, seed=31, chain=1)
        if self.variant == "weights":
            s.set_residual_weights(d["w"])
        s.set_panel(d["X"])
        add_tuple(s, self.NLOC, 2, d["vm"], [(0, 15), (15, self.NLOC)])
        add_sets(s, [(off, 50, "PR"), (off + 50, 40, "B"), (off + 90, 60, "R12")], v)
        self.lv = s.add_marker_set_lv(off + 150, 70, v, d["cov"], 0.5, est_mode=1)
        self.rc = s.add_marker_set_rc(off + 220, 64, 4.0, v * 0.5, v, VC4, PI4, d["annot"], estPi=True)
        s.add_fixed_set(d["Xf"])
        s.add_random_set(d["herd"], 12, df=4.0, scale=0.25 * d["y"].var(), varU0=0.5 * d["y"].var())
        s.add_random_set(d["animal"], 300, K=d["K"], df=4.0, scale=0.25 * d["y"].var(), varU0=0.5 * d["y"].var())
        s.add_random_set_tuple(d["levels"], 300, K=d["K"], varU0=d["V"])
        s.set_holdout(d["H"])
        if self.variant == "genvar":
            s.set_variance_windows(0, [(0, 1), (60, 70)]); s.set_variance_windows(2, [(3, 40)])
            s.enable_genomic_variance(True, 0.05, 8)
        s.set_prediction_panel(d["Xp"])
        s.set_trace_loci([3, 130, 400], 3)
        s.sample_path = os.fspath(tmp_path / f"{tag}.ngpsmp")
        s.set_sample_file(s.sample_path)
        return s

    def everything(self, s):
        out = {"st_" + k: x for k, x in s.get_state().items()}
        out.update({"ps_" + k: x for k, x in s.get_posterior_sums().items()})
        out.update({"fx_" + k: x for k, x in s.get_fixed().items()})
        for r in range(3):
            out.update({f"rnd{r}_" + k: x for k, x in s.get_random_tuple(r).items()})
        out.update({"lv_" + k: x for k, x in s.lv_state(self.lv).items()})
        out.update({"rc_" + k: x for k, x in s.rc_state(self.rc).items()})
        out.update({"cls_" + k: x for k, x in s.get_class_state(3).items()})
        out.update({"ho_" + k: x for k, x in s.holdout_state().items()})
        out.update({"pred_" + k: x for k, x in s.prediction_sums().items()})
        if self.variant == "genvar":
            out.update({"gv_" + k: x for k, x in s.genomic_variance_sums().items()})
            out["gv_trace_V"], out["gv_trace_r"] = s.genomic_variance_trace()
            out["gv_traced"] = s.genomic_variance_layout()[3]
        return out

    def traces(self, s, n):
        out = {"tr_" + k: x for k, x in s.get_trace(n).items()}
        out.update({"trx_" + k: x for k, x in s.get_trace_ext(n).items()})
        return out

    def counters(self, s):
        """launches this handle made, over both its chains"""
        c = list(s.prediction_stats())
        return np.array(c + (list(s.genomic_variance_stats()) if self.variant == "genvar" else []))

    def state(self, s):
        return dict(st=s.get_state(), rnd=[s.get_random(0), s.get_random(1)], rt=s.get_random_tuple(2), lv=s.lv_state(self.lv), rc=s.rc_state(self.rc))

    def set_state(self, s, m):
        s.set_state(m["st"])
        for r in (0, 1):
            s.set_random(r, **m["rnd"][r])
        s.set_random_tuple(2, **m["rt"])
        s.set_lv_state(self.lv, m["lv"])
        s.set_rc_state(self.rc, m["rc"])


class ModelR:
    """Records only (ngp_set_records): a dense set of 65 levels, a hybrid set with a head of 70 and a dense block of 65 levels under the
    level-scheduled head engine, censored records.  (Built from the parts -- test_gpu_singlestep._problem, test_gpu_gblup._spd_K -- and
    not by test_gpu_liability.small: that helper calls ngp_set_y itself, over a marker panel, and the sample file has to be set first.)"""
    N, reads_y = 160, True
    variant = None

    def __init__(self, O, ngp, variant=None):
        self.ngp = ngp
        self.pr = hybrid_problem(ngp, O, 70, 65)
        rng = np.random.default_rng(2)
        self.l65, self.l135 = rng.integers(0, 65, size=self.N), rng.integers(0, self.pr["q"], size=self.N)
        self.K65 = _spd_K(65)
        self.y1 = rng.normal(size=self.N) * 2.0 + 3.0
        self.y2 = rng.normal(size=self.N) * 1.5 - 1.0
        self.rows = np.arange(0, self.N, 3).astype(np.int64)
        self.prior = (4.0, 1.0)

    def build(self, tmp_path, tag):
        s = self.ngp.Sampler(device=0, seed=13, chain=2)
        s.set_records(self.N)
        s.add_random_set_dense(self.l65, 65, K=self.K65, df=4.0, scale=0.5, varU0=1.0)
        rid = s.add_random_set_hybrid(self.l135, self.pr["q"], self.pr["S"], 65, D=self.pr["D"], df=4.0, scale=0.5, varU0=1.0)
        s.set_random_schedule(rid, 2)
        assert s.get_random_schedule(rid)["engine"] == 2
        s.set_censored(self.rows, np.full(len(self.rows), -1.5), np.full(len(self.rows), np.inf))
        s.sample_path = os.fspath(tmp_path / f"{tag}.ngpsmp")
        s.set_sample_file(s.sample_path)
        return s

    def everything(self, s):
        out = {"st_" + k: x for k, x in s.get_state().items()}
        out.update({"ps_" + k: x for k, x in s.get_posterior_sums().items()})
        for r in range(2):
            out.update({f"rnd{r}_" + k: x for k, x in s.get_random(r).items()})
        out.update({"lb_" + k: x for k, x in s.liability_state().items()})
        return out

    def traces(self, s, n):
        return {"tr_" + k: x for k, x in s.get_trace(n).items()}

    def counters(self, s):
        return np.array([s.liability_fallthrough()])


class ModelT:
    """Threshold trait of three classes over byte tiles: a hold-out set (in front of the classes), Cowles' threshold step with the
    proposal SD adapted during burn-in (sigma = 0), class probabilities, a BayesPR and a BayesB set.  (Built from make_codes and
    classes_of, the parts of test_gpu_threshold.small / ordinal, and not by them: they call ngp_set_y themselves and add one BayesPR set
    over fp32 tiles, where this model needs byte tiles, a second set and the sample file in front of ngp_set_y.)"""
    N, P, reads_y = 150, 192, False      # (a threshold trait reads y nowhere: its second chain repeats the first)
    variant = None

    def __init__(self, O, ngp, variant=None):
        self.ngp = ngp
        self.G, y, v = make_codes(O, self.N, self.P)
        self.v = v / float(y.var())
        self.cls = classes_of(y, 3)
        self.H = np.arange(3, self.N, 5).astype(np.int64)
        self.y1, self.y2 = np.zeros(self.N), np.ones(self.N)     # (a threshold trait reads y nowhere)
        self.prior = (4.0, 0.25)

    def build(self, tmp_path, tag):
        s = self.ngp.Sampler(device=0, seed=1001, chain=0, storage="u8")
        s.set_panel(self.G, centre=True)
        add_sets(s, [(0, 100, "PR"), (100, 92, "B")], self.v)
        s.set_holdout(self.H)
        s.set_classes(self.cls, 3)
        s.set_threshold_step("cowles", 0.0)
        s.enable_class_probabilities()
        s.sample_path = os.fspath(tmp_path / f"{tag}.ngpsmp")
        s.set_sample_file(s.sample_path)
        return s

    def everything(self, s):
        out = {"st_" + k: x for k, x in s.get_state().items()}
        out.update({"ps_" + k: x for k, x in s.get_posterior_sums().items()})
        out.update({"lb_" + k: x for k, x in s.liability_state().items()})
        out.update({"ho_" + k: x for k, x in s.holdout_state().items()})
        ts = s.threshold_step()
        out.update(ts_sigma=ts["sigma"], ts_tries=ts["tries"], ts_accepted=ts["accepted"], sum_prob=s.class_probability_sums())
        return out

    def traces(self, s, n):
        return {"tr_" + k: x for k, x in s.get_trace(n).items()}

    def counters(self, s):
        return np.array([s.liability_fallthrough()])

    def state(self, s):
        return dict(st=s.get_state(), lb=s.liability_state(), ts=s.threshold_step())

    def set_state(self, s, m):
        s.set_state(m["st"])
        s.set_liability_state(m["lb"])
        s.set_threshold_step_state(m["ts"])


def _sample_records(ngp, path):
    smp = ngp.read_sample_file(path)
    smp.pop("sets")
    return smp


def _tail(x, n):
    if isinstance(x, list):
        return [_tail(e, n) for e in x]
    if isinstance(x, dict):
        return {k: _tail(e, n) for k, e in x.items()}
    return x[-n:]


def _flat(x, pre=""):
    if not isinstance(x, (dict, list)):
        return {pre: x}
    out = {}
    for k, e in (x.items() if isinstance(x, dict) else enumerate(x)):
        out.update(_flat(e, f"{pre}{k}."))
    return out


CASES = {"G_weights": (ModelG, "weights", False), "G_genvar": (ModelG, "genvar", False), "R_records": (ModelR, None, False), "T_threshold": (ModelT, None, False),
         "G_genvar_setters": (ModelG, "genvar", True), "T_threshold_setters": (ModelT, None, True)}


@pytest.mark.parametrize("case", list(CASES))
def test_set_y_again_starts_the_chain_of_a_fresh_handle(ngp, O, tmp_path, case):
    """Handle A runs a whole chain on y1 (burn-in and kept draws), then ngp_set_y(y2) and the schedule, and a second chain; handle B is
    fresh (same seed and chain) and runs on y2 only.  Right after the second ngp_set_y A reads as B does after its first -- every sum and
    counter zero -- and after the run the two agree in the bytes of their snapshots (derived from the one state table: every
    registered segment, with seed, chain and the sets' call counters; nothing in the file differs legitimately between two such handles,
    so the whole file is compared), in every getter the snapshot does not carry and in the records of their sample files.  The
    *_setters cases also drop the mid-chain state of a third handle into A and B through the setters before the run: get -> set on a
    used handle is get -> set on a fresh one."""
    cls, variant, setters = CASES[case]
    M = cls(O, ngp, variant)
    n = SCHED[0]

    def begin(s, y):
        s.set_y(y); s.set_schedule(*SCHED)

    a = M.build(tmp_path, "a")
    a.set_residual_prior(*M.prior)
    begin(a, M.y1)
    a.run(n)
    used = M.everything(a)
    assert used["ps_nKept"] == 4 and used["st_iter"] == n
    c1 = M.counters(a)
    begin(a, M.y2)                                   # between the chains: ngp_set_y and the schedule, nothing else
    b = M.build(tmp_path, "b")
    b.set_residual_prior(*M.prior)
    begin(b, M.y2)
    za, zb = M.everything(a), M.everything(b)
    _eq(za, zb, "after set_y")
    for k, x in za.items():
        if any(z in k.lower() for z in ZERO):
            assert not np.any(x), k
    left = n
    if setters:
        c = M.build(tmp_path, "c")
        c.set_residual_prior(*M.prior)
        begin(c, M.y2)
        c.run(n // 2)
        mid = M.state(c)
        M.set_state(a, mid); M.set_state(b, mid)
        _eq(M.everything(a), M.everything(b), "after the setters")
        left = n - n // 2
    a.run(left); b.run(left)
    ea, eb = M.everything(a), M.everything(b)
    assert ea["st_iter"] == n and (setters or ea["ps_nKept"] == 4)
    assert np.array_equal(ea["st_ycorr"], used["st_ycorr"]) == (not M.reads_y)   # (a chain that reads y is another chain now)
    _eq(ea, eb, "after the run")
    _eq(M.traces(a, left), M.traces(b, left), "traces")
    assert np.array_equal(M.counters(a) - c1, M.counters(b))          # (launch counters are the handle's, over both chains)
    pa, pb = os.fspath(tmp_path / "a.snap"), os.fspath(tmp_path / "b.snap")
    a.save_snapshot(pa); b.save_snapshot(pb)
    _same_bytes(pa, pb)
    a.set_sample_file(None); b.set_sample_file(None)
    ra, rb = _sample_records(ngp, a.sample_path), _sample_records(ngp, b.sample_path)
    nrec = len(rb["iter"])
    assert nrec == (3 if setters else 4) and len(ra["iter"]) == 4 + nrec          # A's file goes on behind the records of its first chain
    _eq(_flat(_tail(ra, nrec)), _flat(rb), "sample records")
