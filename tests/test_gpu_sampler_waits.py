"""Two waves of the sampler workgroup (role_sampler, ngp_sweep.h) keep memory waits off the block period.  The chain wave (wave 0) takes
over the next block's coefficients AHEAD of its two granule stores of dlt, so that nothing between those stores and the next block's
total waits on memory; the last block of a sweep has no coefficients to take over.  The group-sum wave (wave 2, lag >= 4) keeps the
look at the next accumulator in flight for a block period as eight raw words per lane (plain agent-scope loads; the compiler's wait
stands where the look is examined, behind the next barrier): the request is the wave's last memory operation of a block, a look that
came too early is repeated a block later, a sum that the next block needs is waited for.  The wave stores nothing in its loop: the
block whose accumulator it took goes through an LDS word (ztake, one per block parity) to wave 1, which zeroes the accumulator a
block later.  That hand-over is what the 1-, 2-, 3- and 40-block cases exercise -- no take in the loop, takes up to the last block
but one, two wraps of the 16-slot ring whose slots must be zero again when the block 16 on adds its terms.  Whichever of these paths
a block takes, the chain is the blocked oracle's for the same layout, bit for bit."""
import numpy as np
import pytest

from conftest import add_sets, make_problem
from test_tuple_main_oracle import add_tuple, tuple_problem

pytestmark = pytest.mark.gpu

NITER = 3
KEYS = ("ycorr", "beta", "delta", "varBeta", "piHat")
RELOOK_WORD = (7 << 17) - 3   # NGP_DBG_RELOOK (ngp_sweep_args.h): looks of the last launch that came too early and were repeated
_problems = {}
_references = {}


def _problem(O, N, P):
    """(fp32 panel, genotype codes, y, v) of an N x P problem, made once"""
    if (N, P) not in _problems:
        X, y, bt, v = make_problem(O, N, P, seed=5)
        _, mu = O.generate_panel(N, P)
        G = np.rint(X.astype(np.float64) + mu[None, :]).astype(np.uint8)
        assert G.max() <= 2
        _problems[(N, P)] = (X, G, y, v)
    return _problems[(N, P)]


def _model(m, P, kind, y, v):
    add_sets(m, [(0, P, kind)], v)
    m.set_y(y)
    m.set_residual_prior(4.0, 0.25 * y.var())
    m.set_schedule(NITER, 1, 1)


def _device(ngp, O, N, P, lag, shards, storage, kind, knob=0, streamer=2, near=0, seed=1001, chain=0, y_shift=0.0):
    X, G, y, v = _problem(O, N, P)
    s = ngp.Sampler(device=0, seed=seed, chain=chain, mode=1 if lag else None, lag=lag, streamer=None if storage else streamer, storage=storage)
    s.set_max_shards(shards)
    if near:
        s.set_near(near)
    if knob:
        s.debug_set_knob(knob)
    if storage:
        s.set_panel(G, centre=True)
    else:
        s.set_panel(X)
    _model(s, P, kind, y + y_shift, v)
    return s


def _reference(O, s, N, P, storage, kind, seed=1001, chain=0, y_shift=0.0):
    """state of the blocked oracle after NITER iterations in the layout of handle s; one oracle run per (problem, layout, chain)"""
    R, S, _ = s.layout()
    key = (N, P, storage, kind, R, S, s.config()[1], s.near(), s.streamer()[1], s.chain_form(), seed, chain, y_shift)
    if key not in _references:
        X, G, y, v = _problem(O, N, P)
        o = O.Oracle(order=1, seed=seed, chain=chain)
        if storage:
            o.set_panel_u8(G, R=R, S=S, D=key[6], near=key[7], tform=key[9])
        else:
            o.set_panel_f32(X, R=R, S=S, D=key[6], near=key[7], nchain=key[8], tform=key[9])
        _model(o, P, kind, y + y_shift, v)
        o.run(NITER)
        st = o.get_state()
        for k in KEYS:
            st[k].setflags(write=False)
        _references[key] = st
    return _references[key]


def _same(a, b):
    for k in KEYS:
        assert np.array_equal(a[k], b[k][:len(a[k])]), k
    assert a["varE"] == b["varE"] and a["b"] == b["b"] and a["iter"] == b["iter"] == NITER


@pytest.mark.parametrize("P", [64, 128, 192, 2560], ids=["1_block", "2_blocks", "3_blocks", "40_blocks"])
def test_sweep_lengths(ngp, O, P):
    """One, two and three blocks: the chain wave's last block (no coefficients to take over) is its first, second, third; wave 2 has no
    block to fetch ahead, one (the blocking fetch of block 1), one and a first look.  Forty blocks: two wraps of the 16-slot rings."""
    s = _device(ngp, O, 128, P, 6, 2, None, "PR")
    assert s.layout() == (64, 2, P // 64) and s.config() == (1, 6) and s.streamer() == (2, 7)
    s.run(NITER)
    _same(s.get_state(), _reference(O, s, 128, P, None, "PR"))


@pytest.mark.parametrize("N,R", [(128, 64), (408, 204)], ids=["r64", "r204"])
@pytest.mark.parametrize("lag", [3, 4, 5, 6])
def test_every_lag(ngp, O, lag, N, R):
    """lag 3: wave 2 fetches one block ahead, blocking; lags 4 to 6: the look in flight"""
    s = _device(ngp, O, N, 2560, lag, 2, None, "PR")
    assert s.layout() == (R, 2, 40) and s.config() == (1, lag)
    s.run(NITER)
    _same(s.get_state(), _reference(O, s, N, 2560, None, "PR"))


def test_phase_streamer_default_lag_near_3(ngp, O):
    """shards of 44 rows on the phase streamer (it polls the one-word flag that wave 1 raises, not the granules), the library's lag"""
    s = _device(ngp, O, 88, 2560, None, 2, None, "PR", streamer=None, near=3)
    assert s.layout() == (44, 2, 40) and s.streamer()[0] == 1 and s.near() == 3
    s.run(NITER)
    _same(s.get_state(), _reference(O, s, 88, 2560, None, "PR"))


def test_look_always_complete(ngp, O):
    """BayesB at N = 8: the sampler is the slow end, every look finds its sum complete"""
    s = _device(ngp, O, 8, 2560, 6, 2, None, "B")
    s.run(NITER)
    _same(s.get_state(), _reference(O, s, 8, 2560, None, "B"))


def test_look_too_early(ngp, O):
    """The loader paced (ngp_debug_set_knob: s_sleep 4 after every four tile requests) over tall shards: the streamers are the slow
    end, the sums are late -- a look two blocks ahead finds its sum incomplete and is repeated, a look one block ahead is waited for.
    Once on the production kernel, once on the diagnostic one (the same role; time stamps on), whose debug block counts the
    repeated looks of a launch."""
    s = _device(ngp, O, 408, 2560, 6, 2, None, "PR", knob=4)
    s.run(NITER)
    ref = _reference(O, s, 408, 2560, None, "PR")
    _same(s.get_state(), ref)
    d = _device(ngp, O, 408, 2560, 6, 2, None, "PR", knob=4)
    d.debug_stamps(True)
    d.run(NITER)
    words = d.debug_stamps(True, n=RELOOK_WORD + 1)
    d.debug_stamps(False)
    print("repeated looks in the last launch that had one:", int(words[RELOOK_WORD]))
    assert 1 <= int(words[RELOOK_WORD]) <= 40
    _same(d.get_state(), ref)


def test_failed_census_resumes_the_same_chain(ngp, O):
    """A launch whose census fails ends before any role has run; the call runs that iteration again: the second of three"""
    s = _device(ngp, O, 408, 2560, 6, 2, None, "PR")
    s.debug_fail_census(2)
    s.run(NITER)
    assert s.census()["retries"] == 1
    undisturbed = _device(ngp, O, 408, 2560, 6, 2, None, "PR")
    undisturbed.run(NITER)
    a = s.get_state()
    _same(a, undisturbed.get_state())
    _same(a, _reference(O, s, 408, 2560, None, "PR"))


def test_bayesr_set(ngp, O):
    """k_sweep_r shares the role: one BayesR set of four classes"""
    s = _device(ngp, O, 128, 2560, 6, 2, None, "R")
    assert s.layout() == (64, 2, 40)
    s.run(NITER)
    _same(s.get_state(), _reference(O, s, 128, 2560, None, "R"))


def test_tuple_set(ngp, O):
    """k_sweep_tup shares the role: one Tuple set of k = 2 correlated sets, 1,280 loci each (2,560 columns)"""
    N, nloc, k = 128, 1280, 2
    Xp, y, vm, v, span, off = tuple_problem(O, ngp, N, nloc, k)
    s = ngp.Sampler(device=0, seed=21, chain=0, mode=1, lag=6, streamer=2)
    s.set_max_shards(2)
    s.set_panel(Xp)
    R, S, nb = s.layout()
    assert (R, S) == (64, 2) and nb >= 40 and s.config() == (1, 6)
    o = O.Oracle(order=1, seed=21, chain=0)
    o.set_panel_f32(Xp, R=R, S=S, D=6, near=s.near(), nchain=s.streamer()[1], tform=s.chain_form())
    for m in (s, o):
        add_tuple(m, nloc, k, vm, [(0, nloc // 3), (nloc // 3, nloc)])
        m.set_y(y); m.set_residual_prior(4.0, 0.5); m.set_schedule(NITER, 1, 1); m.run(NITER)
    _same(s.get_state(), o.get_state())


def test_two_chains_per_pass(ngp, O):
    """k_sweep_multi: two chains over one panel in one launch, each the chain it is alone.  Six shards: a fused grid has to reach past
    the second sampler's place (block 8)."""
    N, P, shards = 408, 2560, 6
    fused = []
    for c in range(2):
        X, G, y, v = _problem(O, N, P)
        s = ngp.Sampler(device=0, seed=1001 + c, chain=c, mode=1, lag=6, streamer=2)
        if c == 0:
            s.set_max_shards(shards)
            s.set_panel(X)
        else:
            s.share_panel(fused[0])
        _model(s, P, "PR", y + 0.01 * c, v)
        fused.append(s)
    R, S, nb = fused[0].layout()
    assert R >= 64 and nb == 40 and fused[0].streamer() == (2, 7) and fused[0].config() == (1, 6)
    ngp.Sampler.run_many(fused, NITER)
    assert fused[0].census()["grid"] == 2 * (1 + 1) + S   # ONE launch: two samplers, two reducers, S streamers
    for c in range(2):
        alone = _device(ngp, O, N, P, 6, shards, None, "PR", seed=1001 + c, chain=c, y_shift=0.01 * c)
        assert alone.layout() == (R, S, nb)
        alone.run(NITER)
        f = fused[c].get_state()
        _same(f, alone.get_state())
        _same(f, _reference(O, alone, N, P, None, "PR", seed=1001 + c, chain=c, y_shift=0.01 * c))


def test_byte_tiles(ngp, O):
    s = _device(ngp, O, 416, 2560, 6, 2, "u8", "PR")
    assert s.layout() == (208, 2, 40) and s.config() == (1, 6) and s.streamer() == (3, 7)
    s.run(NITER)
    _same(s.get_state(), _reference(O, s, 416, 2560, "u8", "PR"))
