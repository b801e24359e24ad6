"""The row-owning streamer's poller wave (wave 6 of role_streamer_rows, ngp_sweep.h) asks for the granules of the next dlt before the
block's barrier.  Over fp32 tiles it examines them at the end of its block only (no look, no second request behind the barrier);
over byte tiles it looks behind the barrier and asks again if the tags are stale; the bounded wait at the end of the block is the
same for both.  Whichever of these paths a block takes -- dlt there at the first look, asked for too early, a launch that ends at
its census and is run again -- the chain is the blocked oracle's for the same layout, bit for bit.  P = 2,560 everywhere: 40
blocks, two wraps of the 16-slot rings."""
import numpy as np
import pytest

from conftest import add_sets, make_problem

pytestmark = pytest.mark.gpu

P = 2560
NITER = 3
KEYS = ("ycorr", "beta", "delta", "varBeta", "piHat")
_problems = {}
_references = {}


def _problem(O, N):
    """(fp32 panel, genotype codes, y, v) of an N x P problem, made once"""
    if N not in _problems:
        X, y, bt, v = make_problem(O, N, P, seed=5)
        _, mu = O.generate_panel(N, P)
        G = np.rint(X.astype(np.float64) + mu[None, :]).astype(np.uint8)
        assert G.max() <= 2
        _problems[N] = (X, G, y, v)
    return _problems[N]


def _model(m, kind, y, v):
    add_sets(m, [(0, P, kind)], v)
    m.set_y(y)
    m.set_residual_prior(4.0, 0.25 * y.var())
    m.set_schedule(NITER, 1, 1)


def _device(ngp, O, N, lag, shards, storage, kind, knob=0):
    X, G, y, v = _problem(O, N)
    s = ngp.Sampler(device=0, seed=1001, chain=0, mode=1 if lag else None, lag=lag, streamer=None if storage else 2, storage=storage)  # lag None: the library's own
    s.set_max_shards(shards)
    if knob:
        s.debug_set_knob(knob)
    if storage:
        s.set_panel(G, centre=True)
    else:
        s.set_panel(X)
    assert s.streamer() == ((3, 7) if storage else (2, 7))
    _model(s, kind, y, v)
    return s


def _reference(O, s, N, storage, kind):
    """state of the blocked oracle after NITER iterations in the layout of handle s; one oracle run per (problem, layout)"""
    R, S, _ = s.layout()
    key = (N, storage, kind, R, S, s.config()[1], s.near(), s.chain_form())
    if key not in _references:
        X, G, y, v = _problem(O, N)
        o = O.Oracle(order=1, seed=1001, chain=0)
        if storage:
            o.set_panel_u8(G, R=R, S=S, D=key[5], near=key[6], tform=key[7])
        else:
            o.set_panel_f32(X, R=R, S=S, D=key[5], near=key[6], nchain=7, tform=key[7])
        _model(o, kind, y, v)
        o.run(NITER)
        st = o.get_state()
        for k in KEYS:
            st[k].setflags(write=False)
        _references[key] = st
    return _references[key]


def _same(a, b):
    for k in KEYS:
        assert np.array_equal(a[k], b[k]), k
    assert a["varE"] == b["varE"] and a["b"] == b["b"] and a["iter"] == b["iter"] == NITER


@pytest.mark.parametrize("N,shards,R", [(128, 2, 64), (1024, 8, 128), (408, 2, 204)], ids=["r64", "r128", "r204"])
@pytest.mark.parametrize("lag", [3, 4, 5, 6])
def test_fp32_tiles_every_lag_and_shard_height(ngp, O, lag, N, shards, R):
    s = _device(ngp, O, N, lag, shards, None, "PR")
    assert s.layout() == (R, shards, P // 64) and s.config() == (1, lag)
    s.run(NITER)
    _same(s.get_state(), _reference(O, s, N, None, "PR"))


@pytest.mark.parametrize("N,shards,R", [(128, 2, 64), (416, 2, 208)], ids=["short", "tall"])
@pytest.mark.parametrize("lag", [6, None], ids=["lag6", "default_lag"])
def test_byte_tiles(ngp, O, lag, N, shards, R):
    s = _device(ngp, O, N, lag, shards, "u8", "PR")
    assert s.layout() == (R, shards, P // 64) and s.config() == (1, 6 if lag else 8)
    s.run(NITER)
    _same(s.get_state(), _reference(O, s, N, "u8", "PR"))


@pytest.mark.parametrize("storage", [None, "u8"], ids=["f32", "u8"])
def test_asked_for_too_early_in_every_block(ngp, O, storage):
    """BayesB at tiny N: a block of the sampler takes several times a block of the streamers, so the granules asked for before the
    barrier are stale whenever they are examined -- the second request (byte tiles) and the bounded wait at the end of the block
    carry the chain."""
    N = 16 if storage else 8
    s = _device(ngp, O, N, 6, 2, storage, "B")
    s.run(NITER)
    _same(s.get_state(), _reference(O, s, N, storage, "B"))


@pytest.mark.parametrize("N,storage,kind", [(8, None, "B"), (408, None, "PR"), (416, "u8", "PR")], ids=["tiny_b", "r204_pr", "u8_r208_pr"])
def test_dlt_there_when_first_examined(ngp, O, N, storage, kind):
    """The loader paced (ngp_debug_set_knob: s_sleep 4 after every four tile requests): the streamers are the slow end, dlt of the
    next block is published long before the poller asks -- over byte tiles the look behind the barrier finds it, over fp32 tiles the
    examination at the end of the block.  (The pacing bites on the tall shards, 51 quads / 13 units per tile; the tiny shape is the
    one of the case above.)  The knob changes timing only: the call succeeds and the chain is valid."""
    s = _device(ngp, O, N, 6, 2, storage, kind, knob=4)
    s.run(NITER)
    _same(s.get_state(), _reference(O, s, N, storage, kind))


def test_failed_census_resumes_the_same_chain(ngp, O):
    """A launch whose census fails ends before any role has run; the call runs that iteration again: lag 6, fp32 tiles, the second
    of three iterations."""
    s = _device(ngp, O, 408, 6, 2, None, "PR")
    s.debug_fail_census(2)
    s.run(NITER)
    assert s.census()["retries"] == 1
    undisturbed = _device(ngp, O, 408, 6, 2, None, "PR")
    undisturbed.run(NITER)
    a, b = s.get_state(), undisturbed.get_state()
    _same(a, b)
    _same(a, _reference(O, s, 408, None, "PR"))
