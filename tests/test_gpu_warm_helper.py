"""The warmer (role_warmer, ngp_sweep.h): where the last reducer workgroup of a sweep has no far lag to correct and the dispatcher has
put it on the sampler's XCD, it pulls the next blocks' Gram planes into that XCD's L2, and the streamers' loader waves on that XCD
request their tiles alone (row-owning streamer over fp32 tiles; the phase streamer and byte tiles keep the streamers' warming).
Who warms is decided on the device from two write-once words (the sampler's XCC id, the warmer's), so the tests read the placement
from the census and do not assume it.  Warming never changes a value: whoever warms -- the warmer, the
streamers, nobody (the knob) -- the chain is the blocked oracle's for the same layout, bit for bit.  P = 2,560 everywhere: 40 blocks,
two wraps of the 16-slot rings, five blocks for each of the warmer's eight waves.  The 64-row shards of these cases are below the
height from which the library offers the role (160 rows); a timing knob offers it at any height, which is how they reach it."""
import pytest

from test_gpu_poller_look import NITER, P, _device, _reference, _same
from test_gpu_sampler_waits import _device as _device_w, _reference as _reference_w, _same as _same_w

pytestmark = pytest.mark.gpu

NB = P // 64
N_ROWS = 15744   # 246 shards of 64 rows: row-owning streamer, eight reducer workgroups
N_TALL = 36000   # 225 shards of 160 rows: still eight reducer workgroups
P_TALL = 640
N_PHASE = 10824  # 246 shards of 44 rows: phase streamer
N_U8 = 3936      # 246 shards of 16 rows of byte tiles
KNOB_NO_WARM = 2048     # no streamer warms
KNOB_NO_WARMER = 8192   # the warmer role is withheld
KNOB_ANY_HEIGHT = 16384 # the role is offered below 160-row shards too (the library offers it from 160 rows on, where it was measured to pay)


def _warmer_as_placed(s, candidate=True, nb=NB):
    """the warmer's report against the census of the same launch: active iff workgroup NG shares workgroup 0's XCD"""
    c, w = s.census(), s.warmer()
    S = s.layout()[1]
    NG = c["grid"] - 1 - S
    if not candidate:
        assert w == dict(active=0, blocks=0)
        return
    assert S >= 225 and NG == 8
    print("sampler's XCC", c["xcc"][0], "workgroup NG's", c["xcc"][NG], "warmer", w)
    if c["xcc"][NG] == c["xcc"][0]:
        assert w["active"] == 1 and w["blocks"] == nb
    else:
        assert w == dict(active=0, blocks=0)


@pytest.mark.parametrize("kind", ["PR", "B"])
def test_row_owning_streamer(ngp, O, kind):
    """lag 6, two near lags: reducers 3..7 idle.  BayesB makes the sampler the slow end: the warmer waits for dlt in every block."""
    s = _device(ngp, O, N_ROWS, 6, 246, None, kind, knob=KNOB_ANY_HEIGHT)
    assert s.layout() == (64, 246, NB) and s.config() == (1, 6)
    s.run(NITER)
    _warmer_as_placed(s)
    _same(s.get_state(), _reference(O, s, N_ROWS, None, kind))


def test_phase_streamer(ngp, O):
    """The role is not offered beside the phase streamer (measured at 10k x 100k: one CU does not pull that shape's planes in a block
    period, the sweep lost 22 %): its loaders read one word as they always did, and warm."""
    s = _device_w(ngp, O, N_PHASE, P, 6, 246, None, "PR", streamer=None, near=3)
    assert s.layout() == (44, 246, NB) and s.config() == (1, 6) and s.streamer()[0] == 1 and s.near() == 3
    s.run(NITER)
    _warmer_as_placed(s, candidate=False)
    _same_w(s.get_state(), _reference_w(O, s, N_PHASE, P, None, "PR"))


def test_byte_tiles(ngp, O):
    """Nor beside byte tiles (50k x 600k compact: 1.3 % slower with it; that sweep is bound by the sampler, not by the loaders)."""
    s = _device(ngp, O, N_U8, None, 246, "u8", "PR")
    assert s.layout() == (16, 246, NB)
    s.run(NITER)
    _warmer_as_placed(s, candidate=False)
    _same(s.get_state(), _reference(O, s, N_U8, "u8", "PR"))


@pytest.mark.parametrize("lag", [3, 4, 5])
def test_lags(ngp, O, lag):
    """workgroup 8 is idle at each of these lags too; blocks t <= lag are warmed at once, against rings of every depth"""
    s = _device(ngp, O, N_ROWS, lag, 246, None, "PR", knob=KNOB_ANY_HEIGHT)
    assert s.layout() == (64, 246, NB) and s.config() == (1, lag)
    s.run(NITER)
    _warmer_as_placed(s)
    _same(s.get_state(), _reference(O, s, N_ROWS, None, "PR"))


def test_tall_shards_as_the_library_runs_them(ngp, O):
    """225 shards of 160 rows, no knob: the height from which the library offers the role by itself.  (Ten blocks, to keep a panel of
    this height quick: blocks 0..6 are warmed at once, 7..9 wait for dlt.)"""
    s = _device_w(ngp, O, N_TALL, P_TALL, 6, 225, None, "PR")
    assert s.layout() == (160, 225, P_TALL // 64) and s.config() == (1, 6) and s.streamer() == (2, 7)
    s.run(NITER)
    _warmer_as_placed(s, nb=P_TALL // 64)
    _same_w(s.get_state(), _reference_w(O, s, N_TALL, P_TALL, None, "PR"))


def test_short_shards_without_the_knob(ngp, O):
    """64-row shards as the library runs them: the role is not offered, the streamers warm"""
    s = _device(ngp, O, N_ROWS, 6, 246, None, "PR")
    s.run(NITER)
    _warmer_as_placed(s, candidate=False)
    _same(s.get_state(), _reference(O, s, N_ROWS, None, "PR"))


def test_no_candidate(ngp, O):
    """two shards, one reducer workgroup: nobody takes the warmer role, the streamers warm as they always did"""
    s = _device(ngp, O, 408, 6, 2, None, "PR")
    assert s.layout() == (204, 2, NB)
    s.run(NITER)
    _warmer_as_placed(s, candidate=False)
    _same(s.get_state(), _reference(O, s, 408, None, "PR"))


def test_census_retry(ngp, O):
    """a launch that ends at its census is run again: the warmer's words start from zero in every launch"""
    s = _device(ngp, O, N_ROWS, 6, 246, None, "PR", knob=KNOB_ANY_HEIGHT)
    s.debug_fail_census(2)
    s.run(NITER)
    assert s.census()["retries"] == 1
    _warmer_as_placed(s)
    undisturbed = _device(ngp, O, N_ROWS, 6, 246, None, "PR")
    undisturbed.run(NITER)
    a, b = s.get_state(), undisturbed.get_state()
    _same(a, b)
    _same(a, _reference(O, s, N_ROWS, None, "PR"))


@pytest.mark.parametrize("knob", [KNOB_NO_WARM, KNOB_NO_WARMER, KNOB_NO_WARM | KNOB_NO_WARMER], ids=["streamers_off", "warmer_off", "nobody_warms"])
def test_warming_knobs(ngp, O, knob):
    """the knob bits that keep the streamers from warming and withhold the warmer role change timing only: the call succeeds and the
    chain is the same"""
    s = _device(ngp, O, N_ROWS, 6, 246, None, "PR", knob=knob | KNOB_ANY_HEIGHT)
    s.run(NITER)
    _warmer_as_placed(s, candidate=not (knob & KNOB_NO_WARMER))
    _same(s.get_state(), _reference(O, s, N_ROWS, None, "PR"))
