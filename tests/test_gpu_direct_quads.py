"""Direct quads (k_sweep_dq; role_streamer_rows, ngp_sweep.h): over fp32 tiles every row wave of the row-owning streamer loads the
last quad of its GEMV chain itself -- a plain 16-byte-per-lane load into registers a block ahead, stored into the quad's ring slot
and fed to the same fma at the same place of the chain -- and the loader wave requests seven quads fewer per tile through its
LDS-DMA queue.  The
same values enter the same operations in the same order, so with the feature on, off (the withholding knob) or not offered at all
(byte tiles, the phase streamer, short shards without the knob) the chain is the blocked oracle's for the same layout, bit for
bit.  Whether a launch used them is read from its census: the entry of a streamer workgroup carries the number of quads its wave 0
loaded itself.  The library offers the feature from 160-row shards on; a knob bit offers it at any height that leaves the loader's
early part whole (64 rows: 16 quads, 8 early, the last 7 apart), which is how the short cases reach it."""
import pytest

from test_gpu_poller_look import NITER, P, _device, _reference, _same
from test_gpu_sampler_waits import _device as _device_w, _reference as _reference_w, _same as _same_w

pytestmark = pytest.mark.gpu

NB = P // 64
N_ROWS = 15744   # 246 shards of 64 rows: 16 quads per tile, waves 0 and 1 own three, the others two
N_68 = 16728     # 246 shards of 68 rows: 17 quads, waves 0..2 own three
N_116 = 28536    # 246 shards of 116 rows: 29 quads, wave 0 owns five, the others four
N_TALL = 36000   # 225 shards of 160 rows: the height from which the library offers the feature by itself
P_TALL = 640
N_PHASE = 10824  # 246 shards of 44 rows: phase streamer
N_U8 = 3936      # 246 shards of 16 rows of byte tiles
KNOB_WITHHELD = 1 << 15    # the direct quads are withheld
KNOB_ANY_HEIGHT = 1 << 28  # they are offered below 160-row shards too


def _direct_as_reported(s, active, nb=NB):
    """the census of the last launch: every streamer workgroup fed the same number of own quads per block (1 or 2: NGP_ROWS_DIRECT) to
    wave 0's chain, or none; the sampler and the reducers never do"""
    c = s.census()
    S = s.layout()[1]
    d = c["direct"]
    first = c["grid"] - S
    assert not d[:first].any()
    if active:
        assert d[first] in (nb, 2 * nb) and (d[first:] == d[first]).all(), d
    else:
        assert not d[first:].any(), d
    assert ((c["xcc"] >= 0) & (c["xcc"] < 8)).all()


@pytest.mark.parametrize("kind", ["PR", "B"])
def test_short_shards(ngp, O, kind):
    """64-row shards, lag 6: the smallest tile whose loader keeps its early part (16 quads - 7 direct >= 8 early)"""
    s = _device(ngp, O, N_ROWS, 6, 246, None, kind, knob=KNOB_ANY_HEIGHT)
    assert s.layout() == (64, 246, NB) and s.config() == (1, 6)
    s.run(NITER)
    _direct_as_reported(s, True)
    _same(s.get_state(), _reference(O, s, N_ROWS, None, kind))


@pytest.mark.parametrize("lag", [3, 4, 5])
def test_lags(ngp, O, lag):
    """the delay line is unrolled by the lag: the direct quad's request and use sit in every one of its 3, 4, 5 copies"""
    s = _device(ngp, O, N_ROWS, lag, 246, None, "PR", knob=KNOB_ANY_HEIGHT)
    assert s.layout() == (64, 246, NB) and s.config() == (1, lag)
    s.run(NITER)
    _direct_as_reported(s, True)
    _same(s.get_state(), _reference(O, s, N_ROWS, None, "PR"))


@pytest.mark.parametrize("N,R", [(N_68, 68), (N_116, 116)], ids=["r68", "r116"])
def test_uneven_shard_heights(ngp, O, N, R):
    """quads per tile no multiple of 7: the waves' chains differ in length, and the direct quads start at another wave"""
    s = _device(ngp, O, N, 6, 246, None, "PR", knob=KNOB_ANY_HEIGHT)
    assert s.layout() == (R, 246, NB) and s.config() == (1, 6)
    s.run(NITER)
    _direct_as_reported(s, True)
    _same(s.get_state(), _reference(O, s, N, None, "PR"))


def test_tall_shards_as_the_library_runs_them(ngp, O):
    """225 shards of 160 rows, no knob (ten blocks, to keep a panel of this height quick)"""
    s = _device_w(ngp, O, N_TALL, P_TALL, 6, 225, None, "PR")
    assert s.layout() == (160, 225, P_TALL // 64) and s.config() == (1, 6) and s.streamer() == (2, 7)
    s.run(NITER)
    _direct_as_reported(s, True, nb=P_TALL // 64)
    _same_w(s.get_state(), _reference_w(O, s, N_TALL, P_TALL, None, "PR"))


@pytest.mark.parametrize("p", [64, 128], ids=["1_block", "2_blocks"])
def test_edge_block_counts(ngp, O, p):
    """one block: only the request ahead of the first barrier; two: that one and the single request of the loop"""
    s = _device_w(ngp, O, N_ROWS, p, 6, 246, None, "PR", knob=KNOB_ANY_HEIGHT)
    assert s.layout() == (64, 246, p // 64) and s.config() == (1, 6)
    s.run(NITER)
    _direct_as_reported(s, True, nb=p // 64)
    _same_w(s.get_state(), _reference_w(O, s, N_ROWS, p, None, "PR"))


def test_short_shards_without_the_knob(ngp, O):
    """64-row shards as the library runs them: the loader brings every quad"""
    s = _device(ngp, O, N_ROWS, 6, 246, None, "PR")
    s.run(NITER)
    _direct_as_reported(s, False)
    _same(s.get_state(), _reference(O, s, N_ROWS, None, "PR"))


def test_byte_tiles(ngp, O):
    """byte tiles keep their loader: not offered, even with the any-height knob"""
    s = _device(ngp, O, N_U8, None, 246, "u8", "PR", knob=KNOB_ANY_HEIGHT)
    assert s.layout() == (16, 246, NB)
    s.run(NITER)
    _direct_as_reported(s, False)
    _same(s.get_state(), _reference(O, s, N_U8, "u8", "PR"))


def test_phase_streamer(ngp, O):
    """nor beside the phase streamer, which has no row-owning waves"""
    s = _device_w(ngp, O, N_PHASE, P, 6, 246, None, "PR", knob=KNOB_ANY_HEIGHT, streamer=None, near=3)
    assert s.layout() == (44, 246, NB) and s.config() == (1, 6) and s.streamer()[0] == 1
    s.run(NITER)
    _direct_as_reported(s, False)
    _same_w(s.get_state(), _reference_w(O, s, N_PHASE, P, None, "PR"))


def test_withheld(ngp, O):
    """the withholding knob wins over the any-height knob: the loader requests all 16 quads, and the chain is the one of the
    handle whose row waves load seven of them themselves"""
    off = _device(ngp, O, N_ROWS, 6, 246, None, "PR", knob=KNOB_ANY_HEIGHT | KNOB_WITHHELD)
    off.run(NITER)
    _direct_as_reported(off, False)
    on = _device(ngp, O, N_ROWS, 6, 246, None, "PR", knob=KNOB_ANY_HEIGHT)
    on.run(NITER)
    _direct_as_reported(on, True)
    a, b = off.get_state(), on.get_state()
    _same(a, b)
    _same(a, _reference(O, off, N_ROWS, None, "PR"))


def test_census_retry(ngp, O):
    """a launch that ends at its census is run again: the report starts from zero in every launch, the requests ahead of the first
    barrier are made again"""
    s = _device(ngp, O, N_ROWS, 6, 246, None, "PR", knob=KNOB_ANY_HEIGHT)
    s.debug_fail_census(2)
    s.run(NITER)
    assert s.census()["retries"] == 1
    _direct_as_reported(s, True)
    undisturbed = _device(ngp, O, N_ROWS, 6, 246, None, "PR", knob=KNOB_ANY_HEIGHT | KNOB_WITHHELD)
    undisturbed.run(NITER)
    a, b = s.get_state(), undisturbed.get_state()
    _same(a, b)
    _same(a, _reference(O, s, N_ROWS, None, "PR"))
