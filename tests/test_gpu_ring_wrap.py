"""Every kernel of the persistent sweep past two wraps of its 16-slot rings (NGP_RING, ngp_sweep_args.h: dlt, its granules dltg, the
fixed-point accumulators acc, the sampler's LDS copies hist and vacc), bit for bit.  A slot is reused from block 16 on -- column 1,024 --
and only there do three things happen for the first time: an accumulator must be zero again when the block 16 further on adds its terms
(the ztake hand-over from wave 2 to wave 1), a granule's tag must tell block u from block u - 16, and a partial last block writes fewer
than 64 lanes into a slot that still holds a full block's values.  An error in any of them gives a chain that is wrong only past column
1,024, which a test of at most 16 blocks cannot see.

Shape of every case: P = 2,600 columns = 40 full blocks and a tail of 40 lanes (block 40: slot 8, after blocks 8 and 24), three
iterations with schedule (3, 1, 1), the smallest N that gives the layout.  Two models: one BayesPR set, and the mixed model
[PR 1100 | B 230 | R 500 | C 300 | R16 470], whose seams lie inside blocks 17, 20, 28 and 33 (none at a multiple of 64) and whose last set
reads classes 9..16 from memory per block.  The reference is the blocked oracle told the handle's own layout; where there is none (three
annotations of a BayesRCpi set) the chain is held to its one-shard sibling and to the chain alone.  Every case asserts the layout, lag,
streamer and, for fused and tall launches, the grid, so that it cannot run on another engine unnoticed; and every reference is
checked, on the ORACLE's state, not to be vacuous: 41 blocks, every set with effects past column 1,024, BayesB / BayesC loci both in and
out, an R16 locus in a class >= 9.

Path past 16 blocks, bit for bit                                   | here                                        | elsewhere
-------------------------------------------------------------------|---------------------------------------------|---------------------------
phase streamer, lags 1, 2, 3, 4, 8; near 1, 2, 4 at lag 8          | test_phase_streamer                         | default lag, near 3: test_gpu_sampler_waits
row-owning streamer, lags 3 and 6, R 64 and R 204, mixed model     | test_row_owning_streamer                    | PR, lags 3-6: test_gpu_sampler_waits
byte tiles, lags 3, 8, 12; near 1 / 4 at lag 12                    | test_byte_tiles                             | lags 6, 8: test_gpu_sampler_waits, test_gpu_direct_quads
byte tiles, two and four update tasks                              | test_byte_tiles_tall_shards                 | --
k_sweep_tall, V = 2 and 3: padded, 112-188 rows, 15 / 22 groups    | test_tall_shards                            | --
inverse chain form (k_tinv) on BayesPR sets                        | test_inverse_chain_form                     | --
per-block launches (no ring: the control)                          | test_block_launches_control                 | --
BayesR above 8 classes; set seams inside blocks >= 16              | the mixed model of every test above         | four classes: test_gpu_sampler_waits
k_sweep_tup, k = 4                                                 | test_tuple_of_four                          | k = 2: test_gpu_sampler_waits
k_sweep_rc, k_sweep_tall_rc: one annotation against BayesR         | test_rc_one_annotation_is_the_oracles_bayesr| --
k_sweep_tall_rc, three annotations                                 | test_rc_tall_equals_one_shard_sibling       | --
k_sweep_multi: three chains (phase), two (row-owning, lag 4)       | test_fused_pr_chains                        | two PR chains, lag 6: test_gpu_sampler_waits
k_sweep_multi over byte tiles with two update tasks, K = 2 and 3   | test_fused_pr_chains_over_byte_tiles        | --
k_sweep_multi_r, k_sweep_multi_tup, k_sweep_multi_rc               | test_fused_mixed / _tuple / _rc_and_plain   | --
a partial last block in a reused slot                              | every case (P % 64 = 40)                    | --

(The fused kernel serves three fp32 chains on the phase streamer at lags 6 and 8 only, and lag 4 on the row-owning streamer with two
chains only -- fusable(), ngp_api.hip -- so the fp32 fused cases are K = 3 at lags 6 and 8 and K = 2 at lag 4.)"""
import numpy as np
import pytest

from conftest import add_sets, make_problem
from test_gpu_bayesrc import PI4, VC4, make_annot
from test_gpu_sampler_waits import NITER, _problem, _same
from test_tuple_main_oracle import add_tuple

pytestmark = pytest.mark.gpu

P = 2600
NBLK = (P + 63) // 64
PR = ((0, P, "PR"),)
MIXED = ((0, 1100, "PR"), (1100, 230, "B"), (1330, 500, "R"), (1830, 300, "C"), (2130, 470, "R16"))
R_ALONE = ((0, P, "R"),)
RC1 = ((0, P, "RC1"),)                      # one all-ones annotation: BayesR bit for bit
RC3_MIXED = ((0, 1100, "PR"), (1100, 730, "RC3"), (1830, 300, "C"), (2130, 470, "R16"))   # three annotations, seams inside blocks 17 and 28
TUP4 = ((0, 650, ("TUP", 4)),)              # 650 loci x 4 sets: 16 loci per block, 40 blocks and 10 loci = 40 lanes
TUP2 = ((0, 1300, ("TUP", 2)),)             # 1300 loci x 2 sets: 32 loci per block, 40 blocks and 20 loci = 40 lanes
MODELS = {"pr": PR, "mixed": MIXED}
BOTH = pytest.mark.parametrize("model", ["pr", "mixed"])

_tuple_panels = {}
_references = {}


def _tuple_of(model):
    kind = model[0][2]
    return kind[1] if isinstance(kind, tuple) and kind[0] == "TUP" else 0


def _panel(O, ngp, N, model):
    """(fp32 panel, genotype codes or None, y, v) for the model on N rows, made once: the problem test_gpu_sampler_waits caches, or the
    same columns interleaved for a Tuple set"""
    k = _tuple_of(model)
    if not k:
        return _problem(O, N, P)
    if (N, k) not in _tuple_panels:
        X, y, _, v = make_problem(O, N, P, seed=5, ncausal=12)
        nloc = model[0][1]
        Xt = ngp.tuple_panel([np.asfortranarray(X[:, m * nloc:(m + 1) * nloc]) for m in range(k)])
        assert Xt.shape == (N, P)
        _tuple_panels[(N, k)] = (Xt, None, y, v)
    return _tuple_panels[(N, k)]


def _setup(m, model, y, v):
    """the same calls on a handle and on the oracle (which knows no BayesRCpi set: its callers hand it the BayesR model)"""
    for c0, n, kind in model:
        if kind == "RC1":
            m.add_marker_set_rc(c0, n, 4.0, v * 0.5, v, VC4, PI4, np.ones((n, 1), dtype=np.int32), estPi=True)
        elif kind == "RC3":
            m.add_marker_set_rc(c0, n, 4.0, v * 0.5, v, VC4, PI4, make_annot(n, 3, seed=60), estPi=True)
        elif isinstance(kind, tuple) and kind[0] == "TUP":
            k = kind[1]
            add_tuple(m, n, k, v * (0.6 * np.eye(k) + 0.4 * np.ones((k, k))), [(0, n // 3), (n // 3, n)])
        else:
            add_sets(m, [(c0, n, kind)], v)
    m.set_y(y)
    m.set_residual_prior(4.0, 0.25 * y.var())
    m.set_schedule(NITER, 1, 1)


def _handle(ngp, O, N, model, lag, streamer=None, storage=None, shards=2, near=0, mode=1, form=None, seed=1001, chain=0, y_shift=0.0, owner=None):
    X, G, y, v = _panel(O, ngp, N, model)
    s = ngp.Sampler(device=0, seed=seed, chain=chain, mode=mode, lag=lag, streamer=None if storage else streamer, storage=storage)
    if form is not None:
        s.set_chain_form(form)
    if owner is not None:
        s.share_panel(owner)
    else:
        if shards:
            s.set_max_shards(shards)
        if near:
            s.set_near(near)
        if storage:
            s.set_panel(G, centre=True)
        else:
            s.set_panel(X)
    _setup(s, model, y + y_shift, v)
    return s


def _full(m, model):
    """state, posterior sums and, per set with classes, the class state"""
    st = dict(m.get_state())
    st.update(("post_" + k, x) for k, x in m.get_posterior_sums().items())
    for si, (_, _, kind) in enumerate(model):
        if kind == "RC3":
            st.update((f"rc{si}_{k}", x) for k, x in m.rc_state(si).items())
        elif isinstance(kind, str) and kind.startswith("R"):
            st.update((f"cls{si}_{k}", x) for k, x in m.get_class_state(si).items())
    return st


def _not_vacuous(st, model):
    """on the oracle's state: the rings wrap twice and end on a partial block, and every set does something past the first wrap"""
    assert NBLK >= 41 and P % 64 == 40
    for c0, n, kind in model:
        lo, hi = (1024, P) if _tuple_of(model) else (max(c0, 1024), c0 + n)
        assert hi > lo and np.any(st["beta"][lo:hi] != 0.0), (kind, "no effect past column 1,024")
        if kind in ("B", "C"):
            d = st["delta"][c0:c0 + n]
            assert (d == 1).any() and (d == 0).any(), (kind, "needs loci in and out")
        if kind == "R16":
            assert (st["delta"][lo:hi] >= 9).any(), "R16: no locus in a class read from memory"


def _reference(O, ngp, s, N, model, storage=None, seed=1001, chain=0, y_shift=0.0):
    """full state of the blocked oracle after NITER iterations in the layout of handle s: one run per (problem, layout, model, chain),
    checked not to be vacuous, left unchanged"""
    R, S, nb = s.layout()
    assert nb == NBLK
    D, near, nchain, tform = s.config()[1], s.near(), s.streamer()[1], s.chain_form()
    key = (N, storage, model, R, S, D, near, nchain, tform, seed, chain, y_shift)
    if key not in _references:
        X, G, y, v = _panel(O, ngp, N, model)
        o = O.Oracle(order=1, seed=seed, chain=chain)
        if storage:
            o.set_panel_u8(G, R=R, S=S, D=D, near=near, tform=tform)
        else:
            o.set_panel_f32(X, R=R, S=S, D=D, near=near, nchain=nchain, tform=tform)
        _setup(o, model, y + y_shift, v)
        o.run(NITER)
        st = _full(o, model)
        _not_vacuous(st, model)
        for x in st.values():
            if isinstance(x, np.ndarray):
                x.setflags(write=False)
        _references[key] = st
    return _references[key]


def _equal(a, b, what=""):
    """state a of a handle against state b of the oracle or of another handle: everything _full holds, bit for bit"""
    _same(a, b)
    assert a.keys() == b.keys(), what
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert np.array_equal(x, y[:len(x)] if y.ndim == 1 else y), (what, k)
    assert a["post_nKept"] == NITER - 1


def _hold(ngp, O, s, N, model, storage=None, oracle_model=None, **chain):
    """run the handle and hold it to the oracle's chain of oracle_model (a BayesRCpi set with one annotation: the BayesR set) or model"""
    s.run(NITER)
    a = _full(s, model)
    _equal(a, _reference(O, ngp, s, N, oracle_model or model, storage, **chain))
    return a


# ---- single chains against the oracle ----------------------------------------------------------------------------------------------------
PHASE = [(1, 0), (2, 0), (3, 0), (4, 0), (8, 0), (8, 1), (8, 2), (8, 4)]   # (lag, near): test_gpu_parity's ENGINES without a streamer variant


@BOTH
@pytest.mark.parametrize("lag,near", PHASE, ids=[f"lag{l}" + (f"_near{n}" if n else "") for l, n in PHASE])
def test_phase_streamer(ngp, O, lag, near, model):
    """shards of 44 rows; the streamers poll the one-word flag of a block, the far lags come from the reducers' rings"""
    s = _handle(ngp, O, 88, MODELS[model], lag, streamer=1, near=near)
    assert s.layout() == (44, 2, NBLK) and s.config() == (1, lag) and s.streamer() == (1, 8) and s.near() == (near or 3)
    _hold(ngp, O, s, 88, MODELS[model])


@pytest.mark.parametrize("N,R", [(128, 64), (408, 204)], ids=["r64", "r204"])
@pytest.mark.parametrize("model,lag", [("mixed", 3), ("mixed", 6), ("pr", 6)])
def test_row_owning_streamer(ngp, O, model, lag, N, R):
    """lag 3: wave 2 fetches one block ahead, blocking; lag 6: the look in flight.  The mixed model on both, BayesPR's ragged tail at 6."""
    s = _handle(ngp, O, N, MODELS[model], lag, streamer=2)
    assert s.layout() == (R, 2, NBLK) and s.config() == (1, lag) and s.streamer() == (2, 7)
    _hold(ngp, O, s, N, MODELS[model])


BYTES = [(3, 0), (8, 0), (12, 0), (12, 1), (12, 4)]   # lag 12: 12 of the 16 slots in flight, the tightest margin the plan allows


@BOTH
@pytest.mark.parametrize("lag,near", BYTES, ids=[f"lag{l}" + (f"_near{n}" if n else "") for l, n in BYTES])
def test_byte_tiles(ngp, O, lag, near, model):
    s = _handle(ngp, O, 416, MODELS[model], lag, storage="u8", near=near)
    assert s.layout() == (208, 2, NBLK) and s.config() == (1, lag) and s.streamer() == (3, 7) and s.storage() == 1 and s.near() == (near or 2)
    _hold(ngp, O, s, 416, MODELS[model], "u8")


@BOTH
@pytest.mark.parametrize("N,R,tasks,D", [(900, 240, 2, 8), (1800, 464, 4, 4)], ids=["two_tasks", "four_tasks"])
def test_byte_tiles_tall_shards(ngp, O, N, R, tasks, D, model):
    """two and four update tasks per lane (shards of 225..448 and 449..896 rows): the shapes of test_compact_tall_shards"""
    s = _handle(ngp, O, N, MODELS[model], 8, storage="u8", shards=4)
    assert s.layout() == (R, 4, NBLK) and s.config() == (1, D) and s.streamer() == (3, 7)
    assert {1: 1, 2: 2, 3: 4, 4: 4}[(4 * ((R // 16 + 6) // 7) + 7) // 8] == tasks
    _hold(ngp, O, s, N, MODELS[model], "u8")


TALL = [  # (N, max shards, V, (R, S)): the padded, the tall-shard and the many-group layouts of test_gpu_parity's TALL
    ("padded", 50, 6, 2, (12, 6)), ("r188", 1500, 8, 2, (188, 8)), ("ng15", 1900, 0, 2, (4, 476)),
    ("v3_padded", 50, 6, 3, (12, 6)), ("v3_r112", 1000, 9, 3, (112, 9)), ("v3_ng22", 2790, 0, 3, (4, 699)),
]


@BOTH
@pytest.mark.parametrize("name,N,shards,V,lay", TALL, ids=[t[0] for t in TALL])
def test_tall_shards(ngp, O, name, N, shards, V, lay, model):
    """k_sweep_tall (role_streamer_rows_tall): two shards per workgroup at lag 3, three at lag 2; with 15 and 22 reducer groups the
    sampler adds the group sums it fetched one block ahead"""
    s = _handle(ngp, O, N, MODELS[model], 6, streamer=2 * V, shards=shards)
    R, S, _ = s.layout()
    assert (R, S) == lay and s.config() == (1, 5 - V) and s.streamer() == (2, 7)
    if "padded" in name:
        assert R * (S - 1) >= N                 # the last shard holds no row of the panel
    _hold(ngp, O, s, N, MODELS[model])
    assert s.census()["grid"] == 1 + (S + 31) // 32 + S // V


FORM1 = [  # (N, lag, Sampler arguments, layout, lag in force, model)
    ("phase", 88, 8, dict(streamer=1), (44, 2), 8, "pr"), ("rows", 128, 6, dict(streamer=2), (64, 2), 6, "pr"),
    ("tall_v2", 1500, 6, dict(streamer=4, shards=8), (188, 8), 3, "pr"), ("bytes", 416, 8, dict(storage="u8"), (208, 2), 8, "pr"),
    ("phase_mixed", 88, 4, dict(streamer=1), (44, 2), 4, "mixed"),
]


@pytest.mark.parametrize("name,N,lag,kw,lay,D,model", FORM1, ids=[f[0] for f in FORM1])
def test_inverse_chain_form(ngp, O, name, N, lag, kw, lay, D, model):
    """ngp_set_chain_form(1): BayesPR blocks as dlt = T e0 (k_tinv), the oracle told the same"""
    s = _handle(ngp, O, N, MODELS[model], lag, form=1, **kw)
    assert s.chain_form() == 1 and s.layout() == lay + (NBLK,) and s.config() == (1, D)
    _hold(ngp, O, s, N, MODELS[model], kw.get("storage"))


def test_block_launches_control(ngp, O):
    """mode 0 has no ring: model and oracle agree at this P before a ring is involved"""
    s = _handle(ngp, O, 88, MIXED, 1, streamer=1, shards=0, mode=0)
    assert s.config() == (0, 1) and s.streamer() == (0, 8) and s.layout()[2] == NBLK
    _hold(ngp, O, s, 88, MIXED)


def test_tuple_of_four(ngp, O):
    """k_sweep_tup: one Tuple set of four correlated sets, 650 loci (41 blocks of 16 loci, the last of 10), row-owning streamer"""
    s = _handle(ngp, O, 128, TUP4, 6, streamer=2, seed=21)
    assert s.layout() == (64, 2, NBLK) and s.config() == (1, 6) and s.streamer() == (2, 7)
    _hold(ngp, O, s, 128, TUP4, seed=21)


RC_ONE = [("phase", 88, dict(streamer=1), (44, 2), 6, (1, 8)), ("rows", 128, dict(streamer=2), (64, 2), 6, (2, 7)),
          ("bytes", 416, dict(storage="u8"), (208, 2), 6, (3, 7)), ("tall_v2", 1500, dict(streamer=4, shards=8), (188, 8), 3, (2, 7)),
          ("tall_v3", 1000, dict(streamer=6, shards=9), (112, 9), 2, (2, 7))]


@pytest.mark.parametrize("name,N,kw,lay,D,streamer", RC_ONE, ids=[r[0] for r in RC_ONE])
def test_rc_one_annotation_is_the_oracles_bayesr(ngp, O, name, N, kw, lay, D, streamer):
    """k_sweep_rc and k_sweep_tall_rc: with one annotation column of ones a BayesRCpi set is BayesR bit for bit (test_gpu_bayesrc.py ties
    that at 520 columns), so the set on 2,600 columns is held to the oracle's BayesR chain"""
    s = _handle(ngp, O, N, RC1, 6, **kw)
    R, S, _ = s.layout()
    assert (R, S) == lay and s.config() == (1, D) and s.streamer() == streamer
    a = _hold(ngp, O, s, N, RC1, kw.get("storage"), oracle_model=R_ALONE)
    rc = s.rc_state(0)
    assert np.all(rc["annotCat"] == 1) and np.array_equal(rc["piHat"].ravel(), a["cls0_piHat"])
    if "tall" in name:
        assert s.census()["grid"] == 1 + (S + 31) // 32 + S // (5 - D)


def test_rc_tall_equals_one_shard_sibling(ngp, O):
    """k_sweep_tall_rc with three annotations (no oracle): two shards per workgroup at lag 3 and the row-owning streamer at lag 3 share
    layout, shard partials and reducer groups, so the chain is the same on both -- full state, rc_state included"""
    N = 1500
    tall = _handle(ngp, O, N, RC3_MIXED, 6, streamer=4, shards=8)
    sib = _handle(ngp, O, N, RC3_MIXED, 3, streamer=2, shards=8)
    assert tall.layout() == sib.layout() == (188, 8, NBLK) and tall.config() == sib.config() == (1, 3) and tall.near() == sib.near()
    assert tall.streamer() == sib.streamer() == (2, 7)
    for s in (tall, sib):
        s.run(NITER)
    assert tall.census()["grid"] == 1 + 1 + 4 and sib.census()["grid"] == 1 + 1 + 8
    a, b = _full(tall, RC3_MIXED), _full(sib, RC3_MIXED)
    assert len(np.unique(a["delta"][1100:1830])) >= 3 and len(set(a["rc1_annotCat"])) == 3 and np.any(a["beta"][1100:1830] != 0.0)
    _equal(a, b)


# ---- fused passes: one launch serves several chains ---------------------------------------------------------------------------------------
def _seed(c):
    """seed of chain c of a pass.  (With seed 1002 the oracle's chain 1 of the mixed model includes no BayesB locus in its three
    iterations, found on the CPU oracle alone; with 1003 it includes 16 of 230.  _not_vacuous holds every chain to that.)"""
    return 1001 + 2 * c


def _fused(ngp, O, N, models, lag, storage=None, streamer=None, shards=0, oracle=True):
    """Chains c = 0.. (seed 1001 + 2 c, y + 0.01 c, model models[c]) over one panel in one launch per iteration; each must be the chain it
    is alone in the same layout and, where the oracle knows the model, the oracle's chain for that layout.  Returns the leader."""
    K = len(models)
    fused = []
    for c, model in enumerate(models):
        if c == 0:
            first = ngp.Sampler(device=0)
            n = shards or first.shards_for_pass(K)
            first.close()
        fused.append(_handle(ngp, O, N, model, lag, streamer=streamer, storage=storage, shards=n, seed=_seed(c), chain=c, y_shift=0.01 * c,
                             owner=fused[0] if c else None))
    R, S, nb = fused[0].layout()
    assert nb == NBLK and fused[0].config() == (1, lag)
    ngp.Sampler.run_many(fused, NITER)
    pair = fused[0].streamer()[0] == 1 and K >= 4
    assert fused[0].census()["grid"] == K + ((K + 1) // 2 if pair else K) * ((S + 31) // 32) + S     # ONE launch: K samplers, the reducers, S streamers
    for c, model in enumerate(models):
        alone = _handle(ngp, O, N, model, lag, streamer=streamer, storage=storage, shards=S, seed=_seed(c), chain=c, y_shift=0.01 * c)
        assert alone.layout() == (R, S, nb) and alone.config() == (1, lag) and alone.streamer() == fused[0].streamer()
        alone.run(NITER)
        assert alone.census()["grid"] == 1 + (S + 31) // 32 + S
        f = _full(fused[c], model)
        _equal(f, _full(alone, model), ("alone", c))
        if oracle and not any(kind == "RC3" for _, _, kind in model):
            _equal(f, _reference(O, ngp, alone, N, model, storage, seed=_seed(c), chain=c, y_shift=0.01 * c), ("oracle", c))
    assert not np.array_equal(fused[0].get_state()["beta"], fused[1].get_state()["beta"])
    return fused[0]


@pytest.mark.parametrize("K,lag,N,streamer,shards", [(3, 8, 500, None, 0), (3, 6, 500, None, 0), (2, 4, 408, 2, 6)],
                         ids=["three_chains_lag8", "three_chains_lag6", "rows_two_chains_lag4"])
def test_fused_pr_chains(ngp, O, K, lag, N, streamer, shards):
    """k_sweep_multi over fp32 tiles: three chains on the phase streamer (role_streamer_multi, lags 8 and 6), two on the row-owning
    streamer at lag 4 (role_streamer_rows_multi; six shards: a fused grid has to reach past the second sampler's place, block 8)"""
    lead = _fused(ngp, O, N, [PR] * K, lag, streamer=streamer, shards=shards)
    if streamer:
        assert lead.streamer() == (2, 7) and lead.layout()[0] >= 64
    else:
        assert lead.streamer() == (1, 8) and lead.layout()[0] <= 64


@pytest.mark.parametrize("K,lag,N,shards", [(2, 8, 1500, 6), (3, 8, 4000, 12)], ids=["two_chains", "three_chains"])
def test_fused_pr_chains_over_byte_tiles(ngp, O, K, lag, N, shards):
    """k_sweep_multi over byte tiles with two update tasks per lane: the rows of test_fused_chains_over_compact_storage"""
    lead = _fused(ngp, O, N, [PR] * K, lag, storage="u8", shards=shards)
    R = lead.layout()[0]
    assert lead.streamer() == (3, 7) and lead.storage() == 1 and {1: 1, 2: 2, 3: 4, 4: 4}[(4 * (-(-(R // 16) // 7)) + 7) // 8] == 2


def test_fused_mixed_chains(ngp, O):
    """k_sweep_multi_r: two chains of the mixed model (BayesR and sixteen-class lanes in the fused samplers)"""
    lead = _fused(ngp, O, 500, [MIXED] * 2, 6)
    assert lead.streamer() == (1, 8) and lead.layout()[0] <= 64


def test_fused_tuple_chains(ngp, O):
    """k_sweep_multi_tup: two chains with a Tuple set of two correlated sets, 1,300 loci"""
    lead = _fused(ngp, O, 500, [TUP2] * 2, 6)
    assert lead.streamer() == (1, 8) and lead.layout()[0] <= 64


def test_fused_rc_and_plain_chain(ngp, O):
    """k_sweep_multi_rc: chain 0 holds a BayesRCpi set with three annotations, chain 1 the plain mixed model; each is the chain alone
    (full state, rc_state included), and chain 1 the oracle's"""
    lead = _fused(ngp, O, 500, [RC3_MIXED, MIXED], 6)
    assert lead.streamer() == (1, 8) and lead.layout()[0] <= 64
    a = _full(lead, RC3_MIXED)
    assert len(np.unique(a["delta"][1100:1830])) >= 3 and len(set(a["rc1_annotCat"])) == 3 and np.any(a["beta"][1100:1830] != 0.0)
