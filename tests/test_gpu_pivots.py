"""Law tests on the device: the models of tests/test_pivots_host.py on the library's default plan, ngp_run(1) at a time, the state
read back after every iteration, every conditional draw held to its closed-form law (tests/pivots.py).  One engine is enough: the
others are held bit for bit to this one elsewhere.  The device's bits are the blocked oracle's, so for the oracle-covered models the
figures are those of the host test's blocked order; weighted random-effect sets have no host chain and are checked here only."""
import numpy as np
import pytest

import pivot_models as PM

pytestmark = pytest.mark.gpu

GPU_MODELS = PM.MARKER + PM.RANDOM + [m + "_w" for m in PM.RANDOM]


def device_chain(ngp, O, name):
    spec = PM.build(O, name)
    s = ngp.Sampler(device=0, seed=PM.SEED, chain=0)
    if spec["w"] is not None:
        s.set_residual_weights(spec["w"])
    s.set_panel(spec["X"])
    PM.apply_handle(s, spec, device=True)
    return spec, s, PM.record(lambda: s.run(1), lambda: PM.state_handle(s, spec), spec)


@pytest.mark.parametrize("name", GPU_MODELS)
def test_device_draws_follow_their_laws(ngp, O, name):
    spec, s, states = device_chain(ngp, O, name)
    PM.check(PM.walk(spec, states, device=True), f"{name}/gpu")


def test_class_search_of_twelve_classes(ngp, O):
    """The BayesR set over all-zero columns of tests/test_pivots_host.py on the device: the class counts and the independence of
    neighbouring loci's comparisons, and -- a BayesR set over zero columns had no parity case -- the blocked oracle's chain bit for bit."""
    spec, s, states = device_chain(ngp, O, "search")
    cls = np.array([st["delta"][64:] for st in states[1:]])
    fig = PM.class_search_figures(cls, "search/gpu")
    assert all(p > PM.KS_MIN for p in fig.values()), fig
    PM.check(PM.walk(spec, states, device=True), "search/gpu")
    R, S, _ = s.layout()
    o = O.Oracle(order=1, seed=PM.SEED, chain=0)
    o.set_panel_f32(spec["X"], R=R, S=S, D=s.config()[1], near=s.near(), nchain=s.streamer()[1], tform=s.chain_form())
    PM.apply_handle(o, spec)
    for t in range(spec["iters"]):
        o.run(1)
        a, b = states[t + 1], PM.state_handle(o, spec)
        for k in ("ycorr", "beta", "delta"):
            assert np.array_equal(a[k], b[k]), (t, k)
        assert a["varE"] == b["varE"] and a["b"] == b["b"] and all(np.array_equal(x, y) for x, y in zip(a["varBeta"], b["varBeta"])), t
