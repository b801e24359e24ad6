"""Weighted residuals (E.str == "D", src/mme.jl:71-75; sampleVarE src/functions.jl:526-528; Mp / mpm src/mme.jl:299-303; fixed sets
src/mme.jl:133-136) on the device.  The library samples the row-scaled problem (s = sqrt(w): tiles s x, residual s ycorr, fixed columns
s X, intercept column s); the yardsticks are the existing blocked oracle, driven through its public calls on that problem, and the
weighted reference-order restatement (tests/ref_numpy_weighted.py)."""
import numpy as np
import pytest

from conftest import add_sets, make_problem
from test_gpu_parity import ENGINES, ENGINE_IDS

pytestmark = pytest.mark.gpu

SPEC = [(0, 400, "PR"), (400, 300, "B"), (700, 200, "C"), (900, 200, "R")]   # 1,100 columns: 18 blocks of 64


def _sampler(ngp, engine=(1, 6), seed=1001, chain=0, w=None):
    s = ngp.Sampler(device=0, seed=seed, chain=chain, mode=engine[0], lag=engine[1], streamer=engine[3] if len(engine) > 3 else 1)
    if len(engine) > 2:
        s.set_near(engine[2])
    if w is not None:
        s.set_residual_weights(w)
    return s


def _everything(s, n):
    st, ps, tr = s.get_state(), s.get_posterior_sums(), s.get_trace(n)
    return st, ps, tr


def _same(a, b):
    (sa, pa, ta), (sb, pb, tb) = a, b
    for k in ("ycorr", "beta", "delta", "varBeta", "piHat"):
        assert np.array_equal(sa[k], sb[k]), k
    assert sa["varE"] == sb["varE"] and sa["b"] == sb["b"] and sa["iter"] == sb["iter"]
    for k in ("sum_beta", "sum_beta2", "sum_delta", "sum_varBeta", "sum_pi"):
        assert np.array_equal(pa[k], pb[k]), k
    assert pa["sum_varE"] == pb["sum_varE"] and pa["sum_b"] == pb["sum_b"] and pa["nKept"] == pb["nKept"]
    assert np.array_equal(ta["varE"], tb["varE"]) and np.array_equal(ta["b"], tb["b"])


def _scaled_tiles(s, G, w):
    """The fp32 tiles the header's formula gives: (float)(s_i * ((double)x_ij - mu_j)), mu the device's column means."""
    mu = s.means()
    return (np.sqrt(w)[:, None] * (np.asarray(G, np.float64) - mu[None, :])).astype(np.float32)


@pytest.mark.parametrize("engine", ENGINES, ids=ENGINE_IDS)
def test_all_ones_weights_are_the_unweighted_chain(ngp, O, engine):
    N, P, n = 200, 1100, 8
    X, y, bt, v = make_problem(O, N, P, seed=4)
    runs = []
    for w in (None, np.ones(N)):
        s = _sampler(ngp, engine, w=w)
        s.set_panel(X)
        add_sets(s, SPEC, v)
        s.add_fixed_set(np.linspace(-1.0, 1.0, N))
        s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var()); s.set_schedule(n, 2, 2); s.run(n)
        runs.append(_everything(s, n))
    _same(runs[0], runs[1])


def test_all_ones_weights_tuple_and_fused_chains(ngp, O):
    from test_gpu_tuple import add_tuple, tuple_problem
    N, nloc, k = 300, 90, 2
    Xp, y, vm, v, span, off = tuple_problem(O, ngp, N, nloc, k, extra=40)
    regions = [(0, nloc // 3), (nloc // 3, nloc)]
    runs = []
    for w in (None, np.ones(N)):
        s = _sampler(ngp, (1, 6), seed=21, w=w)
        s.set_panel(Xp)
        add_tuple(s, nloc, k, vm, regions)
        s.add_marker_set(off, 40, 1, 4.0, v * 0.5, [(j, j + 1) for j in range(40)], [v] * 40, pi0=0.2, estPi=True)
        s.set_y(y); s.set_residual_prior(4.0, 0.5); s.set_schedule(10, 2, 2); s.run(10)
        runs.append(_everything(s, 10))
    _same(runs[0], runs[1])
    # three fused chains (ngp_run_many over one shared panel): all-ones weights on the owner reach every chain
    Xf, yf, _, vf = make_problem(O, 300, 1100, seed=6)
    fused = []
    for w in (None, np.ones(300)):
        chains = _fused_chains(ngp, Xf, yf, vf, 3, w)
        ngp.Sampler.run_many(chains, 10)
        fused.append([_everything(c, 10) for c in chains])
    for a, b in zip(*fused):
        _same(a, b)


def _fused_chains(ngp, X, y, v, K, w, spec=SPEC):
    chains = []
    for c in range(K):
        s = ngp.Sampler(device=0, seed=1001 + c, chain=c)
        if c == 0:
            if w is not None:
                s.set_residual_weights(w)
            s.set_max_shards(s.shards_for_pass(K))
            s.set_panel(X)
        else:
            s.share_panel(chains[0])
        add_sets(s, spec, v)
        s.set_y(y + 0.01 * c); s.set_residual_prior(4.0, 1.0); s.set_schedule(10, 2, 2)
        chains.append(s)
    return chains


def _weighted_problem(O, N, P, seed=3):
    X, y, bt, v = make_problem(O, N, P, seed=seed)
    rng = np.random.default_rng(seed + 100)
    G = np.rint(X.astype(np.float64) - X.min(axis=0))        # raw genotype-like codes, centred again on the device
    w = rng.uniform(0.2, 5.0, N)
    return G, y, v, w


@pytest.mark.parametrize("engine", [(0, 1), (1, 6), (1, 8, 4), (1, 6, 2, 2)], ids=["blocklaunch", "persist_lag6", "persist_lag8_near4", "rows_lag6_near2"])
def test_weighted_chain_bit_exact_vs_blocked_oracle_on_the_row_scaled_problem(ngp, O, engine):
    N, P, n = 260, 1100, 10
    G, y, v, w = _weighted_problem(O, N, P)
    sq = np.sqrt(w)
    rng = np.random.default_rng(11)
    C3 = rng.normal(size=(N, 3))
    s = _sampler(ngp, engine, w=w)
    s.set_panel(G, centre=True)
    assert np.array_equal(s.residual_weights(), w)
    R, S, _ = s.layout()
    mode, D = s.config()
    o = O.Oracle(order=1, seed=1001, chain=0)
    o.set_panel_f32(_scaled_tiles(s, G, w), R=R, S=S, D=D, near=s.near(), nchain=s.streamer()[1], tform=s.chain_form())
    s.add_fixed_set(np.ones(N)); s.add_fixed_set(C3)              # the device scales the columns ...
    o.add_fixed_set(sq); o.add_fixed_set(sq[:, None] * C3)       # ... the oracle is handed them scaled
    for m, yy in ((s, y), (o, sq * y)):
        add_sets(m, SPEC, v)
        m.set_intercept(False); m.set_y(yy); m.set_residual_prior(4.0, 0.25 * y.var()); m.set_schedule(n, 2, 2); m.run(n)
    a, b = s.get_state(), o.get_state()
    for k in ("beta", "delta", "varBeta", "piHat"):
        assert np.array_equal(a[k], b[k][:len(a[k])]), k
    assert np.array_equal(a["ycorr"], b["ycorr"][:N] / sq)
    assert a["varE"] == b["varE"] and np.array_equal(s.get_trace(n)["varE"], o.get_trace(n)["varE"])
    assert np.array_equal(s.get_fixed()["b"], o.get_fixed()["b"])
    pa, pb = s.get_posterior_sums(), o.get_posterior_sums()
    for k in ("sum_beta", "sum_beta2", "sum_delta", "sum_varBeta", "sum_pi"):
        assert np.array_equal(pa[k], pb[k][:len(pa[k])]), k
    assert pa["sum_varE"] == pb["sum_varE"] and pa["nKept"] == pb["nKept"]
    assert np.array_equal(s.get_class_state(3)["piHat"], o.get_class_state(3)["piHat"])


def test_weighted_fused_chains_equal_the_chains_alone(ngp, O):
    N, P, K = 300, 1100, 3
    G, y, v, w = _weighted_problem(O, N, P, seed=5)
    fused = _fused_chains(ngp, G, y, v, K, w)
    for c in fused[1:]:
        assert np.array_equal(c.residual_weights(), w)           # a sharer takes the owner's weights
    R, S, _ = fused[0].layout()
    ngp.Sampler.run_many(fused, 10)
    assert fused[0].census()["grid"] == K + K * ((S + 31) // 32) + S     # one fused launch served the three weighted chains
    for c in range(K):
        alone = ngp.Sampler(device=0, seed=1001 + c, chain=c)
        alone.set_residual_weights(w); alone.set_max_shards(S); alone.set_panel(G)
        add_sets(alone, SPEC, v)
        alone.set_y(y + 0.01 * c); alone.set_residual_prior(4.0, 1.0); alone.set_schedule(10, 2, 2); alone.run(10)
        _same(_everything(fused[c], 10), _everything(alone, 10))


def _ref(O, s, G, y, w, seed, chain, intercept=True):
    from ref_numpy_weighted import WeightedRefChain
    Xeff = _scaled_tiles(s, G, w).astype(np.float64) / np.sqrt(w)[:, None]   # the panel the device samples, unscaled
    ref = WeightedRefChain(O, Xeff, y, w, seed=seed, chain=chain, intercept=intercept)
    ref.add_marker_set, ref.add_marker_set_r = ref.add_set, ref.add_set_r     # (conftest.add_sets speaks the library's names)
    return ref


def _close(a, b, tol=1e-9, floor=1e-6):
    a, b = np.asarray(a, float), np.asarray(b, float)
    return np.abs(a - b).max() <= tol * max(floor, np.abs(b).max())


@pytest.mark.parametrize("kind", ["PR", "B", "C", "R"])
def test_weighted_chain_vs_weighted_reference_order(ngp, O, kind):
    N, P = 240, 300
    G, y, v, w = _weighted_problem(O, N, P, seed=7)
    s = _sampler(ngp, (1, 6), seed=31, chain=1, w=w)
    s.set_panel(G, centre=True)
    ref = _ref(O, s, G, y, w, seed=31, chain=1)
    add_sets(s, [(0, P, kind)], v); add_sets(ref, [(0, P, kind)], v)
    s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var())
    ref.E_df, ref.E_scale = 4.0, 0.25 * y.var()
    for it in range(4):
        s.run(1); ref.run(1)
        a, b = s.get_state(), ref.state()
        assert np.array_equal(a["delta"], b["delta"]), it
        for k in ("beta", "ycorr", "varBeta"):
            assert _close(a[k], b[k]), (it, k)
        assert abs(a["varE"] - b["varE"]) <= 1e-9 * b["varE"] and abs(a["b"] - b["b"]) <= 1e-9 * max(1.0, abs(b["b"]))
        if kind == "R":
            assert _close(s.get_class_state(0)["piHat"], b["class_pi"][0])
        elif kind != "PR":
            assert _close(a["piHat"], b["piHat"])


def test_fine_seam_with_weights(ngp, O):
    import torch
    N, P = 240, 300
    G, y, v, w = _weighted_problem(O, N, P, seed=8)
    ycorr0 = y - y.mean()
    out = {}
    for dev in (False, True):
        s = _sampler(ngp, (1, 6), seed=5, w=w)
        s.set_panel(G, centre=True)
        add_sets(s, [(0, P, "PR")], v)
        ref = _ref(O, s, G, ycorr0, w, seed=5, chain=0, intercept=False)
        add_sets(ref, [(0, P, "PR")], v)
        ref.iter = 1                                           # the first fine-seam call of set 0 draws as iteration 1
        ref.sampleBayesPR(0, 1.3)
        ycorr, beta, vb = ycorr0.copy(), np.zeros(P), np.array([v])
        if dev:
            t = {k: torch.tensor(a, dtype=torch.float64, device="cuda:0") for k, a in (("ycorr", ycorr), ("beta", beta), ("vb", vb))}
            torch.cuda.synchronize()
            s.sweep_set_dev(0, 1.3, t["ycorr"].data_ptr(), t["beta"].data_ptr(), t["vb"].data_ptr())
            ycorr, beta, vb = t["ycorr"].cpu().numpy(), t["beta"].cpu().numpy(), t["vb"].cpu().numpy()
        else:
            s.sweep_set(0, 1.3, ycorr, beta, vb)
        assert _close(beta, ref.beta[0]) and _close(vb, ref.varBeta[0])
        assert _close(ycorr, ref.ycorr)                        # unscaled terms, as the caller holds ycorr
        assert np.abs(ycorr - (ycorr0 - s.xbeta(beta))).max() <= 1e-9 * np.abs(ycorr0).max()
        out[dev] = (ycorr, beta)
    assert np.array_equal(out[False][0], out[True][0]) and np.array_equal(out[False][1], out[True][1])


def test_weighted_state_is_consistent_and_mpm_is_xWx(ngp, O):
    N, P = 260, 400
    G, y, v, w = _weighted_problem(O, N, P, seed=9)
    sq = np.sqrt(w)
    Xf = np.random.default_rng(2).normal(size=(N, 2))
    s = _sampler(ngp, (1, 6), w=w)
    s.set_panel(G, centre=True)
    Xt = _scaled_tiles(s, G, w).astype(np.float64)
    assert _close(s.mpm(), (Xt * Xt).sum(axis=0), tol=1e-12)      # x'Wx out of the scaled tiles
    s.add_fixed_set(Xf)
    add_sets(s, [(0, 200, "PR"), (200, 200, "B")], v)
    s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var()); s.run(12)
    st = s.get_state()
    xb = (Xt @ st["beta"]) / sq
    assert _close(s.xbeta(st["beta"]), xb, tol=1e-12)
    expect = y - st["b"] - Xf @ s.get_fixed()["b"] - xb
    assert np.abs(st["ycorr"] - expect).max() <= 1e-9 * np.abs(y).max()


def test_weighted_snapshot_resumes_bit_for_bit_and_refuses_other_weights(ngp, O, tmp_path):
    N, P = 200, 300
    G, y, v, w = _weighted_problem(O, N, P, seed=10)

    def model(weights):
        s = _sampler(ngp, (1, 6), seed=3, w=weights)
        s.set_panel(G, centre=True)
        add_sets(s, [(0, 150, "PR"), (150, 150, "C")], v)
        s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var()); s.set_schedule(14, 2, 2)
        return s
    a = model(w)
    a.run(6)
    snap = str(tmp_path / "w.snap")
    a.save_snapshot(snap)
    a.run(8)
    b = model(w)
    b.load_snapshot(snap)
    b.run(8)
    sa, sb = a.get_state(), b.get_state()
    for k in ("ycorr", "beta", "delta", "varBeta", "piHat"):
        assert np.array_equal(sa[k], sb[k]), k
    assert sa["varE"] == sb["varE"] and a.get_posterior_sums()["sum_beta"].tolist() == b.get_posterior_sums()["sum_beta"].tolist()
    with pytest.raises(ngp.NextGPHipError, match="residual weights"):
        model(w * 1.01).load_snapshot(snap)
    with pytest.raises(ngp.NextGPHipError, match="residual weights"):
        model(None).load_snapshot(snap)


def test_weight_errors_leave_a_usable_handle(ngp, O):
    N, P = 200, 256
    X, y, bt, v = make_problem(O, N, P, seed=12)
    s = ngp.Sampler(device=0, seed=7, chain=0)
    good = np.ones(N)
    for bad in (np.r_[good[:-1], 0.0], np.r_[good[:-1], -2.0], np.r_[good[:-1], np.nan], np.r_[good[:-1], np.inf]):
        with pytest.raises(ngp.NextGPHipError, match="error -1"):
            s.set_residual_weights(bad)
    s.set_storage("u8")
    with pytest.raises(ngp.NextGPHipError, match="error -1.*compact storage"):
        s.set_residual_weights(good)
    s.set_storage("f32")
    s.set_residual_weights(good[:-1])                            # N is checked against the panel
    with pytest.raises(ngp.NextGPHipError, match="error -1"):
        s.set_panel(X)
    with pytest.raises(ngp.NextGPHipError, match="error -1.*compact storage"):
        s.set_storage("u8")
    s.set_residual_weights(None)
    assert s.residual_weights() is None
    s.set_panel(X)
    with pytest.raises(ngp.NextGPHipError, match="error -2"):
        s.set_residual_weights(good)
    R, S, _ = s.layout()
    o = O.Oracle(order=1, seed=7, chain=0)
    o.set_panel_f32(X, R=R, S=S, D=s.config()[1], near=s.near(), nchain=s.streamer()[1], tform=s.chain_form())
    for m in (s, o):
        add_sets(m, [(0, P, "PR")], v); m.set_y(y); m.set_residual_prior(4.0, 0.25 * y.var()); m.run(6)
    with pytest.raises(ngp.NextGPHipError, match="error -2"):
        s.set_residual_weights(good)
    a, b = s.get_state(), o.get_state()
    assert np.array_equal(a["beta"], b["beta"]) and np.array_equal(a["ycorr"], b["ycorr"][:N]) and a["varE"] == b["varE"]


def test_runLMEM_with_weighted_residuals(ngp, O, tmp_path):
    N, P = 300, 200
    G, y, v, w = _weighted_problem(O, N, P, seed=13)
    d = 1.0 / w
    geno = tmp_path / "g.txt"
    np.savetxt(geno, G, fmt="%d", delimiter=" ")
    VCV = {"M": ngp.BayesPR(9999, v), "e": ngp.Random(d, 0.5 * y.var())}
    f = f'y ~ 1 + SNP(M,"{geno}")'
    nChain, nBurn, nThin = 8, 2, 2
    for K in (1, 3):
        out = tmp_path / f"out{K}"
        res = ngp.runLMEM(f, {"y": y}, nChain, nBurn, nThin, outFolder=str(out), VCV=VCV, seed=9, chains=K)
        first = res["samplers"][0] if K > 1 else res["sampler"]
        wr = 1.0 / d
        assert np.array_equal(first.residual_weights(), wr)
        folders = [out] if K == 1 else [out / f"chain{c}" for c in range(K)]
        for fo in folders:
            for name in ("b", "varE", "betaM", "varM"):
                assert len((fo / f"{name}Out").read_text().splitlines()) == 1 + 3, name
        means = []
        for c in range(K):
            ref = _ref(O, first, G, y, wr, seed=9, chain=c)
            add_sets(ref, [(0, P, "PR")], v)
            ref.E_df, ref.E_scale = 4.0, 0.5 * y.var() * 0.5
            kept = []
            for it in range(1, nChain + 1):
                ref.run(1)
                if it >= nBurn + nThin and (it - nBurn) % nThin == 0:
                    kept.append((ref.beta[0].copy(), ref.varE, float(ref.b[0])))
            means.append([np.mean([k[i] for k in kept], axis=0) for i in range(3)])
        mb = np.mean([m[0] for m in means], axis=0)
        assert res["nKept"] == 3 * K
        assert _close(res["sets"]["M"]["beta"], mb, tol=1e-8)
        assert abs(res["varE"] - np.mean([m[1] for m in means])) <= 1e-8 * res["varE"]
