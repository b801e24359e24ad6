"""Convergence diagnostics without a GPU ("Convergence diagnostics"): the numpy restatement tests/ref_diag.py against
bench.py's ess_geyer, the project's own estimator; api.pool_diagnostics against its formulas written out; the new symbols; and
runLMEM's host checks of diagnostics=."""
import ast
import ctypes as C
import os
import re

import numpy as np
import pytest

import ref_diag as RD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = (3, 4, 5, 37, 200, 1000)
LAGS = (2, 8, 32, 64)
NEW = ["ngp_enable_diagnostics", "ngp_get_diagnostics_layout", "ngp_get_diagnostics", "ngp_get_diagnostics_state", "ngp_set_diagnostics_state",
       "ngp_get_diagnostics_stats"]


def bench_ess_geyer():
    """bench.py's ess_geyer, taken out of its source (importing bench.py sets environment defaults meant for a benchmark process)."""
    tree = ast.parse(open(os.path.join(ROOT, "bench.py")).read())
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "ess_geyer")
    ns = {"np": np}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), "bench.py", "exec"), ns)
    return ns["ess_geyer"]


@pytest.fixture(scope="module")
def series():
    """40 series of 1000 draws: 39 AR(1) with phi from -0.5 to 0.9, scales 1e-6 .. 1e3, offsets up to +-1e4, and one constant.  The seed
    is one at which the positive sequence of every series ends inside 64 lags as bench.ess_geyer's own autocorrelations see it (about one
    realisation in four of the phi = 0.9 series stays positive beyond lag 64 at n = 1000); sequence_end() below checks that."""
    rng = np.random.default_rng(2)
    phi = np.linspace(-0.5, 0.9, 39)
    scale = 10.0 ** rng.permutation(np.linspace(-6.0, 3.0, 39))
    offset = rng.uniform(-1e4, 1e4, size=39)
    e = rng.normal(size=(1000, 39))
    x = np.empty((1000, 39))
    x[0] = e[0] / np.sqrt(1.0 - phi * phi)
    for t in range(1, 1000):
        x[t] = phi * x[t - 1] + e[t]
    return np.concatenate([offset + scale * x, np.full((1000, 1), 123.5)], axis=1)


def sequence_end(x):
    """The lag at which bench.ess_geyer's loop over x stops (its autocorrelations, its loop)."""
    x = x - x.mean()
    n = len(x)
    if not np.any(x):
        return 0
    f = np.fft.rfft(x, 2 * n)
    acf = np.fft.irfft(f * np.conj(f))[:n] / (x @ x)
    k = 0
    while k + 1 < n and acf[k] + acf[k + 1] > 0:
        k += 2
    return k


def test_mirror_against_bench_ess_geyer(series):
    """Where the window did not truncate, the streamed lag-window ESS is bench.ess_geyer's: relative error <= 1e-6 (the two routes round
    differently -- shifted streamed products against an FFT of centred data).  Measured with these series: worst 1.3e-7 (n = 200, L >= 32); n <= 5,
    where tau is a near-cancelling sum: 2.4e-8; n = 1000: 8.4e-9.  At L = 64 no series is truncated at any n.  Mean and variance agree with np.mean /
    np.var(ddof=1) to 1e-9 relative."""
    ess_geyer = bench_ess_geyer()
    worst = {}
    assert max(sequence_end(series[:n, j]) for n in NS for j in range(40)) <= 62        # (the inputs: see series())
    for n in NS:
        x = series[:n]
        want = np.array([ess_geyer(x[:, j]) for j in range(x.shape[1])])
        for L in LAGS:
            f = RD.run(x, lags=L, split=n // 2).finalise()
            ok = f["truncated"] == 0
            if L == 64:
                assert ok.all(), (n, np.flatnonzero(~ok))
            if n <= L:
                assert ok.all()
            err = np.abs(f["ess"][ok] - want[ok]) / want[ok]
            worst[(n, L)] = float(err.max()) if ok.any() else 0.0
            assert np.all(f["ess"][~ok] <= n)
            assert np.allclose(f["mean"], x.mean(axis=0), rtol=1e-9, atol=0)
            assert f["var"][-1] == 0.0 and f["ess"][-1] == n                         # the constant series
            assert np.allclose(f["var"][:-1], x[:, :-1].var(axis=0, ddof=1), rtol=1e-9, atol=0)
            hn = f["half_n"]
            assert hn[0] == n // 2 and hn[1] == n - n // 2
            for h, sl in enumerate((slice(0, n // 2), slice(n // 2, n))):
                assert np.allclose(f["half_mean"][h], x[sl].mean(axis=0), rtol=1e-9, atol=0)
                if hn[h] >= 2:
                    assert np.allclose(f["half_var"][h][:-1], x[sl][:, :-1].var(axis=0, ddof=1), rtol=1e-9, atol=0)
                else:
                    assert np.isnan(f["half_var"][h]).all()
    print("worst relative ESS error per (n, L):", worst)
    assert max(worst.values()) <= 1e-6, worst


def test_truncation_is_reported(series):
    """A slowly mixing series in a short window: the positive sequence has not ended, truncated = 1, and the ESS is an upper bound."""
    ess_geyer = bench_ess_geyer()
    x = series[:, 38:39]                                   # phi = 0.9
    f = RD.run(x, lags=4, split=500).finalise()
    assert f["truncated"][0] == 1 and f["ess"][0] >= ess_geyer(x[:, 0])


def chain_of(x, lags, split):
    return RD.run(x, lags=lags, split=split).finalise()


def test_pool_diagnostics_against_the_formulas(ngp):
    """Offsets of the order of the SD: a half's mean is a double near its offset, so B/n = var(mean_s) carries a relative error of about
    ulp(offset) / spread of the means -- 1e-15 here, far inside the 1e-9 asked of R-hat."""
    rng = np.random.default_rng(5)
    phi, x = np.array([-0.5, 0.2, 0.9]), np.empty((400, 4))
    x[0, :3] = rng.normal(size=3)
    for t in range(1, 400):
        x[t, :3] = phi * x[t - 1, :3] + rng.normal(size=3)
    x[:, :3] += [0.0, 10.0, -3.0]
    x[:, 3] = 123.5                                        # three AR(1) series and a constant one
    chains = [chain_of(x[100 * c:100 * (c + 1)], 8, 50) for c in range(4)]
    got = ngp.pool_diagnostics(chains)
    halves = [x[50 * s:50 * (s + 1)] for s in range(8)]
    W = np.mean([h.var(axis=0, ddof=1) for h in halves], axis=0)
    Bn = np.var([h.mean(axis=0) for h in halves], axis=0, ddof=1)
    vp = 49.0 / 50.0 * W + Bn
    with np.errstate(all="ignore"):
        rhat = np.sqrt(vp / W)
    assert got["n"] == 400 and np.isnan(got["rhat"][3]) and np.isnan(rhat[3])                 # the constant parameter: W = 0
    assert np.allclose(got["rhat"][:3], rhat[:3], rtol=1e-9, atol=0) and np.all(got["rhat"][:3] > 0.9)
    assert np.allclose(got["mean"], x.mean(axis=0), rtol=1e-12, atol=0)
    assert np.allclose(got["sd"][:3], np.sqrt(vp[:3]), rtol=1e-9, atol=0) and got["sd"][3] == 0.0
    assert np.array_equal(got["ess"], sum(c["ess"] for c in chains))
    assert np.allclose(got["mcse"][:3], got["sd"][:3] / np.sqrt(got["ess"][:3]), rtol=1e-15, atol=0)
    assert np.array_equal(got["truncated"], np.any([c["truncated"] > 0 for c in chains], axis=0).astype(float))
    ref = RD.pool(chains)
    assert all(np.array_equal(got[k], ref[k], equal_nan=True) for k in ("mean", "sd", "ess", "mcse", "rhat", "truncated"))
    # one chain: its two halves are the sequences
    one = ngp.pool_diagnostics(chains[:1])
    W1 = np.mean([halves[0].var(axis=0, ddof=1), halves[1].var(axis=0, ddof=1)], axis=0)
    B1 = np.var([halves[0].mean(axis=0), halves[1].mean(axis=0)], axis=0, ddof=1)
    assert np.allclose(one["rhat"][:3], np.sqrt((49.0 / 50.0 * W1[:3] + B1[:3]) / W1[:3]), rtol=1e-9, atol=0) and np.isnan(one["rhat"][3])
    # a half with n_s < 2 is no sequence: split 1 leaves half 0 with one draw, so a single chain has one sequence and no R-hat ...
    lone = chain_of(x[:100], 8, 1)
    assert lone["half_n"][0] == 1 and np.isnan(lone["half_var"][0]).all()
    assert np.isnan(ngp.pool_diagnostics([lone])["rhat"]).all()
    # ... and two such chains have two
    two = ngp.pool_diagnostics([lone, chain_of(x[100:200], 8, 1)])
    seq = [x[1:100], x[101:200]]
    W2 = np.mean([s.var(axis=0, ddof=1) for s in seq], axis=0)
    B2 = np.var([s.mean(axis=0) for s in seq], axis=0, ddof=1)
    assert np.allclose(two["rhat"][:3], np.sqrt((98.0 / 99.0 * W2[:3] + B2[:3]) / W2[:3]), rtol=1e-9, atol=0)


def test_new_symbols_everywhere(ngp):
    import __graft_entry__ as g
    g.build()
    hdr = open(os.path.join(ROOT, "include", "nextgp_hip.h")).read()
    declared = set(re.findall(r"^int32_t (ngp_[a-z0-9_]+)\(", hdr, flags=re.M))
    lib = ngp.load()
    for s in NEW:
        assert s in declared and s in ngp.SYMBOLS and hasattr(lib, s), s
    lib.ngp_abi_version.restype = C.c_int32
    assert lib.ngp_abi_version() == 4
    for m in ("enable_diagnostics", "diagnostics", "diagnostics_names", "diagnostics_state", "set_diagnostics_state", "diagnostics_stats"):
        assert callable(getattr(ngp.Sampler, m))


@pytest.mark.parametrize("bad", [1, "yes", {"lags": 7}, {"lags": 0}, {"lags": 258}, {"lags": 8.0}, {"lag": 8}, {"lags": 8, "split": 2}, [64]])
def test_runlmem_refuses_bad_diagnostics_on_the_host(ngp, tmp_path, bad):
    """Argument mistakes are ValueErrors from host checks before any device work: they come with no device present."""
    with pytest.raises(ValueError, match="diagnostics"):
        ngp.runLMEM("y ~ 1 + SNP(M1,\"nowhere.npy\")", {"y": np.zeros(4)}, 10, 2, 2, outFolder=str(tmp_path / "o"), diagnostics=bad)
    assert not (tmp_path / "o").exists()
