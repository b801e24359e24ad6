"""Fixed-effect sets given as sparse matrices (ngp_add_fixed_set_sparse; kernels in csrc/ngp_fixed_sparse.h).  Yardsticks: the dense set
of the same design and the blocked C oracle (bit for bit, designs of at most 64 columns), the restatement tests/ref_fixed_sparse.py (bit
for bit, designs wider than any dense set) and the reference's order (ref_numpy.RefChain.add_fixed on the dense expansion, to the
relative bound 1e-9 that test_gpu_parity.test_fixed_effect_sets_beyond_the_intercept applies to the dense set).

N = 2100: three 1024-row rounds of the column sums, the last one partial, not a multiple of 64.  Every factor has a level whose records
are {5, 1029, 2053} (one accumulator, adjacent entries, three rounds), a level with one record and a level with 100 records inside the
first round (two chunks of 64)."""
import os

import numpy as np
import pytest

import ref_fixed_sparse as RF
import ref_random as RR
from conftest import add_sets, make_problem

pytestmark = pytest.mark.gpu

N, P = 2100, 128
TRIPLE, SINGLE, BLOCK = np.array([5, 1029, 2053]), 777, np.arange(100, 200)


def factor(nlev, seed):
    """Codes of a factor of nlev levels (-1 the base level, nlev - 1 columns): the last three columns are the special levels."""
    rng = np.random.default_rng(seed)
    ncol = nlev - 1
    code = np.full(N, -2, dtype=np.int64)
    code[TRIPLE], code[SINGLE], code[BLOCK] = ncol - 1, ncol - 2, ncol - 3
    rest = np.nonzero(code == -2)[0]
    pool = np.arange(-1, ncol - 3)
    fill = np.concatenate([pool, rng.choice(pool, size=len(rest) - len(pool))])
    code[rest] = fill[rng.permutation(len(rest))]
    return code


def dense_of(codes, cov=None):
    cols = [(c[:, None] == np.arange(c.max() + 1)[None, :]).astype(np.float64) for c in codes]
    if cov is not None:
        cols.append(cov)
    return np.asfortranarray(np.column_stack(cols))


def small_designs():
    rng = np.random.default_rng(12)
    return {"factor40": ([factor(40, 1)], None), "block36": ([factor(6, 2), factor(30, 3)], rng.normal(size=(N, 2)))}


def wide_designs():
    rng = np.random.default_rng(13)
    return {"factor150": ([factor(150, 4)], None), "crossed156": ([factor(150, 5), factor(7, 6)], rng.normal(size=(N, 1)))}


@pytest.fixture(scope="module")
def problem(O):
    X, y, _, v = make_problem(O, N, P, seed=6)
    return X, y, v


def effects(codes, cov, seed=0):
    """A phenotype part from the design, so that the levels matter."""
    rng = np.random.default_rng(100 + seed)
    out = np.zeros(N)
    for c in codes:
        e = np.concatenate([rng.normal(size=c.max() + 1), [0.0]])
        out += e[c]                                                 # (code -1 reads the appended 0)
    if cov is not None:
        out += cov @ rng.normal(size=cov.shape[1])
    return out


def with_panel(ngp, X, y, v, add_fixed, seed=7, chain=0, w=None, share=None, max_shards=None, holdout=None, sched=(12, 2, 2)):
    s = ngp.Sampler(device=0, seed=seed, chain=chain)
    if w is not None:
        s.set_residual_weights(w)
    if max_shards:
        s.set_max_shards(max_shards)
    if share is not None:
        s.share_panel(share)
    else:
        s.set_panel(X)
    add_fixed(s)
    add_sets(s, [(0, P, "PR")], v)
    if holdout is not None:
        s.set_holdout(holdout)
    yvar = np.nanvar(y) if holdout is not None else y.var()         # (held-out rows may carry NaN)
    s.set_y(y); s.set_residual_prior(4.0, 0.25 * yvar); s.set_schedule(*sched)
    return s


def everything(s):
    st, fx, ps = s.get_state(), s.get_fixed(), s.get_posterior_sums()
    return dict(b=fx["b"], sum_b=fx["sum_b"], ycorr=st["ycorr"], beta=st["beta"], varE=np.array(st["varE"]), mu=np.array(st["b"]),
                sum_beta=ps["sum_beta"], varBeta=st["varBeta"])


def same(a, b, keys=None):
    for k in keys or a:
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("name", ["factor40", "block36"])
def test_sparse_is_dense_is_oracle(ngp, O, problem, name):
    X, y, v = problem
    codes, cov = small_designs()[name]
    Xd = dense_of(codes, cov)
    y = y + effects(codes, cov) * np.sqrt(y.var())
    csc = ngp.factors_csc(codes, cov)
    assert csc[1] == Xd.shape[1] <= 64 and np.array_equal(RF.dense_of_csc(*csc), Xd)
    dep = RF.depths(RF.xpx_rows(*csc))
    assert max(dep) == 0 if name == "factor40" else max(dep) >= 3
    d = with_panel(ngp, X, y, v, lambda s: s.add_fixed_set(Xd))
    sp = with_panel(ngp, X, y, v, lambda s: s.add_fixed_factors(codes, cov))
    R, S, _ = d.layout()
    o = O.Oracle(order=1, seed=7, chain=0)
    o.set_panel_f32(X, R=R, S=S, D=d.config()[1], near=d.near(), nchain=d.streamer()[1], tform=d.chain_form())
    o.add_fixed_set(Xd); add_sets(o, [(0, P, "PR")], v)
    o.set_y(y); o.set_residual_prior(4.0, 0.25 * y.var()); o.set_schedule(12, 2, 2)
    for m in (d, sp, o):
        m.run(12)
    ed, es = everything(d), everything(sp)
    same(ed, es)
    fo, so = o.get_fixed(), o.get_state()
    assert np.array_equal(es["b"], fo["b"]) and np.array_equal(es["sum_b"], fo["sum_b"])
    assert np.array_equal(es["ycorr"], so["ycorr"]) and np.array_equal(es["beta"], so["beta"]) and es["varE"] == so["varE"]
    assert np.abs(es["b"]).max() > 0 and np.abs(es["sum_b"]).max() > 0
    # once more under residual weights (device only): the values are scaled on the host, the one multiply of the dense set's row scaling
    w = np.random.default_rng(3).uniform(0.3, 3.0, N)
    d = with_panel(ngp, X, y, v, lambda s: s.add_fixed_set(Xd), w=w)
    sp = with_panel(ngp, X, y, v, lambda s: s.add_fixed_factors(codes, cov), w=w)
    d.run(12); sp.run(12)
    ew = everything(sp)
    same(everything(d), ew)
    assert not np.array_equal(ew["b"], es["b"])


VARE, Q = 1.7, 25


def records_only(ngp, codes, cov, y, level, seed=19, chain=1):
    s = ngp.Sampler(device=0, seed=seed, chain=chain)
    s.set_records(N)
    s.set_intercept(False)
    s.fix_residual_variance(VARE)
    fid = s.add_fixed_factors(codes, cov)
    rid = s.add_random_set(level, Q, df=4.0, scale=0.6, varU0=1.2)
    assert (fid, rid) == (0, 0)
    s.set_y(y); s.set_schedule(40, 10, 1)
    return s


@pytest.mark.parametrize("name", ["factor150", "crossed156"])
def test_wider_than_any_dense_set(ngp, O, name):
    codes, cov = wide_designs()[name]
    rng = np.random.default_rng(21)
    level = rng.integers(0, Q, size=N)
    y = effects(codes, cov, seed=1) * 2.0 + rng.normal(size=Q)[level] + rng.normal(size=N) * np.sqrt(VARE)
    n_, ncol, cp, row, val = ngp.factors_csc(codes, cov)
    assert ncol > 64 and ncol == {"factor150": 149, "crossed156": 156}[name]
    built = (RF.csr_of_csc(N, ncol, cp, row, val), RF.xpx_rows(N, ncol, cp, row, val), None)
    s = records_only(ngp, codes, cov, y, level)
    # one iteration, then three in all: the fixed step of the restatement, chained with the blocked restatement of the (1|g) step
    zpz = RR.zpz_of(level, Q)
    yc, b, u, varU = y.copy(), np.zeros(ncol), np.zeros(Q), 1.2
    for it in (1, 2, 3):
        b, yc = RF.sparse_step(O, 19, 1, it, 0, N, ncol, cp, row, val, yc, b, VARE, built=built)
        yt, u, varU = RR.random_step_blocked(O, 19, 1, it, 0, yc, None, level, Q, None, zpz, u, varU, VARE, 4.0, 0.6)
        yc = np.array(yt)
        s.run(1)
        assert np.array_equal(s.get_fixed()["b"], b), it
        assert np.array_equal(s.get_random(0)["u"], np.array(u)) and s.get_random(0)["varU"] == varU, it
        assert np.array_equal(s.get_state()["ycorr"], yc), it
    assert np.abs(b).max() > 0
    # 40 iterations against the reference's order on the dense expansion
    Xd = dense_of(codes, cov)
    ref = RR.RandomRefChain(O, np.zeros((N, 0)), y, seed=19, chain=1, intercept=False)
    ref.sampleVarE = lambda: VARE                                   # (the handle holds varE: ngp_fix_residual_variance)
    ref.add_fixed(Xd)
    ref.add_random(level, Q, None, df=4.0, scale=0.6, v=1.2)
    s = records_only(ngp, codes, cov, y, level)
    s.run(40); ref.run(40)
    fb, rb = s.get_fixed()["b"], ref.Xfix[0]["b"]
    print(name, "max |b - ref| / max |ref| =", np.abs(fb - rb).max() / np.abs(rb).max())
    assert np.abs(fb - rb).max() <= 1e-9 * np.abs(rb).max()         # the bound of test_fixed_effect_sets_beyond_the_intercept, relative
    uu = s.get_random(0)["u"]
    resid = y - Xd @ fb - uu[level]
    assert np.abs(s.get_state()["ycorr"] - resid).max() <= 1e-9 * np.abs(y).max()
    assert s.get_fixed()["sum_b"].shape == (ncol,) and np.abs(s.get_fixed()["sum_b"]).max() > 0


def test_snapshot_resume_and_get_set_fixed(ngp, O, problem, tmp_path):
    X, y, v = problem
    codes, cov = wide_designs()["crossed156"]
    y = y + effects(codes, cov) * np.sqrt(y.var())
    add = lambda s: s.add_fixed_factors(codes, cov)
    a = with_panel(ngp, X, y, v, add); a.run(12)
    b = with_panel(ngp, X, y, v, add); b.run(5)
    path = str(tmp_path / "fs.ngpsnap")
    b.save_snapshot(path)
    c = with_panel(ngp, X, y, v, add, seed=1, chain=9)
    c.load_snapshot(path); c.run(7)
    same(everything(a), everything(c))
    # a handle without the set, or with a narrower one, does not take the snapshot
    e = with_panel(ngp, X, y, v, lambda s: None)
    with pytest.raises(ngp.NextGPHipError):
        e.load_snapshot(path)
    e = with_panel(ngp, X, y, v, lambda s: s.add_fixed_factors(codes, None))
    with pytest.raises(ngp.NextGPHipError):
        e.load_snapshot(path)
    e.run(1)
    # get_fixed / set_fixed carry the set's columns
    fx = a.get_fixed()
    assert fx["b"].shape == (156,) and fx["sum_b"].shape == (156,)
    c.set_fixed(b=fx["b"] * 2.0, sum_b=fx["sum_b"] + 1.0)
    g = c.get_fixed()
    assert np.array_equal(g["b"], fx["b"] * 2.0) and np.array_equal(g["sum_b"], fx["sum_b"] + 1.0)
    c.set_fixed(b=fx["b"], sum_b=fx["sum_b"])
    a.set_schedule(14, 2, 2); c.set_schedule(14, 2, 2)
    a.run(2); c.run(2)
    same(everything(a), everything(c))
    # the packed posterior carries them: one more entry per column than the same model without the set
    assert a.posterior_len() - with_panel(ngp, X, y, v, lambda s: None).posterior_len() == 156


def test_dense_snapshot_loads_into_the_sparse_twin(ngp, O, problem, tmp_path):
    X, y, v = problem
    codes, cov = small_designs()["block36"]
    Xd = dense_of(codes, cov)
    y = y + effects(codes, cov) * np.sqrt(y.var())
    d = with_panel(ngp, X, y, v, lambda s: s.add_fixed_set(Xd)); d.run(5)
    sp = with_panel(ngp, X, y, v, lambda s: s.add_fixed_factors(codes, cov))
    pd, ps = str(tmp_path / "d.ngpsnap"), str(tmp_path / "s.ngpsnap")
    d.save_snapshot(pd)
    sp.load_snapshot(pd)
    d.run(7); sp.run(7)
    same(everything(d), everything(sp))
    sp.save_snapshot(ps); d.save_snapshot(pd)
    assert open(ps, "rb").read() == open(pd, "rb").read()           # the same chain: the same file
    # mixed with a dense single column in front: the set id enters the draw keys, the order added is the sampling order
    x1 = np.linspace(-1, 1, N)
    m1 = with_panel(ngp, X, y, v, lambda s: (s.add_fixed_set(x1), s.add_fixed_set(Xd)))
    m2 = with_panel(ngp, X, y, v, lambda s: (s.add_fixed_set(x1), s.add_fixed_factors(codes, cov)))
    m1.run(6); m2.run(6)
    same(everything(m1), everything(m2))
    assert not np.array_equal(everything(m2)["b"][1:], everything(sp)["b"])


def test_two_chains_through_run_many(ngp, O, problem):
    X, y, v = problem
    codes, cov = wide_designs()["factor150"]
    y = y + effects(codes, cov) * np.sqrt(y.var())
    add = lambda s: s.add_fixed_factors(codes, cov)
    first = ngp.Sampler(device=0, seed=11, chain=0)
    ms = first.shards_for_pass(2)
    first.close()
    chains = [with_panel(ngp, X, y, v, add, seed=11, chain=0, max_shards=ms)]
    chains.append(with_panel(ngp, X, y + 0.01, v, add, seed=11, chain=1, max_shards=ms, share=chains[0]))
    ngp.Sampler.run_many(chains, 12)
    for c in range(2):
        alone = with_panel(ngp, X, y + 0.01 * c, v, add, seed=11, chain=c, max_shards=ms)
        alone.run(12)
        same(everything(chains[c]), everything(alone))
    assert not np.array_equal(chains[0].get_fixed()["b"], chains[1].get_fixed()["b"])
    # records only, two handles side by side
    level = np.random.default_rng(2).integers(0, Q, size=N)
    yy = y - y.mean()
    pair = [records_only(ngp, codes, cov, yy, level, chain=c) for c in (0, 1)]
    ngp.Sampler.run_many(pair, 6)
    for c in (0, 1):
        alone = records_only(ngp, codes, cov, yy, level, chain=c)
        alone.run(6)
        assert np.array_equal(pair[c].get_fixed()["b"], alone.get_fixed()["b"]) and np.array_equal(pair[c].get_fixed()["sum_b"], alone.get_fixed()["sum_b"])
        assert np.array_equal(pair[c].get_state()["ycorr"], alone.get_state()["ycorr"])


def test_holdout_rows_that_empty_a_level(ngp, O, problem):
    """The records of two levels are all held out: their phenotypes are redrawn every iteration, the columns keep their entries, and the
    level's effect is drawn from what the redrawn records say.  Dense and sparse stay the same chain."""
    X, y, v = problem
    codes, cov = small_designs()["block36"]
    Xd = dense_of(codes, cov)
    y = y + effects(codes, cov) * np.sqrt(y.var())
    rows = np.sort(np.concatenate([TRIPLE, [SINGLE]])).astype(np.int64)
    yh = y.copy(); yh[rows] = np.nan
    d = with_panel(ngp, X, yh, v, lambda s: s.add_fixed_set(Xd), holdout=rows)
    sp = with_panel(ngp, X, yh, v, lambda s: s.add_fixed_factors(codes, cov), holdout=rows)
    d.run(12); sp.run(12)
    es = everything(sp)
    same(everything(d), es)
    hd, hs = d.holdout_state(), sp.holdout_state()
    for k in ("yaug", "sum_fit", "sum_fit2", "n_fit"):
        assert np.array_equal(hd[k], hs[k]), k
    assert np.all(np.isfinite(es["b"])) and np.all(hs["n_fit"][rows] == 5)
    wide, wcov = wide_designs()["crossed156"]
    w = with_panel(ngp, X, yh, v, lambda s: s.add_fixed_factors(wide, wcov), holdout=rows)
    w.run(12)
    assert np.all(np.isfinite(w.get_fixed()["b"])) and np.all(np.isfinite(w.get_state()["ycorr"]))


def test_refusals_leave_a_handle_that_runs(ngp, O, problem):
    X, y, v = problem
    codes, cov = wide_designs()["factor150"]
    n_, ncol, cp, row, val = ngp.factors_csc(codes, cov)
    s = ngp.Sampler(device=0, seed=3, chain=0)
    s.set_panel(X)

    def refused(N_, ncol_, cp_, row_, val_):
        with pytest.raises(ngp.NextGPHipError):
            s.add_fixed_set_sparse(N_, ncol_, cp_, row_, val_)

    k = int(cp[ncol - 3])                                           # the column of 100 records
    unsorted = row.copy(); unsorted[k], unsorted[k + 1] = row[k + 1], row[k]
    refused(N, ncol, cp, unsorted, val)
    dup = row.copy(); dup[k + 1] = row[k]
    refused(N, ncol, cp, dup, val)
    empty = cp.copy(); empty[5] = empty[6]                          # column 5 without an entry
    refused(N, ncol, empty, row, val)
    refused(N, 1, cp[-2:] - cp[-2], row[cp[-2]:], val[cp[-2]:])     # a single column is a dense set
    refused(N + 1, ncol, cp, row, val)                              # another number of records
    outside = row.copy(); outside[-1] = N
    refused(N, ncol, cp, outside, val)
    nonfinite = val.copy(); nonfinite[7] = np.inf
    refused(N, ncol, cp, row, nonfinite)
    shifted = cp.copy(); shifted[0] = 1
    refused(N, ncol, shifted, row, val)
    assert s.get_fixed()["b"].shape == (0,)
    for f in range(16):
        assert s.add_fixed_set_sparse(N, ncol, cp, row, val) == f
    with pytest.raises(ngp.NextGPHipError, match="at most 16"):     # a 17th set
        s.add_fixed_set_sparse(N, ncol, cp, row, val)
    with pytest.raises(ngp.NextGPHipError, match="at most 16"):     # ... of either kind
        s.add_fixed_set(np.linspace(-1, 1, N))
    add_sets(s, [(0, P, "PR")], v)
    s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var()); s.run(2)
    fx = s.get_fixed()["b"]
    assert fx.shape == (16 * ncol,) and np.all(np.isfinite(fx)) and np.abs(fx[15 * ncol:]).max() > 0


def test_runLMEM_with_150_herds(ngp, O, problem, tmp_path):
    from nextgp_jl_amd import api
    X, y, v = problem
    rng = np.random.default_rng(5)
    code = factor(150, 9)
    names = np.array([f"h{k:03d}" for k in range(150)])
    herd = names[code + 1]                                           # (h000 is the base level)
    eff = rng.normal(size=150) * 2.0 * np.sqrt(y.var())
    yy = y + eff[code + 1]
    geno = str(tmp_path / "geno.npy")
    np.save(geno, X.astype(np.float64))
    out = str(tmp_path / "wide")
    res = api.runLMEM(f'y ~ 1 + herd + SNP(M, "{geno}")', dict(y=yy, herd=herd), 40, 10, 2, outFolder=out, VCV={"M": api.BayesPR(9999, v)},
                      diagnostics=True)
    assert res["fixed_names"] == ["(Intercept)"] + [f"herd: {h}" for h in names[1:]] and len(res["fixed"]) == 149
    with open(os.path.join(out, "bOut")) as f:
        assert f.readline().rstrip("\n").split("\t") == res["fixed_names"]
    bm = api.summaryMCMC("b", outFolder=out)[0]
    assert len(bm) == 150 and np.allclose(bm[1:], res["fixed"], rtol=1e-12, atol=1e-12)
    big = np.bincount(code + 1, minlength=150) >= 10                  # levels with records enough to be estimated, against the base level
    assert np.corrcoef(res["fixed"][big[1:]], (eff - eff[0])[1:][big[1:]])[0, 1] > 0.9
    dn = res["diagnostics"]["names"]
    assert [n for n in dn if n.startswith("b:herd")] == [f"b:herd: {h}" for h in names[1:]]
    # a factor of 12 levels: the same files whichever way the set goes
    code12 = factor(12, 10)
    herd12 = names[code12 + 1]
    outs = []
    for tag, kw in (("auto", {}), ("sparse", dict(sparseFixed=True))):
        o = str(tmp_path / tag)
        r = api.runLMEM(f'y ~ 1 + herd + SNP(M, "{geno}")', dict(y=yy, herd=herd12), 20, 4, 2, outFolder=o, VCV={"M": api.BayesPR(9999, v)}, **kw)
        outs.append((o, r))
    (oa, ra), (ob, rb) = outs
    assert sorted(os.listdir(oa)) == sorted(os.listdir(ob)) and "bOut" in os.listdir(oa)
    for f in os.listdir(oa):
        assert open(os.path.join(oa, f), "rb").read() == open(os.path.join(ob, f), "rb").read(), f
    assert np.array_equal(ra["fixed"], rb["fixed"]) and len(ra["fixed"]) == 11
