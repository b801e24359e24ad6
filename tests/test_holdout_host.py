"""Held-out records, the parts that need no device: the symbols and the stream kind, the dealing of folds, runLMEM's argument checks, the
restatement's own arithmetic, the three layouts of ngp_state.h and the Julia bindings."""
import os
import re

import numpy as np
import pytest

import ref_holdout as RH
from test_julia_shim_static import C2J, c_declarations, julia_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "nextgp.jl_amd", "csrc")
NEW = ["ngp_set_holdout", "ngp_get_holdout", "ngp_set_holdout_state", "ngp_get_holdout_layout"]
# the groups of the three layouts as they stood before hold-out sets existed: a chain without a mask describes exactly these
POSTERIOR = [["SEG_SUM_BETA"], ["SEG_SUM_BETA2"], ["SEG_SUM_DELTA"], ["SEG_SUM_VARBETA"], ["SEG_SUM_PI"], ["SEG_SUM_CLS"], ["SEG_SUM_FIX"],
             ["SEG_SUM_U"], ["SEG_SUM_VARU"], ["SEG_SUM_LV"], ["SEG_SUM_RC"], ["SEG_SUM_VARE"], ["SEG_SUM_B"], ["SEG_NKEPT_F64"]]
SAMPLE = [["SEG_ITER"], ["SEG_VARE"], ["SEG_B"], ["SEG_FIX"], ["SEG_U"], ["SEG_VARU"], ["SEG_BETA"], ["SEG_VARBETA"], ["SEG_PI"], ["SEG_CLS"],
          ["SEG_LV"], ["SEG_RC_PROB"], ["SEG_DELTA"], ["SEG_RC_CAT"]]
SNAPSHOT_BODY = [["SEG_VARE"], ["SEG_B"], ["SEG_SUM_VARE"], ["SEG_SUM_B"], ["SEG_YCORR"], ["SEG_BETA"], ["SEG_DELTA"], ["SEG_VARBETA"], ["SEG_PI"],
                 ["SEG_SUM_BETA"], ["SEG_SUM_BETA2"], ["SEG_SUM_DELTA"], ["SEG_SUM_VARBETA"], ["SEG_SUM_PI"], ["SEG_FINE"], ["SEG_NFIX"], ["SEG_FIX"],
                 ["SEG_SUM_FIX"], ["SEG_CLS", "SEG_SUM_CLS"], ["SEG_U", "SEG_SUM_U", "SEG_VU", "SEG_RFINE"], ["SEG_LV_ALL", "SEG_ZETA"],
                 ["SEG_RC_PROB", "SEG_SUM_RC", "SEG_RC_CAT"]]
HOLDOUT_SEGS = {"SEG_YAUG", "SEG_SUM_FIT", "SEG_SUM_FIT2", "SEG_N_FIT"}


def layout(name):
    txt = open(os.path.join(CSRC, "ngp_state.h")).read()
    m = re.search(r"inline const Layout " + name + r" = \{(.*?)\};", txt, flags=re.S)
    assert m, name
    return [re.findall(r"SEG_[A-Z0-9_]+", g) for g in re.findall(r"\{([^{}]*)\}", m.group(1))]


def test_symbols_stream_kind_and_abi_version(ngp):
    hdr = open(os.path.join(ROOT, "include", "nextgp_hip.h")).read()
    assert "#define NGP_ABI_VERSION 4" in hdr                       # additive: the version stays
    decl = c_declarations()
    for s in NEW:
        assert s in ngp.SYMBOLS and s in decl, s
    assert decl["ngp_set_holdout"] == ["ngp_handle*", "int64_t*", "int64_t"]
    assert decl["ngp_get_holdout"] == ["ngp_handle*", "int64_t*", "double*", "double*", "double*", "double*", "int64_t", "int64_t"]
    assert decl["ngp_set_holdout_state"] == ["ngp_handle*", "double*", "double*", "double*", "double*", "int64_t", "int64_t"]
    assert decl["ngp_get_holdout_layout"] == ["ngp_handle*", "int64_t*"]
    src = open(os.path.join(CSRC, "ngp_api.hip")).read()
    for s in NEW:                                                   # every entry point behind the exception barrier
        assert re.search(r"\nint32_t " + s + r"\([^)]*\) \{\n    NGP_TRY\n", src), s
    assert re.search(r"^#define NGP_KIND_AUGMENT 21\b", open(os.path.join(CSRC, "ngp_rng.h")).read(), flags=re.M)
    assert RH.KIND_AUGMENT == 21
    k = open(os.path.join(CSRC, "ngp_holdout.h")).read()
    assert "k_holdout_augment" in k and "k_holdout_accum" in k and "NGP_KIND_AUGMENT" in k
    code = re.sub(r"//[^\n]*", "", k)
    assert "atomic" not in code and "__shared__" not in code and "asm" not in code     # plain loads and stores only
    for unit in ("ngp_sweep.h", "ngp_sweep_inst.hip", "ngp_sweep_body.inc", "ngp_sweep_multi_body.inc"):   # the sweep units do not know it
        assert "holdout" not in open(os.path.join(CSRC, unit)).read()


def test_folds_are_dealt_deterministically_and_cover_every_observed_record_once(ngp):
    rng = np.random.default_rng(5)
    y = rng.normal(size=53)
    y[[0, 17, 52]] = np.nan
    f1, f2 = ngp.deal_folds(y, 5, foldSeed=3), ngp.deal_folds(y, 5, foldSeed=3)
    assert np.array_equal(f1, f2) and f1.dtype == np.int64
    assert np.all(f1[[0, 17, 52]] == -1) and np.all(f1[~np.isnan(y)] >= 0) and f1.max() == 4
    obs = np.flatnonzero(~np.isnan(y))
    order = obs[np.random.default_rng(3).permutation(len(obs))]                 # the permutation, dealt round-robin
    assert np.array_equal(f1[order], np.arange(len(obs)) % 5)
    assert sorted(np.bincount(f1[obs]).tolist()) == [10, 10, 10, 10, 10]
    assert sorted(np.concatenate([np.flatnonzero(f1 == c) for c in range(5)]).tolist()) == obs.tolist()   # every observed record exactly once
    assert not np.array_equal(f1, ngp.deal_folds(y, 5, foldSeed=4))
    for bad in (1, 51):
        with pytest.raises(ValueError, match="folds"):
            ngp.deal_folds(y, bad)


def test_runlmem_holdout_arguments_are_checked_before_any_device_work(ngp, tmp_path):
    """Every keyword clash and every bad row list is a ValueError from host checks -- this test runs where there is no device."""
    rng = np.random.default_rng(3)
    N = 30
    A = rng.integers(0, 3, size=(N, 20)).astype(np.uint8)
    np.save(tmp_path / "a.npy", A)
    f = f'y ~ 1 + SNP(M1,"{tmp_path / "a.npy"}")'
    data = {"y": rng.normal(size=N)}
    k = [0]

    def run(**kw):
        k[0] += 1
        return ngp.runLMEM(f, data, 4, 2, 1, outFolder=str(tmp_path / f"o{k[0]}"), **kw)

    with pytest.raises(ValueError, match="chains"):
        run(folds=3, chains=2)
    with pytest.raises(ValueError, match="holdout"):
        run(folds=3, holdout=[1, 2])
    for bad in (1, 9, 2.5):
        with pytest.raises(ValueError, match="folds"):
            run(folds=bad)
    with pytest.raises(ValueError, match="missing"):
        run(missing="skip")
    with pytest.raises(ValueError, match="twice"):
        run(holdout=[3, 3])
    with pytest.raises(ValueError, match="numbered"):
        run(holdout=[0, N])
    with pytest.raises(ValueError, match="numbered"):
        run(holdout=[-1])
    with pytest.raises(ValueError, match="record numbers"):
        run(holdout=[0.5])
    with pytest.raises(ValueError, match="record numbers"):
        run(holdout=[])
    with pytest.raises(ValueError, match="keep its response"):
        run(holdout=list(range(N)))


def test_holdout_summary(ngp):
    rng = np.random.default_rng(2)
    fit = rng.normal(size=(6, 4))
    N, H = 9, np.array([0, 3, 4, 8])
    s1 = np.zeros(N); s2 = np.zeros(N); nf = np.zeros(N)
    for d in fit:
        got = RH.accumulate(s1, s2, nf, H, d + 1.0, np.ones(4))
        assert np.array_equal(got, (d + 1.0) - 1.0)
    hs = ngp.holdout_summary(dict(sum_fit=s1, sum_fit2=s2, n_fit=nf))
    assert np.array_equal(hs["rows"], H) and np.array_equal(hs["n"], [6] * 4)
    m = s1[H] / 6
    assert np.array_equal(hs["mean"], m) and np.array_equal(hs["sd"], np.sqrt(np.maximum(0.0, s2[H] / 6 - m * m)))
    assert np.all(s1[[1, 2, 5, 6, 7]] == 0) and np.all(nf[[1, 2, 5, 6, 7]] == 0)
    with pytest.raises(ValueError):
        ngp.holdout_summary(dict(sum_fit=np.zeros(3), sum_fit2=np.zeros(3), n_fit=np.zeros(3)))


def test_restatement_start_and_step():
    y = np.array([1.0, np.nan, 0.1, 0.2, 1e6, 0.3])
    H = [1, 4]
    yb = ((1.0 + 0.1) + 0.2) + 0.3
    assert RH.ybar_obs(y, H) == yb / 4.0
    y0, ya = RH.start(y, H)
    assert np.array_equal(y0, [1.0, yb / 4.0, 0.1, 0.2, yb / 4.0, 0.3]) and np.array_equal(ya, [yb / 4.0] * 2)
    same, e, ep = RH.step(ya, y0[H], 0.0, [0.5, -0.5])                          # varE == 0: the start survives
    assert np.array_equal(same, ya) and e is None and ep is None
    ya1, e, ep = RH.step(ya, np.array([0.25, -0.5]), 4.0, [0.5, -1.5])
    assert np.array_equal(e, [1.0, -3.0]) and ep is e and np.array_equal(ya1, [(yb / 4.0 - 0.25) + 1.0, (yb / 4.0 + 0.5) - 3.0])
    ya2, e, ep = RH.step(ya, np.array([0.25, -0.5]), 4.0, [0.5, -1.5], s_H=[2.0, 0.5])
    assert np.array_equal(e, [1.0, -3.0]) and np.array_equal(ep, [0.5, -6.0]) and np.array_equal(ya2, [(yb / 4.0 - 0.25) + 0.5, (yb / 4.0 + 0.5) - 6.0])


def test_layouts_without_a_mask_are_todays_and_the_new_groups_come_last():
    post, snap = layout("posterior_layout"), layout("snapshot_body_layout")
    assert post == POSTERIOR + [["SEG_SUM_FIT"], ["SEG_SUM_FIT2"], ["SEG_N_FIT"]]
    assert snap == SNAPSHOT_BODY + [["SEG_YAUG", "SEG_SUM_FIT", "SEG_SUM_FIT2", "SEG_N_FIT"]]
    assert layout("sample_layout") == SAMPLE                                     # the sample file is unchanged
    assert layout("snapshot_head_layout") == [["SEG_ITER"], ["SEG_NKEPT"], ["SEG_SEED"], ["SEG_CHAIN"]]
    # a chain without a mask describes none of the new segments, so place() skips their groups: they are described in one place only,
    # under the mask's condition
    api = open(os.path.join(CSRC, "ngp_api.hip")).read()
    body = api[api.index("void describe(ngp_handle *h, ChainState &st) {"):api.index("static_assert(offsetof(DSet, piHat1)")]
    guard = body.index("if (!h->cm.ho_rows.empty()) {")
    for seg in HOLDOUT_SEGS:
        assert body.count(seg + ",") == 1 and body.index(seg + ",") > guard, seg
    assert api.count("SEG_YAUG") == 1
    # the ids were appended to the enum: every earlier id keeps its value
    txt = open(os.path.join(CSRC, "ngp_state.h")).read()
    enum = re.findall(r"SEG_[A-Z0-9_]+", re.sub(r"//[^\n]*", "", txt[txt.index("enum SegId"):txt.index("struct Seg {")]))
    assert enum[-4:] == ["SEG_YAUG", "SEG_SUM_FIT", "SEG_SUM_FIT2", "SEG_N_FIT"] and enum[-5] == "SEG_SUM_RC"


def test_julia_binds_the_holdout_entry_points():
    decl = c_declarations()
    calls = {name: (ret, types, vals) for name, ret, types, vals in julia_ccalls()}
    for s in NEW:
        assert s in calls, s
        ret, types, vals = calls[s]
        assert ret == "Int32" and len(types) == len(decl[s]) == len(vals)
        assert all(jt in C2J[ct] for jt, ct in zip(types, decl[s])), s
    jl = open(os.path.join(ROOT, "nextgp.jl_amd", "julia", "NextGPHIP.jl")).read()
    assert "holdout::Vector{Int}=Int[]" in jl and "sort(holdout) .- 1" in jl and "holdoutPredict.txt" in jl
    assert jl.index("set_holdout!(h, Vector{Int64}(sort(holdout) .- 1))") < jl.index("set_y!(h, Vector{Float64}(ycorr))")


def test_the_law_bound_holds_for_the_restatement():
    """The closed form behind test_gpu_holdout's law test, on the CPU: intercept only, 16 of 64 records held out; the mean of b and of
    every held-out fitted value over 4,000 kept draws lies within 6 sqrt(v (1 + f) / ((1 - f) n_obs nKept)) of the observed mean."""
    from test_gpu_holdout import LAW
    y, H = LAW["y"](), LAW["H"]
    mb, mfit, mv = RH.simulate_intercept_only(y, H, LAW["burn"], LAW["kept"], 4.0, LAW["e_scale"], seed=LAW["seed"])
    tol = RH.law_bound(mv, len(H) / len(y), len(y) - len(H), LAW["kept"])
    yb = RH.ybar_obs(y, H)
    assert abs(mb - yb) <= tol and np.all(np.abs(mfit - yb) <= tol)
    assert tol < 0.05 * np.sqrt(mv)                                              # (the bound is a tight one: a 20th of the residual SD)
