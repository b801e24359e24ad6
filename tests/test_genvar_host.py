"""Genomic variance per kept draw, the parts that need no device: the restatement of the normative arithmetic (tests/ref_genvar.py)
against exact rational variances inside ref_genvar.bound, the segment / item rules, the host summary, the symbol list and the Julia
bindings."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import ref_genvar as RG
from test_julia_shim_static import C2J, c_declarations, julia_ccalls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["ngp_set_variance_windows", "ngp_enable_genomic_variance", "ngp_get_genomic_variance_layout", "ngp_get_genomic_variance",
       "ngp_set_genomic_variance", "ngp_get_genomic_variance_trace", "ngp_get_genomic_variance_stats"]


def test_segments_and_items():
    assert RG.segments(0, 100, []) == [(0, 100, -1)]
    assert RG.segments(100, 92, [(0, 1), (60, 70), (80, 92)]) == [(100, 101, 0), (101, 160, -1), (160, 170, 1), (170, 180, -1), (180, 192, 2)]
    assert RG.segments(0, 5000, []) == [(0, 2048, -1), (2048, 4096, -1), (4096, 5000, -1)]      # a gap is cut, counted from its start
    s = RG.segments(10, 2200, [(50, 2150)])                                                      # a window never is
    assert s == [(10, 60, -1), (60, 2160, 0), (2160, 2210, -1)]
    assert RG.items(s) == [[0], [1], [2]]
    s = RG.segments(0, 4200, [(k * 100, k * 100 + 100) for k in range(42)])
    assert RG.items(s) == [list(range(0, 20)), list(range(20, 40)), [40, 41]]
    assert RG.items(RG.segments(0, 4096, [])) == [[0], [1]]


def test_ilog_and_exponent():
    assert RG.ilog(1.0) == 1 and RG.ilog(0.99) == 0 and RG.ilog(2.0) == 2 and RG.ilog(0.0) == -1022 and RG.ilog(5e-324) == -1022
    assert RG.ilog(float("inf")) == 4000 and RG.ilog(float("nan")) == 4000
    for m in (1e-9, 0.3, 1.0, 1.5, 2.0, 3.9, 255.0):
        assert 2.0 ** RG.xexp(m) > m >= 2.0 ** (RG.xexp(m) - 1)
    assert RG.xmax(np.array([[0.0, 2.0], [1.0, 0.0]]), np.array([0.5, 0.25])) == 1.75 and RG.xmax(np.array([[-3.0, 2.0]])) == 3.0
    assert RG.exponent(3, 0.0) == -400 and RG.exponent(3, 1e300) == 400 and RG.exponent(3, 0.75) == 4


def case(N, P, seed, u8):
    rng = np.random.default_rng(seed)
    G = rng.integers(0, 3, size=(N, P)).astype(np.float64)
    mu = G.mean(axis=0)
    beta = rng.normal(size=P) * rng.choice([0.0, 1e-3, 1.0], size=P)
    if u8:
        X, mean = G, mu
    else:
        X, mean = RG.stored_f32(G, mu), None
    return X, mean, beta


@pytest.mark.parametrize("u8", [False, True], ids=["f32", "u8"])
@pytest.mark.parametrize("N", [2, 5, 40])
def test_restatement_against_rational_variances(N, u8, capsys):
    """V of every slot (windows, sets, total) against var_i of the exact row sums in rational arithmetic, inside ref_genvar.bound; the
    bound is reported relative to V_g.  Two sets that meet inside block 1, a gap, a single-column window, a set without windows."""
    P = 200
    X, mean, beta = case(N, P, 10 * N + u8, u8)
    sets = [(0, 100), (100, 60), (170, 30)]
    windows = [[(0, 1), (60, 70), (90, 100)], [], [(5, 25)]]
    V, E = RG.draw(X, beta, sets, windows, mean)
    cols = [[0], list(range(60, 70)), list(range(90, 100)), list(range(175, 195)), list(range(0, 100)), list(range(100, 160)),
            list(range(170, 200)), list(range(0, 160)) + list(range(170, 200))]
    assert len(V) == len(cols) == 8
    Vg = V[-1]
    assert Vg > 0
    for k, c in enumerate(cols):
        exact = RG.exact_variance(X, beta, c, mean)
        b = RG.bound(X, beta, c, E[k], V[k], mean)
        with capsys.disabled():
            print(f"\n  genvar N={N} {'u8' if u8 else 'f32'} slot {k}: V={V[k]:.6e} |err|={abs(float(Fraction(float(V[k])) - exact)):.3e} bound={b:.3e} "
                  f"bound/V_g={b / Vg:.3e}", end="")
        assert abs(Fraction(float(V[k])) - exact) <= Fraction(float(b))
        assert b <= 2.0 ** -30 * max(Vg, 2.0 ** (2 * E[k] - 2))        # the bound itself: 2^-43 G^2 and change
    # every |g| is inside the range its exponent promises
    gw, gs, a = RG.rows(X, beta, sets, windows, mean)
    for g, e in zip(gw + gs, E):
        assert np.all(np.abs(g) < 2.0 ** (e - 1))


def test_zero_effects_and_sums():
    X, mean, beta = case(7, 80, 3, False)
    V, E = RG.draw(X, np.zeros(80), [(0, 80)], [[(3, 9)]])
    assert np.array_equal(V, np.zeros(3)) and E == [-400] * 3
    S = RG.Sums(3, 0.01, trace_rows=1)
    q, r = S.add(V, 0.0)
    assert not q.any() and r == 0.0 and np.isfinite(S.a).all()
    V2, _ = RG.draw(X, beta, [(0, 80)], [[(3, 9)]])
    q, r = S.add(V2, 0.5)
    assert q[-1] == 1.0 and 0 < r < 1 and S.n == 2 and len(S.trV) == 1 and np.array_equal(S.a[5], V2)
    assert np.array_equal(S.a[4], (V2 / V2[-1] > 0.01).astype(float))


def test_summary_and_names(ngp):
    assert ngp.genomic_variance_names([2, 0]) == ["set0:win_1", "set0:win_2", "set0", "set1", "total"]
    rng = np.random.default_rng(5)
    V = rng.uniform(0.1, 1.0, size=(6, 4)); V[:, 3] = V[:, :3].sum(axis=1)
    q = V / V[:, 3:4]
    r = rng.uniform(0.2, 0.8, size=6)
    gs = dict(sumV=V.sum(0), sumV2=(V * V).sum(0), sumQ=q.sum(0), sumQ2=(q * q).sum(0), count=(q > 0.3).sum(0).astype(float),
              ratio=np.array([r.sum(), (r * r).sum()]), nKept=6)
    out = ngp.genomic_variance_summary(gs, ["a", "b", "c", "total"])
    assert np.allclose(out["meanV"], V.mean(0)) and np.allclose(out["sdV"], V.std(0)) and np.allclose(out["meanQ"], q.mean(0))
    assert np.allclose(out["sdQ"], q.std(0)) and np.array_equal(out["wppa"], (q > 0.3).mean(0)) and out["names"][-1] == "total"
    assert np.isclose(out["ratio"][0], r.mean()) and np.isclose(out["ratio"][1], r.std())
    with pytest.raises(ValueError):
        ngp.genomic_variance_summary(dict(gs, nKept=0))


def test_symbols_header_and_library(ngp):
    hdr = open(os.path.join(ROOT, "include", "nextgp_hip.h")).read()
    assert "#define NGP_ABI_VERSION 4" in hdr                       # additive: the version stays
    decl = c_declarations()
    for s in NEW:
        assert s in ngp.SYMBOLS and s in decl, s
    assert decl["ngp_set_variance_windows"] == ["ngp_handle*", "int32_t", "int64_t*", "int64_t*", "int64_t"]
    assert decl["ngp_enable_genomic_variance"] == ["ngp_handle*", "int32_t", "double", "int64_t"]
    assert decl["ngp_get_genomic_variance"] == ["ngp_handle*"] + ["double*"] * 6 + ["int64_t", "double*", "int64_t*"]
    src = open(os.path.join(ROOT, "nextgp.jl_amd", "csrc", "ngp_api.hip")).read()
    for s in NEW:                                                   # every entry point behind the exception barrier
        assert re.search(r"int32_t " + s + r"\([^)]*\) \{\n    NGP_TRY\n", src), s
    for unit in ("ngp_sweep.h", "ngp_sweep_inst.hip", "ngp_sweep_body.inc", "ngp_sweep_multi_body.inc"):   # the sweep units do not know it
        txt = open(os.path.join(ROOT, "nextgp.jl_amd", "csrc", unit)).read()
        assert "ngp_genvar" not in txt and "k_genvar" not in txt and "GvItem" not in txt


def test_julia_binds_the_genomic_variance_entry_points():
    decl = c_declarations()
    calls = {name: (ret, types, vals) for name, ret, types, vals in julia_ccalls()}
    for s in NEW:
        assert s in calls, s
        ret, types, vals = calls[s]
        assert ret == "Int32" and len(types) == len(decl[s]) == len(vals)
        assert all(jt in C2J[ct] for jt, ct in zip(types, decl[s])), s
    jl = open(os.path.join(ROOT, "nextgp.jl_amd", "julia", "NextGPHIP.jl")).read()
    assert "function getGenomicVariance(h::Handle)" in jl and "function set_variance_windows!(h::Handle" in jl


def test_runlmem_window_arguments_are_checked_before_any_device_work(ngp, tmp_path):
    """Every mistake in windows= / windowThreshold= is a ValueError raised from host checks -- this test runs where there is no
    device, so a check that came after the first device call could not raise what is expected here."""
    rng = np.random.default_rng(3)
    N = 30
    A, B = rng.integers(0, 3, size=(N, 20)).astype(np.uint8), rng.integers(0, 3, size=(N, 12)).astype(np.uint8)
    np.save(tmp_path / "a.npy", A); np.save(tmp_path / "b.npy", B)
    f = f'y ~ 1 + SNP(M1,"{tmp_path / "a.npy"}") + SNP(M2,"{tmp_path / "b.npy"}")'
    data = {"y": rng.normal(size=N)}
    k = [0]

    def run(**kw):
        k[0] += 1
        return ngp.runLMEM(f, data, 4, 2, 1, outFolder=str(tmp_path / f"o{k[0]}"), **kw)

    for bad in ([(5, 5)], [(3, 8), (6, 10)], [(10, 12), (0, 4)], [(15, 21)], [(-1, 3)]):
        with pytest.raises(ValueError, match="ascending, disjoint, non-empty"):
            run(windows={"M1": bad})
    with pytest.raises(ValueError, match="unknown set 'M3'"):
        run(windows={"M1": 5, "M3": 5})
    for thr in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match="windowThreshold"):
            run(windows={"M1": 5}, windowThreshold=thr)
    with pytest.raises(ValueError, match="windowThreshold"):
        run(genomicVariance=True, windowThreshold=2.0)
    with pytest.raises(ValueError, match="mapping"):
        run(windows=[(0, 5)])
    with pytest.raises(ValueError, match="at least one SNP"):
        run(windows={"M1": 0})
    with pytest.raises(ValueError, match="window size or a list"):
        run(windows={"M1": "ten"})
    with pytest.raises(ValueError, match="GBLUP"):
        run(windows={"M2": 4}, VCV={"M2": ngp.Random("G", 1.0)})
    with pytest.raises(NotImplementedError, match="weighted residuals"):
        run(windows={"M1": 5}, VCV={"e": ngp.Random(list(rng.uniform(0.5, 2.0, size=N)), 1.0)})


def test_window_sizes_follow_the_map_file(ngp, tmp_path):
    """An integer window size goes through prep2RegionData where the SNP term has a map: windows never cross a chromosome."""
    from nextgp_jl_amd.api import _variance_windows, parse_formula
    mp = tmp_path / "map.txt"
    mp.write_text("snpID,snpOrder,chrID\n" + "".join(f"s{i},{i + 1},{1 if i < 7 else 2}\n" for i in range(12)))
    np.save(tmp_path / "b.npy", np.zeros((4, 12), dtype=np.uint8))
    snps = parse_formula(f'y ~ 1 + SNP(M2,"{tmp_path / "b.npy"}","{mp}")', random_effects=True, pedigree=True)[2]
    w = _variance_windows({"M2": 3}, 0.01, False, snps, [np.zeros((4, 12))], set(), {})
    assert w == {"M2": [(0, 3), (3, 6), (6, 7), (7, 10), (10, 12)]}
    assert _variance_windows(None, 0.01, False, snps, [np.zeros((4, 12))], set(), {}) is None
    assert _variance_windows(None, 0.01, True, snps, [np.zeros((4, 12))], set(), {}) == {}


def test_output_file_headers(ngp, tmp_path):
    """windowVar<set>Out, genVarOut and gwas<set>.txt: the header row and the rows, in the format summaryMCMC reads."""
    names, wins = ["M1", "M2"], [[(0, 5), (5, 9)], []]
    V = np.arange(10.0).reshape(2, 5) + 0.5          # two draws: 2 windows | 2 sets | total
    r = np.array([0.25, 0.75])
    ngp.write_variance_out_files(str(tmp_path), names, wins, V, r)
    assert (tmp_path / "windowVarM1Out").read_text().splitlines()[0].split("\t") == ["win_1", "win_2"]
    assert not (tmp_path / "windowVarM2Out").exists()
    assert (tmp_path / "genVarOut").read_text().splitlines()[0].split("\t") == ["M1", "M2", "total", "ratio"]
    assert np.array_equal(ngp.summaryMCMC("windowVarM1", str(tmp_path)), [[3.0, 4.0]])
    assert np.array_equal(ngp.summaryMCMC("genVar", str(tmp_path)), [[5.0, 6.0, 7.0, 0.5]])
    from nextgp_jl_amd.api import _variance_result
    q = V / V[:, 4:5]
    gs = dict(sumV=V.sum(0), sumV2=(V * V).sum(0), sumQ=q.sum(0), sumQ2=(q * q).sum(0), count=(q > 0.2).sum(0).astype(float),
              ratio=np.array([r.sum(), (r * r).sum()]), nKept=2)
    var = _variance_result(gs, names, wins, 0.2)
    ngp.write_gwas_files(str(tmp_path), var)
    lines = (tmp_path / "gwasM1.txt").read_text().splitlines()
    assert lines[0].split("\t") == ["window", "firstSNP", "lastSNP", "meanV", "meanQ", "sdQ", "WPPA"] and len(lines) == 3
    assert lines[2].split("\t")[:3] == ["2", "6", "9"] and float(lines[2].split("\t")[3]) == 4.0
    assert not (tmp_path / "gwasM2.txt").exists() and var["sets"]["M2"]["meanV"] == 6.0 and var["total"]["meanV"] == 7.0


def test_julia_coarse_seam_writes_the_same_files():
    jl = open(os.path.join(ROOT, "nextgp.jl_amd", "julia", "NextGPHIP.jl")).read()
    sig = jl[jl.index("function runSampler!("):jl.index("function runSampler!(") + 400]
    assert "windows::Dict=Dict()" in sig and "windowThreshold::Float64=0.01" in sig and "genomicVariance::Bool=false" in sig
    body = jl[jl.index("function write_genomic_variance("):]
    for name in ('"/windowVar$(s)Out"', '"/genVarOut"', '"/gwas$(s).txt"', '"win_$(i)"', '"total", "ratio"'):
        assert name in body, name
    assert "gvar && write_genomic_variance(h, outPut, sets, ids, gvwins)" in jl
