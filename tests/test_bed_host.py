"""PLINK .bed filesets on the host (no GPU): write_plink -> read_plink -> decode_bed against a per-genotype loop written here, the
refusals that come before any device work, and the static side of the two new entry points (header, SYMBOLS, Julia shim)."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FILE, P = 341, 7   # 341 mod 4 = 1: three pad genotypes in every column's last byte
NEW = ["ngp_panel_columns_bed", "ngp_prediction_columns_bed"]


def fileset(ngp, tmp_path, name="g", miss_share=0.05):
    rng = np.random.default_rng(5)
    G = rng.integers(0, 3, size=(N_FILE, P)).astype(np.uint8)
    miss = rng.random((N_FILE, P)) < miss_share
    miss[:, 2] = False            # a column without a missing call
    miss[:, 4] = True             # a column without an observed call
    bed = ngp.write_plink(tmp_path / name, G, missing=miss, iid=[f"a{i}" for i in range(N_FILE)], chr=[1, 1, 1, 2, 2, 3, 3])
    raw = bytearray(open(bed, "rb").read())
    nb = (N_FILE + 3) // 4
    for j in range(P):            # the pad bits of every column's last byte hold the missing code: they are no genotypes
        raw[3 + j * nb + nb - 1] |= 0b01010100
    open(bed, "wb").write(bytes(raw))
    return bed, G, miss


def loop_decode(raw, n_file, rows, cols, allele, policy):
    """One genotype per iteration, straight from the file's bytes (behind the magic): the matrix decode_bed has to give."""
    nb = (n_file + 3) // 4
    out = np.zeros((len(rows), len(cols)))
    cnt = np.zeros((len(cols), 4), dtype=np.int64)
    for jj, j in enumerate(cols):
        vals = []
        for i in rows:
            two = (raw[3 + j * nb + i // 4] >> (2 * (i % 4))) & 3
            a1 = {0: 2, 1: None, 2: 1, 3: 0}[two]
            vals.append(None if a1 is None else (a1 if allele == 1 else 2 - a1))
        obs = [v for v in vals if v is not None]
        for v in vals:
            cnt[jj, 3 if v is None else v] += 1
        total, n_obs = sum(obs), len(obs)
        if policy == "mean":
            fill = total / n_obs if n_obs else 0.0
        else:
            fill = (2 * total + n_obs) // (2 * n_obs) if n_obs else 0
        out[:, jj] = [fill if v is None else v for v in vals]
    return out, cnt


@pytest.mark.parametrize("allele", [1, 2])
def test_round_trip_against_a_per_genotype_loop(ngp, tmp_path, allele):
    bed, G, miss = fileset(ngp, tmp_path)
    info = ngp.read_plink(bed)
    assert ngp.is_bed_file(bed) and (info["n"], info["P"]) == (N_FILE, P) and info["bed"].shape == (P, 86)
    assert info["iid"][:2] == ["a0", "a1"] and info["fid"][3] == "a3" and info["snp"][6] == "snp7" and info["chr"] == list("1112233")
    assert info["a1"] == ["A"] * P and info["a2"] == ["B"] * P and info["pos"] == list(range(1, P + 1))
    assert ngp.read_plink(bed[:-4])["n"] == N_FILE                      # the prefix names the same fileset
    raw = open(bed, "rb").read()
    rng = np.random.default_rng(2)
    perm = rng.permutation(N_FILE)[:200]
    perm[17] = perm[3]                                                  # one animal with two records
    for rows, cols in ((None, None), (perm, None), (perm, [5, 0, 2])):
        r = list(range(N_FILE)) if rows is None else [int(i) for i in rows]
        c = list(range(P)) if cols is None else cols
        for policy in ("mean", "round"):
            want, wcnt = loop_decode(raw, N_FILE, r, c, allele, policy)
            got, cnt = ngp.decode_bed(info["bed"], N_FILE, rows=rows, cols=cols, allele=allele, missing=policy, counts=True)
            assert got.dtype == (np.float64 if policy == "mean" else np.uint8) and got.shape == want.shape
            assert np.array_equal(got.astype(np.float64), want) and np.array_equal(cnt, wcnt)
    # what was written comes back where it was observed, and the all-missing column is a zero column
    full = ngp.decode_bed(info["bed"], N_FILE, allele=1, missing="round")
    assert np.array_equal(full[~miss], G[~miss]) and not full[:, 4].any()
    # "error": refused where a selected row is missing, uint8 codes where none is
    with pytest.raises(ValueError, match=r"column 1 holds 341 missing calls"):   # (counted within cols=)
        ngp.decode_bed(info["bed"], N_FILE, cols=[2, 4], missing="error")
    clean = ngp.decode_bed(info["bed"], N_FILE, cols=[2], allele=allele, missing="error")
    assert clean.dtype == np.uint8 and np.array_equal(clean[:, 0], G[:, 2] if allele == 1 else 2 - G[:, 2])
    # read_genotypes on the path: the host matrix, file order, missing calls at the column mean
    assert np.array_equal(ngp.read_genotypes(bed), ngp.decode_bed(info["bed"], N_FILE, missing="mean"))


def test_refusals_before_any_device_work(ngp, tmp_path):
    bed, G, miss = fileset(ngp, tmp_path)
    raw = open(bed, "rb").read()
    sm = tmp_path / "sm.bed"
    sm.write_bytes(b"\x6c\x1b\x00" + raw[3:])
    with pytest.raises(ValueError, match="sample-major"):
        ngp.is_bed_file(sm)
    assert not ngp.is_bed_file(tmp_path / "g.bim") and not ngp.is_bed_file(tmp_path / "absent.bed")
    for ext in (".bim", ".fam"):
        (tmp_path / ("cut" + ext)).write_bytes((tmp_path / ("g" + ext)).read_bytes())
    (tmp_path / "cut.bed").write_bytes(raw[:-1])
    with pytest.raises(ValueError, match=r"cut\.bed holds 604 bytes.*3 \+ 7 x 86 = 605"):
        ngp.read_plink(tmp_path / "cut.bed")
    (tmp_path / "nofam.bed").write_bytes(raw)
    (tmp_path / "nofam.bim").write_bytes((tmp_path / "g.bim").read_bytes())
    with pytest.raises(ValueError, match=r"nofam\.fam is absent"):
        ngp.read_plink(tmp_path / "nofam")
    with pytest.raises(ValueError, match="rows outside"):
        ngp.decode_bed(ngp.read_plink(bed)["bed"], N_FILE, rows=[0, N_FILE])
    # runLMEM: both refusals are raised on the host, in front of the handle
    rng = np.random.default_rng(1)
    data = {"y": rng.normal(size=30), "id": [f"a{i}" for i in range(29)] + ["zz9"]}
    kw = dict(VCV={"M1": ngp.BayesPR(9999, 0.01), "e": ngp.Random("I", 1.0)}, outFolder=str(tmp_path / "out"), overwrite=True)
    with pytest.raises(ValueError, match=r"genoID: 'zz9' \(record 30\) is not an IID of .*g\.fam"):
        ngp.runLMEM(f'y ~ 1 + SNP(M1, "{bed}")', data, 10, 2, 2, genoID="id", **kw)
    with pytest.raises(ValueError, match='missingGeno="mean" with storage="u8"'):
        ngp.runLMEM(f'y ~ 1 + SNP(M1, "{bed}")', data, 10, 2, 2, genoID="id", storage="u8", missingGeno="mean", **kw)


def test_entry_points_are_declared_listed_and_bound(ngp):
    hdr = open(os.path.join(ROOT, "include", "nextgp_hip.h")).read()
    assert re.search(r"#define\s+NGP_ABI_VERSION\s+4\b", hdr)            # additive: the version stays
    for name, val in (("ERROR", 0), ("MEAN", 1), ("ROUND", 2)):
        assert re.search(rf"#define\s+NGP_BED_MISSING_{name}\s+{val}\b", hdr)
    from test_julia_shim_static import c_declarations, julia_ccalls
    decl = c_declarations()
    sig = ["ngp_handle*", "int64_t", "uint8_t*", "int64_t", "int64_t", "int64_t", "int64_t*", "int32_t", "int32_t", "int32_t", "int64_t*"]
    calls = {c[0]: c for c in julia_ccalls()}
    for s in NEW:
        assert s in ngp.SYMBOLS and decl[s] == sig
        assert calls[s][2] == ["Ptr{Cvoid}", "Int64", "Ptr{UInt8}", "Int64", "Int64", "Int64", "Ptr{Int64}", "Int32", "Int32", "Int32", "Ptr{Int64}"]
        assert len(calls[s][3]) == len(sig)
    jl = open(os.path.join(ROOT, "nextgp.jl_amd", "julia", "NextGPHIP.jl")).read()
    assert "function read_plink(" in jl and "Mmap.mmap(io, Matrix{UInt8}, (nb, P), 3)" in jl
    src = open(os.path.join(ROOT, "nextgp.jl_amd", "csrc", "ngp_api.hip")).read()
    for s in NEW:
        assert re.search(rf"^int32_t {s}\(", src, flags=re.M)
    assert '#include "ngp_bed.h"' in src and '"ngp_bed.h"' in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    for f in ("is_bed_file", "read_plink", "write_plink", "decode_bed"):
        assert callable(getattr(ngp, f))
