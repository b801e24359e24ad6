"""PLINK .bed columns decoded on the device (include/nextgp_hip.h: ngp_panel_columns_bed, ngp_prediction_columns_bed; csrc/ngp_bed.h).

The packed columns go up as they are in the file, in the three out-of-order calls of tests/test_gpu_ingest.py and about 40 columns per
staging chunk, and the stored panel is read back as there: ngp_xbeta(e_j) column by column, the means, mpm and the Gram blocks.  What
it must equal is a handle loaded through ngp_panel_columns_u8 from codes decoded -- and, under ROUND, imputed -- in this file with
plain numpy, or, under MEAN, float32(g - mu_obs) with zeros at the missing calls.  Every comparison is np.array_equal."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import add_sets

pytestmark = pytest.mark.gpu

N_FILE, N, P = 341, 333, 330                 # five full 64-column blocks and a partial one; both sample counts end mid-byte
CALLS = ((130, 330), (0, 57), (57, 130))     # boundaries inside blocks, out of order
CHUNK = 40                                   # columns per staging chunk: chunks end inside blocks
NP_ = 70
SPEC = [(0, 100, "PR"), (100, 230, "R")]
SCHED = (6, 2, 2)
V0 = 0.01
ALL_MISSING, ONE_MISSING, MONO = 70, 200, 131
STORAGES = {"f32": (None, False), "f32w": (None, True), "u8": ("u8", False)}


def pack(G, miss=None, allele_one=True, stride=0, fill=0x00, pad_bits=True):
    """(P, stride) packed columns of the A1 counts G (n x P): two-bit values 0 = two A1, 1 = missing, 2 = one, 3 = none.  The pad
    bits of the last byte hold the missing code and the bytes up to `stride` are `fill`: neither is a genotype."""
    n, p = G.shape
    code = np.array([3, 2, 0], dtype=np.uint8)[G.astype(np.int64)]
    if miss is not None:
        code = np.where(miss, np.uint8(1), code)
    nb = (n + 3) // 4
    full = np.full((4 * nb, p), 1 if pad_bits else 0, dtype=np.uint8)
    full[:n] = code
    by = (full[0::4] | (full[1::4] << 2) | (full[2::4] << 4) | (full[3::4] << 6)).T
    out = np.full((p, max(stride, nb)), fill, dtype=np.uint8)
    out[:, :nb] = by
    return np.ascontiguousarray(out)


@functools.lru_cache(None)
def data():
    rng = np.random.default_rng(20261)
    G = rng.integers(0, 3, size=(N_FILE, P)).astype(np.uint8)
    G[:, MONO] = 2
    rows = rng.permutation(N_FILE)[:N].astype(np.int64)
    rows[40] = rows[7]                                   # one animal with two records
    miss = rng.random((N_FILE, P)) < 0.03
    miss[:, ALL_MISSING] = True
    miss[:, ONE_MISSING] = False; miss[rows[11], ONE_MISSING] = True
    miss[:, MONO] = False
    w = rng.uniform(0.25, 4.0, size=N)
    bt = np.zeros(P); bt[rng.choice(P, 8, replace=False)] = rng.normal(size=8)
    y = 10.0 + (G[:N] - G[:N].mean(axis=0)) @ bt + rng.normal(size=N)
    Gp = rng.integers(0, 3, size=(NP_ + 10, P)).astype(np.uint8)
    pmiss = rng.random((NP_ + 10, P)) < 0.03
    prow = rng.permutation(NP_ + 10)[:NP_].astype(np.int64)
    d = dict(G=G, rows=rows, miss=miss, w=w, y=y, Gp=Gp, pmiss=pmiss, prow=prow)
    for a in d.values():
        a.setflags(write=False)
    return d


def counts_of(G, miss):
    """(P, 4): the numbers of 0, 1, 2 and missing calls of every column."""
    return np.stack([((G == v) & ~miss).sum(axis=0) for v in range(3)] + [miss.sum(axis=0)], axis=1).astype(np.int64)


def round_imputed(G, miss):
    cnt = counts_of(G, miss)
    total, n_obs = cnt[:, 1] + 2 * cnt[:, 2], cnt[:, 0] + cnt[:, 1] + cnt[:, 2]
    g_round = np.where(n_obs > 0, (2 * total + n_obs) // np.maximum(2 * n_obs, 1), 0).astype(np.uint8)
    return np.asfortranarray(np.where(miss, g_round[None, :], G))


# ---- reading a handle back (as tests/test_gpu_ingest.py does) -------------------------------------------------------------------
def stored_columns(s):
    out = np.empty((s.N, s.P))
    e = np.zeros(s.P)
    for j in range(s.P):
        e[j] = 1.0
        out[:, j] = s.xbeta(e)
        e[j] = 0.0
    return out


def summary(s):
    return dict(means=s.means(), mpm=s.mpm(), gram=np.array([s.gram(t) for t in range((s.P + 63) // 64)]), layout=s.layout())


def assert_same_panel(a, b):
    sa, sb = summary(a), summary(b)
    assert sa["layout"] == sb["layout"]
    for k in ("means", "mpm", "gram"):
        assert np.array_equal(sa[k], sb[k]), k
    assert np.array_equal(stored_columns(a), stored_columns(b))


def new_sampler(ngp, kind):
    storage, weighted = STORAGES[kind]
    s = ngp.Sampler(device=0, seed=1, chain=0, storage=storage)
    if weighted:
        s.set_residual_weights(data()["w"])
    return s


def load_u8(ngp, kind, codes):
    s = new_sampler(ngp, kind)
    s.begin_panel(*codes.shape)
    for a, b in CALLS:
        s.panel_columns(a, np.asfortranarray(codes[:, a:b]), centre=True)
    s.end_panel()
    return s


def load_bed(ngp, kind, packed, n_file, n, rows=None, allele=1, missing="round", short=False):
    """The packed panel in the three calls of CALLS, CHUNK columns per staging chunk; returns the handle and the (P, 4) counts.
    short: by direct C calls from buffers that end ceil(n_file / 4) bytes into their last column."""
    s = new_sampler(ngp, kind)
    stride = packed.shape[1]
    s.debug_set_staging_bytes(CHUNK * stride)
    s.begin_panel(n, P)
    cnt = np.zeros((P, 4), dtype=np.int64)
    r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
    for a, b in CALLS:
        if short:
            flat = np.ascontiguousarray(packed[a:b].reshape(-1)[:(b - a - 1) * stride + (n_file + 3) // 4])
            c = np.zeros((b - a, 4), dtype=np.int64)
            s._chk(s.L.ngp_panel_columns_bed(s.h, C.c_int64(a), flat.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_int64(b - a), C.c_int64(stride),
                                             C.c_int64(n_file), None if r is None else r.ctypes.data_as(C.POINTER(C.c_int64)), C.c_int32(allele),
                                             C.c_int32({"error": 0, "mean": 1, "round": 2}[missing]), C.c_int32(1), c.ctypes.data_as(C.POINTER(C.c_int64))))
            cnt[a:b] = c
        else:
            cnt[a:b] = s.panel_columns_bed(a, packed[a:b], n_file, rows=r, allele=allele, missing=missing, centre=True)
    s.end_panel()
    return s, cnt


# ---- 1. no missing calls, no row map ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "f32w", "u8"])
def test_clean_file_in_file_order_is_the_u8_panel(ngp, kind):
    G = data()["G"][:N]
    none = np.zeros_like(G, dtype=bool)
    for missing in ("error", "round") + (("mean",) if kind != "u8" else ()):
        s, cnt = load_bed(ngp, kind, pack(G), N, N, missing=missing)
        assert_same_panel(s, load_u8(ngp, kind, G))
        assert np.array_equal(cnt, counts_of(G, none))


@pytest.mark.parametrize("kind", ["f32", "u8"])
def test_allele_two_counts_the_other_allele(ngp, kind):
    G = data()["G"][:N]
    s, cnt = load_bed(ngp, kind, pack(G), N, N, allele=2, missing="error")
    assert_same_panel(s, load_u8(ngp, kind, np.asfortranarray(2 - G)))
    assert np.array_equal(cnt, counts_of(2 - G, np.zeros_like(G, dtype=bool)))


# ---- 2. a row map ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "f32w", "u8"])
def test_row_map_gathers_the_records(ngp, kind):
    d = data()
    s, cnt = load_bed(ngp, kind, pack(d["G"]), N_FILE, N, rows=d["rows"], missing="error")
    sel = np.asfortranarray(d["G"][d["rows"]])
    assert_same_panel(s, load_u8(ngp, kind, sel))
    assert np.array_equal(cnt, counts_of(sel, np.zeros_like(sel, dtype=bool)))


# ---- 3. missing calls --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "f32w", "u8"])
def test_round_is_the_u8_panel_of_the_imputed_codes(ngp, kind):
    d = data()
    sel, msel = d["G"][d["rows"]], d["miss"][d["rows"]]
    s, cnt = load_bed(ngp, kind, pack(d["G"], d["miss"]), N_FILE, N, rows=d["rows"], missing="round")
    imp = round_imputed(sel, msel)
    assert not imp[:, ALL_MISSING].any() and msel[:, ONE_MISSING].sum() == 1 and (imp[:, MONO] == 2).all()
    assert_same_panel(s, load_u8(ngp, kind, imp))
    assert np.array_equal(cnt, counts_of(sel, msel))


def mean_reference(sel, msel, w=None):
    cnt = counts_of(sel, msel)
    total, n_obs = cnt[:, 1] + 2 * cnt[:, 2], cnt[:, 0] + cnt[:, 1] + cnt[:, 2]
    mu = np.where(n_obs > 0, total.astype(np.float64) / np.maximum(n_obs, 1).astype(np.float64), 0.0)
    D = np.where(msel, 0.0, sel.astype(np.float64) - mu[None, :])
    if w is None:
        return mu, D.astype(np.float32).astype(np.float64)
    sc = np.sqrt(w)[:, None]
    return mu, (sc * D).astype(np.float32).astype(np.float64) / sc


@pytest.mark.parametrize("kind", ["f32", "f32w"])
def test_mean_fills_in_a_centred_zero(ngp, kind):
    d = data()
    sel, msel = d["G"][d["rows"]], d["miss"][d["rows"]]
    s, cnt = load_bed(ngp, kind, pack(d["G"], d["miss"]), N_FILE, N, rows=d["rows"], missing="mean")
    mu, X = mean_reference(sel, msel, d["w"] if kind == "f32w" else None)
    got = stored_columns(s)
    assert np.array_equal(got, X) and np.array_equal(s.means(), mu)
    assert not got[:, ALL_MISSING].any() and mu[ALL_MISSING] == 0.0 and not got[msel].any()
    assert not got[:, MONO].any() and mu[MONO] == 2.0
    assert np.array_equal(cnt, counts_of(sel, msel))


# ---- 4. stride, filler bytes, short buffers, pad bits ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind,missing", [("f32", "mean"), ("f32", "round"), ("u8", "round")])
def test_filler_bytes_and_pad_bits_are_no_genotypes(ngp, kind, missing):
    """A stride of ceil(n_file / 4) + 5 with every filler byte 0x55 (four missing codes), through the wrapper and as short buffers by
    direct C calls: the panel and the counts of the tight file whose pad bits are clear."""
    d = data()
    nb = (N_FILE + 3) // 4
    want, wcnt = load_bed(ngp, kind, pack(d["G"], d["miss"], pad_bits=False), N_FILE, N, rows=d["rows"], missing=missing)
    wide = pack(d["G"], d["miss"], stride=nb + 5, fill=0x55, pad_bits=True)
    assert wide.shape == (P, nb + 5) and (wide[:, nb:] == 0x55).all() and ((wide[:, nb - 1] & 0xFC) == 0x54).all()
    for short in (False, True):
        s, cnt = load_bed(ngp, kind, wide, N_FILE, N, rows=d["rows"], missing=missing, short=short)
        assert_same_panel(s, want)
        assert np.array_equal(cnt, wcnt) and np.array_equal(cnt, counts_of(d["G"][d["rows"]], d["miss"][d["rows"]]))


# ---- 5. refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_come_from_the_host_checks(ngp):
    d = data()
    packed = pack(d["G"])
    s = new_sampler(ngp, "f32")
    s.begin_panel(N, P)
    for bad, at in ((N_FILE, 5), (-1, 300)):            # checked on the host: no index outside the file reaches a kernel
        rows = d["rows"].copy(); rows[at] = bad
        with pytest.raises(ngp.NextGPHipError, match=rf"error -1: \.bed row map: rows\[{at}\] = {bad} is outside the file's 341 samples"):
            s.panel_columns_bed(0, packed, N_FILE, rows=rows)
    with pytest.raises(ngp.NextGPHipError, match=r"error -1: \.bed columns without a row map: the file holds 341 samples, the panel 333 rows"):
        s.panel_columns_bed(0, packed, N_FILE)
    with pytest.raises(ngp.NextGPHipError, match=r"error -1: \.bed columns: stride 85 is smaller than ceil\(n_file / 4\) = 86"):
        s.panel_columns_bed(0, packed[:, :85].copy(), N_FILE, rows=d["rows"])
    with pytest.raises(ngp.NextGPHipError, match="error -1: column range outside the panel"):
        s.panel_columns_bed(1, packed, N_FILE, rows=d["rows"])
    with pytest.raises(ngp.NextGPHipError, match=r"error -1: \.bed columns: allele must be 1"):
        s.panel_columns_bed(0, packed, N_FILE, rows=d["rows"], allele=3)
    r = d["rows"].copy()
    for pol, msg in ((7, "unknown missing-call policy 7"),):
        rc = s.L.ngp_panel_columns_bed(s.h, C.c_int64(0), packed.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_int64(P), C.c_int64(packed.shape[1]), C.c_int64(N_FILE),
                                       r.ctypes.data_as(C.POINTER(C.c_int64)), C.c_int32(1), C.c_int32(pol), C.c_int32(1), None)
        assert rc == -1 and msg in s.L.ngp_last_error(s.h).decode()
    rc = s.L.ngp_panel_columns_bed(s.h, C.c_int64(0), None, C.c_int64(P), C.c_int64(packed.shape[1]), C.c_int64(N_FILE),
                                   r.ctypes.data_as(C.POINTER(C.c_int64)), C.c_int32(1), C.c_int32(2), C.c_int32(1), None)
    assert rc == -1 and "null pointer to the packed .bed columns" in s.L.ngp_last_error(s.h).decode()
    # MEAN under byte tiles: refused whether or not a call is missing
    s8 = new_sampler(ngp, "u8")
    s8.begin_panel(N, P)
    with pytest.raises(ngp.NextGPHipError, match="error -1: .*NGP_BED_MISSING_MEAN needs fp32 storage"):
        s8.panel_columns_bed(0, packed, N_FILE, rows=d["rows"], missing="mean")


def test_error_policy_names_the_column_and_leaves_the_handle_usable(ngp):
    d = data()
    sel = np.asfortranarray(d["G"][d["rows"]])
    miss = np.zeros((N_FILE, P), dtype=bool)
    miss[d["rows"][3], 57] = True; miss[d["rows"][40], 57] = True      # (rows[40] == rows[7]: an animal with two records counts twice)
    miss[d["rows"][7], 57] = True
    bad, good = pack(d["G"], miss), pack(d["G"])
    s = new_sampler(ngp, "f32")
    s.debug_set_staging_bytes(CHUNK * bad.shape[1])
    s.begin_panel(N, P)
    with pytest.raises(ngp.NextGPHipError, match=r"error -1: column 57 holds 3 missing calls"):   # columns 50 .. 89: the call's second chunk
        s.panel_columns_bed(10, bad[10:130], N_FILE, rows=d["rows"], missing="error")
    s.begin_panel(N, P)
    for a, b in CALLS:
        s.panel_columns_bed(a, good[a:b], N_FILE, rows=d["rows"], missing="error")
    s.end_panel()
    assert_same_panel(s, load_u8(ngp, "f32", sel))


# ---- 6. prediction -----------------------------------------------------------------------------------------------------------------
def run_prediction(ngp, s):
    y = data()["y"]
    add_sets(s, SPEC, V0)
    s.set_y(y); s.set_residual_prior(4.0, 0.25 * y.var()); s.set_schedule(*SCHED)
    s.run(6)
    return s.prediction_sums()


@pytest.mark.parametrize("kind,missing", [("f32", "mean"), ("f32", "round"), ("u8", "round")])
def test_prediction_panel_from_a_second_bed(ngp, kind, missing):
    """70 candidates gathered from a file of 80 with missing calls: the prediction sums are those of a twin whose candidates came
    through ngp_prediction_columns_f64 with the training mean at the missing calls (MEAN) or through ngp_prediction_columns_u8 with the
    training mean rounded to a code (ROUND)."""
    d = data()
    train = np.asfortranarray(d["G"][:N])
    psel, pmsel = d["Gp"][d["prow"]], d["pmiss"][d["prow"]]
    packed = pack(d["Gp"], d["pmiss"])
    sums = []
    for twin in (False, True):
        s = new_sampler(ngp, kind)
        s.set_panel(train, centre=True)
        mean = s.means()
        s.begin_prediction_panel(NP_)
        if not twin:
            s.debug_set_staging_bytes(CHUNK * packed.shape[1])
            cnt = np.zeros((P, 4), dtype=np.int64)
            for a, b in CALLS:
                cnt[a:b] = s.prediction_columns_bed(a, packed[a:b], NP_ + 10, rows=d["prow"], missing=missing, centre=True)
            assert np.array_equal(cnt, counts_of(psel, pmsel))                    # over the prediction rows
        elif missing == "mean":
            s.prediction_columns(0, np.asfortranarray(np.where(pmsel, mean[None, :], psel.astype(np.float64))), centre=True)
        else:
            code = np.clip(np.floor(mean + 0.5), 0, 2).astype(np.uint8)
            s.prediction_columns(0, np.asfortranarray(np.where(pmsel, code[None, :], psel)), centre=True)
        s.end_prediction_panel()
        sums.append(run_prediction(ngp, s))
    assert sums[0]["nKept"] == sums[1]["nKept"] == 2 and np.abs(sums[0]["sum"]).max() > 0
    assert np.array_equal(sums[0]["sum"], sums[1]["sum"]) and np.array_equal(sums[0]["sum2"], sums[1]["sum2"])


def test_prediction_mean_needs_centring(ngp):
    d = data()
    s = new_sampler(ngp, "f32")
    s.set_panel(np.asfortranarray(d["G"][:N]), centre=True)
    s.begin_prediction_panel(NP_)
    with pytest.raises(ngp.NextGPHipError, match="error -1: .*NGP_BED_MISSING_MEAN writes the training mean, which needs centre != 0"):
        s.prediction_columns_bed(0, pack(d["Gp"]), NP_ + 10, rows=d["prow"], missing="mean", centre=False)


# ---- 7. runLMEM end to end ---------------------------------------------------------------------------------------------------------
def test_runlmem_from_a_fileset(ngp, tmp_path):
    """40 samples in the fileset, 32 records matched through genoID in shuffled order, 130 SNPs on two chromosomes.  Under "round" the
    posterior means are those of the same records from an .npy of the imputed codes; the counts, the map and the windows come from
    the fileset."""
    rng = np.random.default_rng(77)
    nf, nr, p = 40, 32, 130
    G = rng.integers(0, 3, size=(nf, p)).astype(np.uint8)
    miss = rng.random((nf, p)) < 0.03
    iid = [f"an{i:03d}" for i in range(nf)]
    rows = rng.permutation(nf)[:nr]
    bed = ngp.write_plink(tmp_path / "geno", G, iid=iid, missing=miss, chr=[1] * 70 + [2] * 60)
    sel, msel = G[rows], miss[rows]
    imp = round_imputed(sel, msel)
    np.save(tmp_path / "imp.npy", imp)
    bt = np.zeros(p); bt[[5, 60, 100]] = (1.0, -1.0, 0.5)
    y = 3.0 + (imp - imp.mean(axis=0)) @ bt + rng.normal(size=nr)
    userData = {"y": y, "animal": [iid[i] for i in rows]}
    VCV = {"M1": ngp.BayesC(0.3, 0.05, estimatePi=True), "e": ngp.Random("I", 0.5 * y.var())}
    a = ngp.runLMEM(f'y ~ 1 + SNP(M1,"{bed}")', userData, 12, 4, 2, outFolder=str(tmp_path / "bed"), VCV=VCV, seed=5, genoID="animal", missingGeno="round",
                    samples="none")
    b = ngp.runLMEM(f'y ~ 1 + SNP(M1,"{tmp_path / "imp.npy"}")', userData, 12, 4, 2, outFolder=str(tmp_path / "npy"), VCV=VCV, seed=5, samples="none")
    assert a["nKept"] == b["nKept"] == 4 and a["b"] == b["b"] and a["varE"] == b["varE"] and np.abs(a["sets"]["M1"]["beta"]).max() > 0
    for k in ("beta", "delta", "var", "pi"):
        assert np.array_equal(a["sets"]["M1"][k], b["sets"]["M1"][k]), k
    st = a["sets"]["M1"]["snpStats"]
    cnt = counts_of(sel, msel)
    assert np.array_equal(np.stack([st["n0"], st["n1"], st["n2"], st["nMissing"]], axis=1), cnt) and st["snp"][129] == "snp130"
    lines = (tmp_path / "bed" / "snpStatsM1.txt").read_text().splitlines()
    assert lines[0] == "snp a1 a2 n0 n1 n2 nMissing freq" and len(lines) == p + 1
    assert lines[1].split()[:7] == ["snp1", "A", "B"] + [str(int(v)) for v in cnt[0]]
    mp = (tmp_path / "bed" / "map_M1.txt").read_text().splitlines()
    assert mp[0] == "snpID,snpOrder,chrID" and mp[1] == "snp1,1,1" and mp[130] == "snp130,130,2" and len(mp) == p + 1
    w = ngp.runLMEM(f'y ~ 1 + SNP(M1,"{bed}")', userData, 12, 4, 2, outFolder=str(tmp_path / "win"), VCV=VCV, seed=5, genoID="animal", missingGeno="round",
                    samples="none", windows={"M1": 50})
    assert list(w["variance"]["sets"]["M1"]["windows"]["last"]) == [50, 70, 120, 130]      # windows inside the .bim's chromosomes
    assert (tmp_path / "win" / "gwasM1.txt").exists()
