"""ctypes binding of libnextgp_hip.so (include/nextgp_hip.h).

This is the stand-in for the Julia `ccall` shim (julia/NextGPHIP.jl): one thin method per C entry
point, no arithmetic on the Python side.  There is no CPU fallback: if the shared library is
missing, or no gfx950 device is usable, construction raises.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NGP_HIP_LIB") or os.path.join(_HERE, "libnextgp_hip.so")  # override: a library built elsewhere

METHOD_BAYESPR, METHOD_BAYESB, METHOD_BAYESC, METHOD_BAYESR, METHOD_TUPLE, METHOD_BAYESLV, METHOD_BAYESRC = 0, 1, 2, 3, 4, 5, 6
LV_MAXCOV, LV_WORDS = 16, 17  # a BayesLV set in a sample record: c padded to 16 words | varZeta


def _sample_header(f, path):
    """(P, nvb, nsets, nfix, nclass, record bytes, sets, random-effect q per set, (set, ncov) per BayesLV set, thresholds per record) of an
    open sample file, positioned at its first record."""
    magic = f.read(8)
    if magic not in (b"NGPSMP01", b"NGPSMP02", b"NGPSMP03", b"NGPSMP04", b"NGPSMP05"):
        raise NextGPHipError(f"not a sample file: {path}")
    P, nvb, nsets, nfix, ncls, rec = (int(v) for v in np.frombuffer(f.read(48), dtype=np.int64))
    sets = [dict(zip(("method", "K", "col0", "ncol", "nvb", "tk"), np.frombuffer(f.read(48), dtype=np.int64).tolist())) for _ in range(nsets)]
    rq = []
    if magic in (b"NGPSMP02", b"NGPSMP03", b"NGPSMP04", b"NGPSMP05"):  # random-effect sets: int64 nrand | q per set; records hold u and varU behind b_fixed
        nr = int(np.frombuffer(f.read(8), dtype=np.int64)[0])
        rq = np.frombuffer(f.read(8 * nr), dtype=np.int64).tolist()
    lv = []
    if magic in (b"NGPSMP03", b"NGPSMP04", b"NGPSMP05"):  # BayesLV sets: int64 nlv | (marker set, ncov) per set; records hold c[16] | varZeta behind the class probabilities
        nl = int(np.frombuffer(f.read(8), dtype=np.int64)[0])
        lv = [tuple(np.frombuffer(f.read(16), dtype=np.int64).tolist()) for _ in range(nl)]
    if magic in (b"NGPSMP04", b"NGPSMP05"):  # BayesRCpi sets: int64 nrc | (marker set, A, K) per set; records hold annotProb[A][ncol] behind the BayesLV words
        nrc = int(np.frombuffer(f.read(8), dtype=np.int64)[0])  # and annotCat[ncol] (uint8) behind delta.  They ride on the sets' entries.
        for _ in range(nrc):
            si, A, K = np.frombuffer(f.read(24), dtype=np.int64).tolist()
            sets[si].update(rcA=A, rcK=K)
    nthr = 0
    if magic == b"NGPSMP05":  # C >= 3 liability classes: int64 nthr; records end with thr[nthr] (t_2 .. t_{C-1}) directly behind their bytes
        nthr = int(np.frombuffer(f.read(8), dtype=np.int64)[0])
    return P, nvb, nsets, nfix, ncls, rec, sets, rq, lv, nthr


def _rand_qk(w):
    """(q, k) of a random-effect set from its header word: q, and k - 1 of a correlated (Tuple) set in the bits from 32 up."""
    return int(w) & 0xFFFFFFFF, (int(w) >> 32) + 1


def _sample_fields(P, nvb, nsets, nfix, ncls, rq, lv):
    """Where the fields of a sample record lie (the record: csrc/ngp_state.h, sample_layout): (name -> (first double, doubles) in record
    order, doubles of the record in front of the delta bytes).  u<i> / lv<i> are the words of random-effect set i / BayesLV set i."""
    at, o = {}, 0
    for name, n in ([("iter", 1), ("varE", 1), ("b", 1), ("b_fixed", nfix)] + [(f"u{i}", q * k) for i, (q, k) in enumerate(map(_rand_qk, rq))] + [("varU", sum(k * k for _, k in map(_rand_qk, rq))),
                    ("beta", P), ("varBeta", nvb), ("piHat", 2 * nsets), ("class_pi", ncls)] + [(f"lv{i}", LV_WORDS) for i in range(len(lv))]):
        at[name] = (o, n); o += n
    return at, o


def _sample_rc(sets, nd, P):
    """BayesRCpi sets of a sample file: [(marker set, ncol, A, first double of annotProb, first byte of annotCat behind the doubles)],
    and the doubles of a record in front of delta with their annotProb counted in."""
    out, cat = [], P
    for si, s in enumerate(sets):
        if "rcA" in s:
            out.append((si, s["ncol"], s["rcA"], nd, cat))
            nd += s["rcA"] * s["ncol"]; cat += s["ncol"]
    return out, nd


def _sample_record(d, at, rq, lv):
    """The named fields of record doubles d (records along every axis but the last); iter and delta are the caller's."""
    cut = lambda name, n=None: d[..., at[name][0]:at[name][0] + (at[name][1] if n is None else n)]
    out = {k: cut(k) for k in ("b_fixed", "varU", "beta", "varBeta", "piHat", "class_pi")}
    out["varE"], out["b"] = d[..., at["varE"][0]][()], d[..., at["b"][0]][()]  # ([()]: a scalar, not a 0-d array, for a single record)
    out["u"] = [cut(f"u{i}") for i in range(len(rq))]
    out["lv_c"] = [cut(f"lv{i}", ncov) for i, (_, ncov) in enumerate(lv)]  # (c is padded to LV_MAXCOV words, varZeta follows it)
    out["lv_varZeta"] = np.stack([d[..., at[f"lv{i}"][0] + LV_MAXCOV] for i in range(len(lv))], axis=-1) if lv else d[..., 0:0]
    return out


def read_sample_file(path):
    """Binary sample file of ngp_set_sample_file -> dict(iter[n], varE[n], b[n], b_fixed[n, nfix], beta[n, P], varBeta[n, nvb], piHat[n, 2 nsets],
    class_pi[n, nclass], delta[n, P] (uint8), sets=[dict(method, K, col0, ncol, nvb, tk)], u=[[n, q] per random-effect set], varU[n, nrand],
    lv_c=[[n, ncov] per BayesLV set], lv_varZeta[n, nlv]).  A correlated (Tuple) random-effect set of k components has u [n, q k] (the
    components of a level adjacent) and k k words in varU (row-major, in set order)."""
    with open(path, "rb") as f:
        P, nvb, nsets, nfix, ncls, rec, sets, rq, lv, nthr = _sample_header(f, path)
        raw = np.frombuffer(f.read(), dtype=np.uint8)
    n = len(raw) // rec
    raw = raw[:n * rec].reshape(n, rec)
    at, nd0 = _sample_fields(P, nvb, nsets, nfix, ncls, rq, lv)
    rcs, nd = _sample_rc(sets, nd0, P)
    d = raw[:, :nd * 8].copy().view(np.float64)
    out = _sample_record(d, at, rq, lv)
    out.update(iter=raw[:, :8].copy().view(np.int64)[:, 0], sets=sets, delta=raw[:, nd * 8:nd * 8 + P])
    if rcs:  # per BayesRCpi set, keyed by its marker set: annotProb [n, ncol, A], annotCat [n, ncol]
        out["annotProb"] = {si: d[:, o:o + A * nc].reshape(n, A, nc).transpose(0, 2, 1) for si, nc, A, o, _ in rcs}
        out["annotCat"] = {si: raw[:, nd * 8 + c:nd * 8 + c + nc] for si, nc, A, _, c in rcs}
    if nthr:  # the thresholds t_2 .. t_{C-1} of every draw [n, nthr]
        to = nd * 8 + P + sum(nc for _, nc, _, _, _ in rcs)
        out["thr"] = raw[:, to:to + 8 * nthr].copy().view(np.float64)
    return out


def iter_sample_file(path):
    """The records of a sample file ONE AT A TIME (a record of a 600k-SNP model is 5 MB; a whole file of 1000 kept samples would be
    5 GB): yields dicts with the fields of read_sample_file for a single kept iteration.  Memory-mapped, nothing is copied but
    the record being looked at."""
    with open(path, "rb") as f:
        P, nvb, nsets, nfix, ncls, rec, sets, rq, lv, nthr = _sample_header(f, path)
        off = f.tell()
        size = os.fstat(f.fileno()).st_size
    n = (size - off) // rec
    if n <= 0:
        return
    at, nd0 = _sample_fields(P, nvb, nsets, nfix, ncls, rq, lv)
    rcs, nd = _sample_rc(sets, nd0, P)
    mm = np.memmap(path, dtype=np.uint8, mode="r", offset=off, shape=(n, rec))
    for i in range(n):
        d = np.frombuffer(mm[i, :nd * 8].tobytes(), dtype=np.float64)
        out = _sample_record(d, at, rq, lv)
        out.update(iter=int(np.frombuffer(mm[i, :8].tobytes(), dtype=np.int64)[0]), sets=sets, delta=np.asarray(mm[i, nd * 8:nd * 8 + P]))
        if rcs:
            out["annotProb"] = {si: d[o:o + A * nc].reshape(A, nc).T for si, nc, A, o, _ in rcs}
            out["annotCat"] = {si: np.asarray(mm[i, nd * 8 + c:nd * 8 + c + nc]) for si, nc, A, _, c in rcs}
        if nthr:
            to = nd * 8 + P + sum(nc for _, nc, _, _, _ in rcs)
            out["thr"] = np.frombuffer(mm[i, to:to + 8 * nthr].tobytes(), dtype=np.float64)
        yield out
    del mm


def k_csr(K):
    """A random-effect set's K as CSR arrays (int64 k_ptr, int32 k_col, float64 k_val): a (k_ptr, k_col, k_val) triple is passed on as
    it is, a dense q x q array by its nonzero entries, row by row, columns ascending."""
    if isinstance(K, tuple):
        kp, kc, kv = K
        return (np.ascontiguousarray(kp, dtype=np.int64), np.ascontiguousarray(kc, dtype=np.int32), np.ascontiguousarray(kv, dtype=np.float64))
    K = np.asarray(K, dtype=np.float64)
    if K.ndim != 2 or K.shape[0] != K.shape[1]:
        raise ValueError("K: a q x q matrix or a CSR triple")
    nz = K != 0.0
    kp = np.concatenate([[0], np.cumsum(nz.sum(axis=1))]).astype(np.int64)
    rows, cols = np.nonzero(nz)
    return kp, np.ascontiguousarray(cols, dtype=np.int32), np.ascontiguousarray(K[rows, cols], dtype=np.float64)


def factors_csc(codes, covariates=None):
    """Factors and covariates as one sparse design in CSC form: (N, ncol, col_ptr int64, row int32, val float64).  codes: a list of int
    arrays, one per factor; code c >= 0 puts a 1.0 into column c of that factor, -1 is the base level (no column).  covariates: None,
    an N vector or an N x k array, stored as full columns behind the factors.  Rows ascend inside every column.  No dense matrix is
    built.  A level without a record (an empty column) is a ValueError."""
    codes = [np.asarray(c, dtype=np.int64) for c in codes]
    cov = None if covariates is None else np.asarray(covariates, dtype=np.float64)
    if cov is not None and cov.ndim == 1:
        cov = cov[:, None]
    if not codes and cov is None:
        raise ValueError("no factor and no covariate")
    N = len(codes[0]) if codes else cov.shape[0]
    counts, rows, vals = [], [], []
    for f, c in enumerate(codes):
        if c.ndim != 1 or len(c) != N or (len(c) and c.min() < -1):
            raise ValueError(f"factor {f}: {N} codes, each -1 (base level) or a level 0, 1, ...")
        q = int(c.max()) + 1 if len(c) else 0
        keep = np.nonzero(c >= 0)[0]
        order = keep[np.argsort(c[keep], kind="stable")]            # by level, records ascending inside a level
        cnt = np.bincount(c[keep], minlength=q)
        if np.any(cnt == 0):
            raise ValueError(f"factor {f}: level {int(np.nonzero(cnt == 0)[0][0])} has no record")
        counts.append(cnt); rows.append(order); vals.append(np.ones(len(order)))
    if cov is not None:
        if cov.shape[0] != N:
            raise ValueError(f"covariates: {cov.shape[0]} rows for {N} records")
        for j in range(cov.shape[1]):
            counts.append(np.array([N])); rows.append(np.arange(N)); vals.append(cov[:, j])
    cp = np.concatenate([[0], np.cumsum(np.concatenate(counts))]).astype(np.int64)
    return (N, len(cp) - 1, cp, np.ascontiguousarray(np.concatenate(rows), dtype=np.int32),
            np.ascontiguousarray(np.concatenate(vals), dtype=np.float64))


def dense_csc(X):
    """The nonzero entries of a dense N x ncol design in CSC form: (N, ncol, col_ptr, row, val) as factors_csc returns them."""
    X = np.asarray(X, dtype=np.float64)
    if X.ndim != 2:
        raise ValueError("X: an N x ncol matrix")
    nz = (X != 0.0).T                                                # by columns, rows ascending
    cols, rows = np.nonzero(nz)
    cp = np.concatenate([[0], np.cumsum(nz.sum(axis=1))]).astype(np.int64)
    return X.shape[0], X.shape[1], cp, np.ascontiguousarray(rows, dtype=np.int32), np.ascontiguousarray(X[rows, cols], dtype=np.float64)


def tuple_columns(col0, nloc, k):
    """Panel columns of a Tuple (correlated BayesPR) set: array [nloc, k], component m of locus l at col0 + 64 (l // Lb) + k (l % Lb) + m
    with Lb = 64 // k loci per 64-column block (include/nextgp_hip.h, ngp_add_marker_set_tuple)."""
    if col0 % 64 or not 1 <= k <= 4:
        raise ValueError("tuple set: col0 on a 64-column boundary, k in 1..4")
    l = np.arange(nloc, dtype=np.int64)[:, None]
    Lb = 64 // k
    return col0 + 64 * (l // Lb) + k * (l % Lb) + np.arange(k, dtype=np.int64)[None, :]


def tuple_span(nloc, k):
    """Panel columns a tuple set occupies from its first column on (holes included)."""
    Lb = 64 // k
    nblk = (nloc + Lb - 1) // Lb
    return 64 * (nblk - 1) + k * (nloc - Lb * (nblk - 1))


def tuple_panel(sets):
    """k matrices (N x nloc, one per correlated set, same loci) -> the interleaved N x span block a tuple set occupies (unused
    columns zero), same dtype."""
    k, (N, nloc) = len(sets), sets[0].shape
    out = np.zeros((N, tuple_span(nloc, k)), dtype=sets[0].dtype, order="F")
    cols = tuple_columns(0, nloc, k)
    for m, X in enumerate(sets):
        out[:, cols[:, m]] = X
    return out

# every symbol include/nextgp_hip.h declares
SYMBOLS = [
    "ngp_abi_version", "ngp_create", "ngp_destroy", "ngp_last_error", "ngp_set_panel_f64", "ngp_set_panel_f32", "ngp_set_panel_u8",
    "ngp_begin_panel", "ngp_panel_columns_f64", "ngp_panel_columns_f32", "ngp_panel_columns_u8", "ngp_end_panel",
    "ngp_generate_panel", "ngp_get_layout", "ngp_get_mpm", "ngp_get_gram", "ngp_xbeta", "ngp_add_marker_set", "ngp_set_y",
    "ngp_set_residual_prior", "ngp_set_intercept", "ngp_set_schedule", "ngp_run", "ngp_get_state", "ngp_set_state",
    "ngp_get_trace", "ngp_get_posterior_sums", "ngp_posterior_len", "ngp_export_posterior_device", "ngp_sweep_set", "ngp_sweep_set_dev",
    "ngp_get_timing", "ngp_profile_iteration", "ngp_draws_indexed", "ngp_eval_math", "ngp_configure", "ngp_get_config", "ngp_debug_stamps", "ngp_set_near_lags", "ngp_get_near_lags",
    "ngp_set_streamer", "ngp_get_streamer", "ngp_set_storage", "ngp_get_storage", "ngp_set_max_shards", "ngp_shards_for_chains", "ngp_run_many", "ngp_write_panel_file", "ngp_read_panel_header", "ngp_load_panel_file", "ngp_debug_set_mode", "ngp_debug_set_knob", "ngp_set_posterior_sums", "ngp_save_snapshot", "ngp_load_snapshot",
    "ngp_set_trace_loci", "ngp_get_trace_ext", "ngp_allreduce_posterior", "ngp_add_marker_set_r", "ngp_get_class_state", "ngp_set_class_state", "ngp_add_fixed_set", "ngp_add_fixed_set_sparse", "ngp_get_fixed", "ngp_set_fixed", "ngp_debug_throw", "ngp_get_census", "ngp_debug_set_virtual_device", "ngp_debug_fail_census", "ngp_add_marker_set_tuple", "ngp_share_panel", "ngp_shards_for_pass", "ngp_set_sample_file",
    "ngp_set_chain_form", "ngp_get_chain_form", "ngp_get_setup_timing", "ngp_set_residual_weights", "ngp_get_residual_weights",
    "ngp_add_random_set", "ngp_get_random", "ngp_set_random", "ngp_sample_random_set",
    "ngp_add_marker_set_lv", "ngp_get_lv_state", "ngp_set_lv_state",
    "ngp_grm_begin", "ngp_grm_columns_f64", "ngp_grm_columns_f32", "ngp_grm_columns_u8", "ngp_grm_end", "ngp_grm_get", "ngp_grm_invert",
    "ngp_add_random_set_dense", "ngp_set_records",
    "ngp_set_random_schedule", "ngp_get_random_schedule", "ngp_pedigree_ainv",
    "ngp_pedigree_a22", "ngp_grm_single_step", "ngp_add_random_set_hybrid",
    "ngp_add_random_set_tuple", "ngp_get_random_tuple", "ngp_set_random_tuple", "ngp_sample_random_set_tuple",
    "ngp_get_warmer",
    "ngp_add_marker_set_rc", "ngp_get_rc_state", "ngp_set_rc_state",
    "ngp_begin_prediction_panel", "ngp_prediction_columns_f64", "ngp_prediction_columns_f32", "ngp_prediction_columns_u8",
    "ngp_end_prediction_panel", "ngp_load_prediction_file", "ngp_get_prediction_layout", "ngp_get_prediction", "ngp_set_prediction",
    "ngp_get_prediction_last", "ngp_get_prediction_stats",
    "ngp_set_variance_windows", "ngp_enable_genomic_variance", "ngp_get_genomic_variance_layout", "ngp_get_genomic_variance",
    "ngp_set_genomic_variance", "ngp_get_genomic_variance_trace", "ngp_get_genomic_variance_stats",
    "ngp_set_holdout", "ngp_get_holdout", "ngp_set_holdout_state", "ngp_get_holdout_layout",
    "ngp_set_liability_classes", "ngp_set_liability_bounds", "ngp_get_liability_layout", "ngp_get_liability", "ngp_set_liability_state",
    "ngp_get_liability_stats", "ngp_fix_residual_variance", "ngp_tnormal_indexed",
    "ngp_debug_set_staging_bytes",
    "ngp_set_threshold_step", "ngp_get_threshold_step", "ngp_set_threshold_step_state",
    "ngp_enable_class_probabilities", "ngp_get_class_probabilities", "ngp_set_class_probabilities", "ngp_debug_pnorm",
    "ngp_enable_diagnostics", "ngp_get_diagnostics_layout", "ngp_get_diagnostics", "ngp_get_diagnostics_state", "ngp_set_diagnostics_state",
    "ngp_get_diagnostics_stats", "ngp_debug_time_diagnostics",
    "ngp_panel_columns_bed", "ngp_prediction_columns_bed",
]

BED_MISSING = {"error": 0, "mean": 1, "round": 2}   # NGP_BED_MISSING_*

THRESHOLD_STEPS = {"albert-chib": 0, "cowles": 1}

_lib = None


def prediction_summary(ps):
    """Mean and SD per row of prediction sums ({"sum", "sum2", "nKept"}; sums of several chains may have been added up)."""
    n = int(ps["nKept"])
    if n < 1:
        raise ValueError("no kept draw yet: the prediction sums are empty")
    mean = ps["sum"] / n
    sd = np.sqrt(np.maximum(0.0, ps["sum2"] / n - mean * mean))
    return dict(nKept=n, mean=mean[-1], sd=sd[-1], sets=[dict(mean=mean[s], sd=sd[s]) for s in range(mean.shape[0] - 1)])


def holdout_summary(hs):
    """Mean and SD of the fitted value of every record of hold-out sums ({"sum_fit", "sum_fit2", "n_fit"}, N entries each; the sums of
    several fold-chains may have been added up): {"rows" (the records with at least one kept draw), "n", "mean", "sd"}."""
    n = np.asarray(hs["n_fit"], dtype=np.float64)
    rows = np.flatnonzero(n > 0)
    if len(rows) == 0:
        raise ValueError("no kept draw yet: the hold-out sums are empty")
    mean = np.asarray(hs["sum_fit"])[rows] / n[rows]
    sd = np.sqrt(np.maximum(0.0, np.asarray(hs["sum_fit2"])[rows] / n[rows] - mean * mean))
    return dict(rows=rows.astype(np.int64), n=n[rows].astype(np.int64), mean=mean, sd=sd)


def class_metrics(prob, obs):
    """Scores of class probabilities prob[n][C] against the observed classes obs[n] (1..C): {"n", "brier" (sum over the classes of the
    squared error, mean over the records), "logloss" (mean of -log p of the observed class, p floored at the smallest normal double),
    "class_accuracy" (share of the records whose most probable class is the observed one; ties go to the lower class)} and, for
    C == 2, "auc": the probability that a record of class 2 has a larger p_2 than a record of class 1, ties counting half (NaN when a
    class has no record)."""
    p = np.asarray(prob, dtype=np.float64)
    o = np.asarray(obs).astype(np.int64)
    n, nc = p.shape
    if n == 0:
        out = dict(n=0, brier=float("nan"), logloss=float("nan"), class_accuracy=float("nan"))
        if nc == 2:
            out["auc"] = float("nan")
        return out
    hit = np.zeros_like(p)
    hit[np.arange(n), o - 1] = 1.0
    po = p[np.arange(n), o - 1]
    out = dict(n=int(n), brier=float(((p - hit) ** 2).sum(axis=1).mean()), logloss=float(-np.log(np.maximum(po, np.finfo(np.float64).tiny)).mean()),
               class_accuracy=float((p.argmax(axis=1) + 1 == o).mean()))
    if nc == 2:
        npos, nneg = int((o == 2).sum()), int((o == 1).sum())
        if npos and nneg:   # rank-sum with average ranks
            _, inv, cnt = np.unique(p[:, 1], return_inverse=True, return_counts=True)
            rank = (np.cumsum(cnt) - (cnt - 1) / 2.0)[inv]
            out["auc"] = float((rank[o == 2].sum() - npos * (npos + 1) / 2.0) / (float(npos) * float(nneg)))
        else:
            out["auc"] = float("nan")
    return out


LIABILITY_MAX_CLASSES = 8


def check_classes(cls, N, C_=None):
    """cls as the int32 vector ngp_set_liability_classes takes: N integers in 1..C, 2 <= C <= 8 (C_ or the largest class)."""
    a = np.asarray(cls)
    if a.shape != (N,):
        raise ValueError(f"classes: one entry per record ({N})")
    c = a.astype(np.int32)
    if not np.array_equal(c, a):
        raise ValueError("classes: integers 1..C")
    nc = int(c.max()) if C_ is None else int(C_)
    if nc < 2 or nc > LIABILITY_MAX_CLASSES:
        raise ValueError(f"classes: between 2 and {LIABILITY_MAX_CLASSES} classes, not {nc}")
    return np.ascontiguousarray(c)  # (the range 1..C is checked where the held-out rows, whose entries are not read, are known)


def class_codes(y):
    """Classes of a categorical response: the sorted distinct values of y become 1..C; a NaN (a record without a response) gets 0.
    Returns (codes int32, the distinct values)."""
    y = np.asarray(y, dtype=np.float64)
    obs = ~np.isnan(y)
    vals = np.unique(y[obs])
    if len(vals) < 2 or len(vals) > LIABILITY_MAX_CLASSES:
        raise ValueError(f'trait="categorical": the response takes {len(vals)} distinct values; between 2 and {LIABILITY_MAX_CLASSES} classes are supported')
    codes = np.zeros(len(y), dtype=np.int32)
    codes[obs] = np.searchsorted(vals, y[obs]) + 1
    return codes, vals


def check_bounds(rows, lo, hi, N):
    """(rows int64, lo, hi) as ngp_set_liability_bounds takes them: strictly increasing rows in [0, N), lo < hi, one of them finite."""
    r = np.ascontiguousarray(rows, dtype=np.int64)
    lo = np.ascontiguousarray(lo, dtype=np.float64); hi = np.ascontiguousarray(hi, dtype=np.float64)
    if r.ndim != 1 or len(r) == 0 or lo.shape != r.shape or hi.shape != r.shape:
        raise ValueError("censored records: rows, lo and hi are non-empty vectors of one length")
    if r[0] < 0 or r[-1] >= N or np.any(np.diff(r) <= 0):
        raise ValueError(f"censored records: rows strictly increasing in 0..{N - 1}")
    if not np.all(lo < hi) or np.any(~np.isfinite(lo) & ~np.isfinite(hi)):
        raise ValueError("censored records: lo < hi, at least one of them finite")
    return r, lo, hi


def censored_bounds(lower, upper):
    """runLMEM(censored={"lower", "upper"}): (rows, lo, hi) of the censored records.  A record with lower == upper is exact (not
    listed); NaN or an infinity means open on that side; a record open on both sides, or with lower > upper, raises ValueError."""
    lo = np.asarray(lower, dtype=np.float64).copy(); hi = np.asarray(upper, dtype=np.float64).copy()
    if lo.ndim != 1 or lo.shape != hi.shape:
        raise ValueError("censored: lower and upper have one entry per record")
    lo[np.isnan(lo)] = -np.inf; hi[np.isnan(hi)] = np.inf
    if np.any(lo > hi) or np.any(np.isinf(lo) & np.isinf(hi)):
        raise ValueError("censored: lower <= upper, and at least one of them finite, at every record")
    rows = np.flatnonzero(lo < hi).astype(np.int64)
    return rows, lo[rows], hi[rows]


def deal_folds(y, folds, foldSeed=1):
    """Fold of every record for K-fold cross-validation: the records with an observed (non-NaN) response, in the order of
    np.random.default_rng(foldSeed).permutation, dealt round-robin into folds 0 .. K-1; a record without a response gets -1."""
    y = np.asarray(y, dtype=np.float64)
    K = int(folds)
    obs = np.flatnonzero(~np.isnan(y))
    if K < 2 or K > len(obs):
        raise ValueError(f"folds={folds}: between 2 and the number of records with a response ({len(obs)})")
    fold = np.full(len(y), -1, dtype=np.int64)
    fold[obs[np.random.default_rng(foldSeed).permutation(len(obs))]] = np.arange(len(obs)) % K
    return fold


def genomic_variance_names(nwin_per_set):
    """Slot names in slot order: "set<s>:win_<k>" for the windows of every set, then "set<s>", then "total"."""
    return ([f"set{s}:win_{k + 1}" for s, n in enumerate(nwin_per_set) for k in range(n)] + [f"set{s}" for s in range(len(nwin_per_set))] + ["total"])


def genomic_variance_summary(gs, names=None):
    """Means, SDs and WPPA per slot of genomic-variance sums ({"sumV", "sumV2", "sumQ", "sumQ2", "count", "ratio", "nKept"}; sums of
    several chains may have been added up): mean / SD of V and of q = V / V_g, wppa = share of the draws with q > threshold, and
    ratio = mean and SD of V_g / (V_g + varE)."""
    n = int(gs["nKept"])
    if n < 1:
        raise ValueError("no kept draw yet: the genomic-variance sums are empty")
    mV, mQ = gs["sumV"] / n, gs["sumQ"] / n
    out = dict(nKept=n, meanV=mV, sdV=np.sqrt(np.maximum(0.0, gs["sumV2"] / n - mV * mV)), meanQ=mQ,
               sdQ=np.sqrt(np.maximum(0.0, gs["sumQ2"] / n - mQ * mQ)), wppa=gs["count"] / n)
    mr = gs["ratio"][0] / n
    out["ratio"] = (mr, float(np.sqrt(max(0.0, gs["ratio"][1] / n - mr * mr))))
    if names is not None:
        out["names"] = list(names)
    return out


class NextGPHipError(RuntimeError):
    pass


def load():
    """dlopen the HIP library; raises if it has not been built (see __graft_entry__.build)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise NextGPHipError(
                f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
        L = C.CDLL(LIB_PATH)
        L.ngp_last_error.restype = C.c_char_p
        L.ngp_last_error.argtypes = [C.c_void_p]
        _lib = L
    return _lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None else None


def _columns(M):
    """(array, ctypes element type, suffix, leading dimension) of a host matrix handed over in whole columns: uint8 and float32 go as they
    are, anything else as float64.  The first N rows of a taller Fortran-ordered array (M = big[:N]) go over without a copy, with the
    parent's leading dimension; everything else is made Fortran-contiguous."""
    M = np.asarray(M)
    t, sfx = {np.dtype(np.uint8): (C.c_uint8, "u8"), np.dtype(np.float32): (C.c_float, "f32")}.get(M.dtype, (C.c_double, "f64"))
    if t is C.c_double and M.dtype != np.float64:
        M = np.asfortranarray(M, dtype=np.float64)
    if M.ndim != 2:
        raise ValueError("a matrix of N rows and one column per marker")
    if not (M.strides[0] == M.itemsize and M.strides[1] % M.itemsize == 0 and M.strides[1] >= M.shape[0] * M.itemsize):
        M = np.asfortranarray(M)
    return M, t, sfx, max(M.strides[1] // M.itemsize, M.shape[0])


def write_panel_file(path, G, bits=8):
    """Genotype codes (N x P, uint8) as a binary panel file: 8 bits per genotype, or 2 (allele counts 0/1/2 only)."""
    G = np.asfortranarray(G, dtype=np.uint8)
    rc = load().ngp_write_panel_file(str(path).encode(), _p(G, C.c_uint8), C.c_int64(G.shape[0]), C.c_int64(G.shape[1]),
                                     C.c_int64(G.shape[0]), C.c_int32(bits))
    if rc != 0:
        raise NextGPHipError(f"ngp_write_panel_file failed ({rc}): path not writable, or codes above 2 with bits=2")


def pedigree_ainv(sire, dam):
    """(F, (k_ptr, k_col, k_val)): inbreeding coefficients and A^-1 as CSR (columns ascending) of a pedigree listed parents first; sire /
    dam are 1-based positions in the list, 0 = unknown (ngp_pedigree_ainv: Henderson's rules with inbreeding, on the host)."""
    s = np.ascontiguousarray(sire, dtype=np.int32); d = np.ascontiguousarray(dam, dtype=np.int32)
    if s.ndim != 1 or s.shape != d.shape or len(s) < 1:
        raise ValueError("pedigree: one sire and one dam per animal")
    n = len(s)
    L = load()
    F = np.empty(n); kp = np.empty(n + 1, dtype=np.int64); nnz = C.c_int64(0)
    rc = L.ngp_pedigree_ainv(C.c_int64(n), _p(s, C.c_int32), _p(d, C.c_int32), _p(F, C.c_double), _p(kp, C.c_int64), None, None, C.c_int64(0),
                             C.byref(nnz))
    if rc != 0 and nnz.value <= 0:
        raise NextGPHipError(f"ngp_pedigree_ainv failed ({rc}): " + (L.ngp_last_error(None) or b"").decode())
    kc = np.empty(nnz.value, dtype=np.int32); kv = np.empty(nnz.value)
    rc = L.ngp_pedigree_ainv(C.c_int64(n), _p(s, C.c_int32), _p(d, C.c_int32), _p(F, C.c_double), _p(kp, C.c_int64), _p(kc, C.c_int32),
                             _p(kv, C.c_double), C.c_int64(nnz.value), C.byref(nnz))
    if rc != 0:
        raise NextGPHipError(f"ngp_pedigree_ainv failed ({rc}): " + (L.ngp_last_error(None) or b"").decode())
    return F, (kp, kc, kv)


def pedigree_a22(sire, dam, F, idx):
    """A[idx, idx] of a pedigree without the dense A (ngp_pedigree_a22: Colleau's indirect method, one O(n) column per listed animal,
    on the host).  sire / dam as pedigree_ainv takes them, F the inbreeding coefficients it returns, idx 0-based positions."""
    s = np.ascontiguousarray(sire, dtype=np.int32); d = np.ascontiguousarray(dam, dtype=np.int32)
    f = np.ascontiguousarray(F, dtype=np.float64); ix = np.ascontiguousarray(idx, dtype=np.int64)
    if s.ndim != 1 or s.shape != d.shape or f.shape != s.shape or ix.ndim != 1 or len(ix) < 1:
        raise ValueError("pedigree_a22: one sire, dam and F per animal, and at least one listed animal")
    m = len(ix)
    out = np.empty((m, m))
    L = load()
    rc = L.ngp_pedigree_a22(C.c_int64(len(s)), _p(s, C.c_int32), _p(d, C.c_int32), _p(f, C.c_double), _p(ix, C.c_int64), C.c_int64(m),
                            _p(out, C.c_double), C.c_int64(m))
    if rc != 0:
        raise NextGPHipError(f"ngp_pedigree_a22 failed ({rc}): " + (L.ngp_last_error(None) or b"").decode())
    return out


def read_panel_header(path):
    n, p, b = C.c_int64(), C.c_int64(), C.c_int32()
    rc = load().ngp_read_panel_header(str(path).encode(), C.byref(n), C.byref(p), C.byref(b))
    if rc != 0:
        raise NextGPHipError(f"not a panel file: {path}")
    return n.value, p.value, b.value


class Sampler:
    """One chain on one device == one `ngp_handle` (reference: one Julia task running runSampler!)."""

    def __init__(self, device=0, seed=1, chain=0, mode=None, lag=None, streamer=None, storage=None):
        self.L = load()
        self.h = C.c_void_p()
        rc = self.L.ngp_create(C.c_int32(device), C.c_uint64(seed), C.c_uint32(chain), C.byref(self.h))
        if rc != 0:
            raise NextGPHipError(f"ngp_create failed ({rc}): " + (self.L.ngp_last_error(None) or b"").decode())
        self.nsets = 0
        self.set_shapes = []  # (ncol, nreg) per set
        self.ntl = 0
        self.ntvb = 0
        if mode is not None or lag is not None:
            self.configure(1 if mode is None else mode, 8 if lag is None else lag)
        if streamer is not None:
            self.set_streamer(streamer)
        if storage is not None:
            self.set_storage(storage)

    def configure(self, mode, lag):
        self._chk(self.L.ngp_configure(self.h, C.c_int32(mode), C.c_int32(lag)))

    def set_near(self, near):
        self._chk(self.L.ngp_set_near_lags(self.h, C.c_int32(near)))

    def near(self):
        n = C.c_int32()
        self._chk(self.L.ngp_get_near_lags(self.h, C.byref(n)))
        return n.value

    def setup_timing(self):
        """Parts of the last generate_panel in ms: dict(alloc_ms, tiles_ms, gram_ms)."""
        a, t, g = C.c_double(), C.c_double(), C.c_double()
        self._chk(self.L.ngp_get_setup_timing(self.h, C.byref(a), C.byref(t), C.byref(g)))
        return dict(alloc_ms=a.value, tiles_ms=t.value, gram_ms=g.value)

    def set_chain_form(self, form):
        """0 (default): the 64 serial steps per block; 1: linear blocks (BayesPR, BayesLV, Tuple) as dlt = T e0 (k_tinv).  May be called
        between runs of one chain: the next run takes the new form."""
        self._chk(self.L.ngp_set_chain_form(self.h, C.c_int32(int(form))))

    def chain_form(self):
        n = C.c_int32()
        self._chk(self.L.ngp_get_chain_form(self.h, C.byref(n)))
        return n.value

    def set_streamer(self, variant):
        self._chk(self.L.ngp_set_streamer(self.h, C.c_int32(variant)))

    def set_max_shards(self, n):
        self._chk(self.L.ngp_set_max_shards(self.h, C.c_int32(int(n))))

    def shards_for_chains(self, chains):
        """The largest max_shards with which `chains` chains share this device side by side."""
        v = C.c_int32()
        self._chk(self.L.ngp_shards_for_chains(self.h, C.c_int32(int(chains)), C.byref(v)))
        return v.value

    def shards_for_pass(self, chains):
        """The largest max_shards with which `chains` chains share one fused sweep launch (K chains per pass)."""
        v = C.c_int32()
        self._chk(self.L.ngp_shards_for_pass(self.h, C.c_int32(int(chains)), C.byref(v)))
        return v.value

    def share_panel(self, owner):
        """Take `owner`'s panel by reference (K chains per pass): same tiles, Gram window and layout; chain state is this handle's."""
        self._chk(self.L.ngp_share_panel(self.h, owner.h))
        self.N, self.P = owner.N, owner.P
        self._panel_owner = owner   # keeps the owner's Python object alive as long as this one

    def set_storage(self, storage):
        """0 / "f32": centred fp32 tiles; 1 / "u8": compact storage (bytes + Float64 column means, analytic centring)."""
        code = {"f32": 0, "u8": 1}.get(storage, storage)
        self._chk(self.L.ngp_set_storage(self.h, C.c_int32(int(code))))

    def storage(self):
        v = C.c_int32()
        self._chk(self.L.ngp_get_storage(self.h, C.byref(v), None, C.c_int64(0)))
        return v.value

    def means(self):
        """Compact storage: the P column means the centring uses."""
        out = np.zeros(self.P)
        v = C.c_int32()
        self._chk(self.L.ngp_get_storage(self.h, C.byref(v), _p(out, C.c_double), C.c_int64(self.P)))
        return out

    def streamer(self):
        """(variant in force, GEMV chains per shard partial)"""
        v, n = C.c_int32(), C.c_int32()
        self._chk(self.L.ngp_get_streamer(self.h, C.byref(v), C.byref(n)))
        return v.value, n.value

    def debug_set_knob(self, knob):
        self._chk(self.L.ngp_debug_set_knob(self.h, C.c_int32(knob)))

    def debug_set_staging_bytes(self, nbytes):
        """Test hook: the size every staged loader takes for its chunk in place of 256 MiB / 64 MiB (0: those)."""
        self._chk(self.L.ngp_debug_set_staging_bytes(self.h, C.c_int64(int(nbytes))))

    def debug_set_mode(self, mode):
        self._chk(self.L.ngp_debug_set_mode(self.h, C.c_int32(mode)))

    def config(self):
        m, l = C.c_int32(), C.c_int32()
        self._chk(self.L.ngp_get_config(self.h, C.byref(m), C.byref(l)))
        return m.value, l.value

    def debug_stamps(self, enable=True, n=0):
        out = np.zeros(max(n, 1), dtype=np.uint64)
        self._chk(self.L.ngp_debug_stamps(self.h, C.c_int32(int(enable)), _p(out, C.c_uint64) if n else None, C.c_int64(n)))
        return out

    def _chk(self, rc):
        if rc != 0:
            raise NextGPHipError(f"libnextgp_hip error {rc}: " + (self.L.ngp_last_error(self.h) or b"").decode())

    def close(self):
        if getattr(self, "h", None):
            self.L.ngp_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- panel -------------------------------------------------------------------------
    def load_panel_file(self, path, centre=True):
        """Binary panel file (write_panel_file) straight into the tiles of this handle's storage."""
        n, p, _ = read_panel_header(path)
        self._chk(self.L.ngp_load_panel_file(self.h, str(path).encode(), C.c_int32(1 if centre else 0)))
        self.N, self.P = n, p

    def set_panel(self, M, centre=False):
        """uint8 (one byte per genotype: converted and centred on the device), float32 or float64; big[:N] of a taller Fortran-ordered
        array goes over without a copy (_columns)."""
        M, t, sfx, ld = _columns(M)
        self.N, self.P = M.shape
        f = getattr(self.L, "ngp_set_panel_" + sfx)
        self._chk(f(self.h, _p(M, t), C.c_int64(self.N), C.c_int64(self.P), C.c_int64(ld), C.c_int32(int(centre))))

    def begin_panel(self, N, P):
        """A panel handed over in column ranges (one marker set after another, no concatenated host copy): begin_panel,
        panel_columns(col0, M) for every range, end_panel."""
        self._chk(self.L.ngp_begin_panel(self.h, C.c_int64(N), C.c_int64(P)))
        self.N, self.P = N, P

    def panel_columns(self, col0, M, centre=False):
        """uint8 (genotype codes: the only form the compact storage takes), float32 or float64; big[:N] without a copy (_columns)."""
        M, t, sfx, ld = _columns(M)
        f = getattr(self.L, "ngp_panel_columns_" + sfx)
        self._chk(f(self.h, C.c_int64(col0), _p(M, t), C.c_int64(M.shape[1]), C.c_int64(ld), C.c_int32(int(centre))))

    def _columns_bed(self, f, col0, packed, n_file, rows, allele, missing, centre):
        packed = np.asanyarray(packed)   # (a memmap stays a memmap: the library reads the file's pages, no copy)
        if packed.dtype != np.uint8 or packed.ndim != 2 or not packed.flags.c_contiguous:
            raise ValueError("packed .bed columns: a C-ordered uint8 array of (ncol, stride), one row per SNP")
        if missing not in BED_MISSING:
            raise ValueError(f"missing-call policy {missing!r}: one of 'error', 'mean', 'round'")
        ncol, stride = packed.shape
        r = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
        counts = np.zeros((ncol, 4), dtype=np.int64)
        self._chk(f(self.h, C.c_int64(col0), _p(packed, C.c_uint8), C.c_int64(ncol), C.c_int64(stride), C.c_int64(int(n_file)), _p(r, C.c_int64),
                    C.c_int32(int(allele)), C.c_int32(BED_MISSING[missing]), C.c_int32(int(centre)), _p(counts, C.c_int64)))
        return counts

    def panel_columns_bed(self, col0, packed, n_file, rows=None, allele=1, missing="mean", centre=True):
        """Packed PLINK .bed columns (read_plink()["bed"][a:b]: (ncol, stride) uint8, one row per SNP of n_file samples) into columns
        col0 .. of the open panel, decoded on the device.  rows: the file's sample of every panel row (None: file order); allele: count
        A1 or A2; missing: "error", "mean" (fp32 storage) or "round".  Returns the (ncol, 4) counts of 0, 1, 2 and missing calls."""
        return self._columns_bed(self.L.ngp_panel_columns_bed, col0, packed, n_file, rows, allele, missing, centre)

    def prediction_columns_bed(self, col0, packed, n_file, rows=None, allele=1, missing="mean", centre=True):
        """The same into the open prediction panel: the training means are subtracted, and a missing call takes the training mean
        ("mean") or the training mean rounded to a code ("round")."""
        return self._columns_bed(self.L.ngp_prediction_columns_bed, col0, packed, n_file, rows, allele, missing, centre)

    def end_panel(self):
        self._chk(self.L.ngp_end_panel(self.h))

    def generate_panel(self, N, P, maf_lo=0.05, maf_hi=0.5, seed=20250509):
        self._chk(self.L.ngp_generate_panel(self.h, C.c_int64(N), C.c_int64(P), C.c_double(maf_lo), C.c_double(maf_hi),
                                            C.c_uint64(seed)))
        self.N, self.P = N, P

    def layout(self):
        R, S, nb = C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(self.L.ngp_get_layout(self.h, C.byref(R), C.byref(S), C.byref(nb)))
        return R.value, S.value, nb.value

    def mpm(self):
        out = np.empty(self.P)
        self._chk(self.L.ngp_get_mpm(self.h, _p(out, C.c_double), C.c_int64(self.P)))
        return out

    def gram(self, t):
        out = np.empty((64, 64))
        self._chk(self.L.ngp_get_gram(self.h, C.c_int64(t), _p(out, C.c_double)))
        return out

    def xbeta(self, beta):
        beta = np.ascontiguousarray(beta, dtype=np.float64)
        out = np.empty(self.N)
        self._chk(self.L.ngp_xbeta(self.h, _p(beta, C.c_double), C.c_int64(len(beta)), _p(out, C.c_double), C.c_int64(self.N)))
        return out

    # ---- prediction panel: new individuals x the training panel's columns ---------------
    def begin_prediction_panel(self, Np):
        """A prediction panel of Np individuals beside the training panel: begin_prediction_panel, prediction_columns(col0, M)
        for every column range, end_prediction_panel.  Every kept iteration then accumulates g = X_new beta (prediction())."""
        self._chk(self.L.ngp_begin_prediction_panel(self.h, C.c_int64(Np)))

    def prediction_columns(self, col0, M, centre=False):
        """centre: subtract the TRAINING panel's column means (means()), never means of these rows.  Input forms as panel_columns."""
        M, t, sfx, ld = _columns(M)
        f = getattr(self.L, "ngp_prediction_columns_" + sfx)
        self._chk(f(self.h, C.c_int64(col0), _p(M, t), C.c_int64(M.shape[1]), C.c_int64(ld), C.c_int32(int(centre))))

    def end_prediction_panel(self):
        self._chk(self.L.ngp_end_prediction_panel(self.h))

    def set_prediction_panel(self, M, centre=False):
        """The three calls above for one matrix of Np x P."""
        M = np.asarray(M)
        self.begin_prediction_panel(M.shape[0])
        self.prediction_columns(0, M, centre=centre)
        self.end_prediction_panel()

    def load_prediction_file(self, path, centre=True):
        """Binary panel file (write_panel_file) of the training panel's P columns as the prediction panel."""
        self._chk(self.L.ngp_load_prediction_file(self.h, str(path).encode(), C.c_int32(1 if centre else 0)))

    def prediction_layout(self):
        """(Np, rows per shard, shards, columns per chunk of the normative sum) of the prediction panel."""
        v = [C.c_int64() for _ in range(4)]
        self._chk(self.L.ngp_get_prediction_layout(self.h, *[C.byref(x) for x in v], None))
        return tuple(x.value for x in v)

    def prediction_sums(self):
        """Sums over the kept draws: sum and sum2 are [nsets + 1][Np] (last row: all sets together), nKept the number of draws."""
        Np = self.prediction_layout()[0]
        rows = self.nsets + 1
        s1, s2, n = np.empty((rows, Np)), np.empty((rows, Np)), C.c_int64()
        self._chk(self.L.ngp_get_prediction(self.h, _p(s1, C.c_double), _p(s2, C.c_double), C.c_int64(rows), C.c_int64(Np), C.byref(n)))
        return dict(sum=s1, sum2=s2, nKept=n.value)

    def set_prediction_sums(self, ps):
        s1 = np.ascontiguousarray(ps["sum"], dtype=np.float64)
        s2 = np.ascontiguousarray(ps["sum2"], dtype=np.float64)
        self._chk(self.L.ngp_set_prediction(self.h, _p(s1, C.c_double), _p(s2, C.c_double), C.c_int64(s1.shape[0]), C.c_int64(s1.shape[1])))

    def prediction_last(self):
        """g of the last kept draw, [nsets + 1][Np]."""
        Np = self.prediction_layout()[0]
        out = np.empty((self.nsets + 1, Np))
        self._chk(self.L.ngp_get_prediction_last(self.h, _p(out, C.c_double), C.c_int64(out.shape[0]), C.c_int64(Np)))
        return out

    def prediction_stats(self):
        """(launches of the prediction pass this handle made, chains they served)."""
        a, b = C.c_int64(), C.c_int64()
        self._chk(self.L.ngp_get_prediction_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def prediction(self):
        """Posterior mean and SD of the breeding values of the prediction panel's individuals: {"nKept", "mean", "sd" (all sets
        together), "sets": [{"mean", "sd"} per marker set]}, sd = sqrt(max(0, sum2 / n - mean^2))."""
        return prediction_summary(self.prediction_sums())

    # ---- genomic variance of the kept draws: windows, sets, total, WPPA ------------------
    def set_variance_windows(self, set_id, windows):
        """Windows of marker set set_id: [(a, b), ...] half-open column ranges relative to the set's first column (ascending,
        disjoint, non-empty, inside the set); [] drops them.  Zeroes this chain's variance sums."""
        a = np.ascontiguousarray([w[0] for w in windows], dtype=np.int64)
        b = np.ascontiguousarray([w[1] for w in windows], dtype=np.int64)
        self._chk(self.L.ngp_set_variance_windows(self.h, C.c_int32(int(set_id)), _p(a, C.c_int64), _p(b, C.c_int64), C.c_int64(len(a))))
        if not hasattr(self, "_gv_nwin"):
            self._gv_nwin = {}
        self._gv_nwin[int(set_id)] = len(a)

    def enable_genomic_variance(self, on=True, threshold=0.01, trace_rows=0):
        """Every kept iteration then forms var(X beta) per window, set and in all (genomic_variance()); trace_rows: draws whose V and
        r are kept for genomic_variance_trace()."""
        self._chk(self.L.ngp_enable_genomic_variance(self.h, C.c_int32(int(bool(on))), C.c_double(threshold), C.c_int64(int(trace_rows))))

    def genomic_variance_layout(self):
        """(nslots, windows in all, marker sets, trace rows stored, draws beyond the trace's capacity)."""
        v = [C.c_int64() for _ in range(5)]
        self._chk(self.L.ngp_get_genomic_variance_layout(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def genomic_variance_names(self):
        nw = getattr(self, "_gv_nwin", {})
        return genomic_variance_names([nw.get(s, 0) for s in range(self.nsets)])

    def genomic_variance_sums(self):
        """The sums over the kept draws per slot (windows of set 0, of set 1, ..., the sets, the total): dict(sumV, sumV2, sumQ, sumQ2,
        count, last, ratio=[sum r, sum r^2], nKept)."""
        n = self.genomic_variance_layout()[0]
        a = [np.empty(n) for _ in range(6)]
        ratio, k = np.empty(2), C.c_int64()
        self._chk(self.L.ngp_get_genomic_variance(self.h, *[_p(x, C.c_double) for x in a], C.c_int64(n), _p(ratio, C.c_double), C.byref(k)))
        return dict(sumV=a[0], sumV2=a[1], sumQ=a[2], sumQ2=a[3], count=a[4], last=a[5], ratio=ratio, nKept=k.value)

    def set_genomic_variance_sums(self, gs):
        a = [np.ascontiguousarray(gs[k], dtype=np.float64) for k in ("sumV", "sumV2", "sumQ", "sumQ2", "count", "last")]
        ratio = np.ascontiguousarray(gs["ratio"], dtype=np.float64)
        self._chk(self.L.ngp_set_genomic_variance(self.h, *[_p(x, C.c_double) for x in a], C.c_int64(len(a[0])), _p(ratio, C.c_double),
                                                  C.c_int64(int(gs["nKept"]))))

    def genomic_variance(self):
        """Posterior means and SDs of V and q per slot, WPPA per slot, mean and SD of r, with slot names (genomic_variance_summary)."""
        return genomic_variance_summary(self.genomic_variance_sums(), self.genomic_variance_names())

    def genomic_variance_last(self):
        """V of the last kept draw per slot."""
        n = self.genomic_variance_layout()[0]
        out = np.empty(n)
        self._chk(self.L.ngp_get_genomic_variance(self.h, None, None, None, None, None, _p(out, C.c_double), C.c_int64(n), None, None))
        return out

    def genomic_variance_trace(self):
        """(V [rows][nslots], r [rows]) of the kept draws the trace holds."""
        n, _, _, rows, _ = self.genomic_variance_layout()
        V, r = np.empty((rows, n)), np.empty(rows)
        self._chk(self.L.ngp_get_genomic_variance_trace(self.h, _p(V, C.c_double), _p(r, C.c_double), C.c_int64(rows), C.c_int64(n)))
        return V, r

    def genomic_variance_stats(self):
        """(variance passes this handle launched, chains they served)."""
        a, b = C.c_int64(), C.c_int64()
        self._chk(self.L.ngp_get_genomic_variance_stats(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    # ---- convergence diagnostics (ngp_enable_diagnostics; DESIGN.md section 2, "Convergence diagnostics") ----
    def enable_diagnostics(self, on=True, lags=64, split=0):
        """Every kept iteration then updates a lag-window autocovariance (lags 0 .. lags-1) of every monitored scalar (diagnostics());
        draws with index < split feed half 0, the others half 1.  Zeroes the state."""
        self._chk(self.L.ngp_enable_diagnostics(self.h, C.c_int32(int(bool(on))), C.c_int32(int(lags)), C.c_int64(int(split))))

    def diagnostics_layout(self):
        """(D, lags, split, draws taken, words of the state image)."""
        D, L, H, n, w = C.c_int64(), C.c_int32(), C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(self.L.ngp_get_diagnostics_layout(self.h, C.byref(D), C.byref(L), C.byref(H), C.byref(n), C.byref(w)))
        return D.value, L.value, H.value, n.value, w.value

    def diagnostics(self):
        """dict(n, mean, var, sd, ess, mcse, truncated [D], half_n [2], half_mean, half_var [2, D]); the arrays are NaN while no draw is taken."""
        D = self.diagnostics_layout()[0]
        a = {k: np.full(D, np.nan) for k in ("mean", "var", "ess", "mcse", "truncated")}
        hn, hm, hv, n = np.zeros(2), np.full((2, D), np.nan), np.full((2, D), np.nan), C.c_int64()
        self._chk(self.L.ngp_get_diagnostics(self.h, *[_p(a[k], C.c_double) for k in ("mean", "var", "ess", "mcse", "truncated")], _p(hn, C.c_double),
                                             _p(hm, C.c_double), _p(hv, C.c_double), C.c_int64(D), C.byref(n)))
        return dict(n=n.value, sd=np.sqrt(a["var"]), half_n=hn, half_mean=hm, half_var=hv, **a)

    def diagnostics_names(self):
        """One name per monitored scalar, "<Out-file stem>:<column header>" (betaM1:M7, varM1:reg_1, varE:e): the names runLMEM derived
        from the headers of its *Out files, or theta:<i> for a chain that was built by hand."""
        D = self.diagnostics_layout()[0]
        names = getattr(self, "_diag_names", None)
        return list(names) if names is not None and len(names) == D else [f"theta:{i + 1}" for i in range(D)]

    def diagnostics_state(self):
        """dict(state, n): x1[D] | S1[2][D] | S2[2][D] | C[lags][D] | head[lags][D] | ring[lags][D] and the draws taken (resume)."""
        w = self.diagnostics_layout()[4]
        st, n = np.empty(w), C.c_int64()
        self._chk(self.L.ngp_get_diagnostics_state(self.h, _p(st, C.c_double), C.c_int64(w), C.byref(n)))
        return dict(state=st, n=n.value)

    def set_diagnostics_state(self, ds):
        st = np.ascontiguousarray(ds["state"], dtype=np.float64)
        self._chk(self.L.ngp_set_diagnostics_state(self.h, _p(st, C.c_double), C.c_int64(st.size), C.c_int64(int(ds["n"]))))

    def diagnostics_stats(self):
        """Updates this handle launched."""
        a = C.c_int64()
        self._chk(self.L.ngp_get_diagnostics_stats(self.h, C.byref(a)))
        return a.value

    def debug_time_diagnostics(self, reps=20):
        """(ms per full-window update, ms per finalise kernel) between device events; the chain's state is not touched."""
        a, b = C.c_double(), C.c_double()
        self._chk(self.L.ngp_debug_time_diagnostics(self.h, C.c_int32(int(reps)), C.byref(a), C.byref(b)))
        return a.value, b.value

    # ---- model -------------------------------------------------------------------------
    def add_marker_set(self, col0, ncol, method, df, scale, regions, varBeta0, pi0=0.0, estPi=False, lhs0=None, rhs0=None):
        rs = np.ascontiguousarray([r[0] for r in regions], dtype=np.int64)
        re = np.ascontiguousarray([r[1] for r in regions], dtype=np.int64)
        vb = np.ascontiguousarray(varBeta0, dtype=np.float64)
        if len(vb) != len(rs):
            raise ValueError("varBeta0 needs one entry per region")
        l0 = None if lhs0 is None else np.ascontiguousarray(lhs0, dtype=np.float64)
        r0 = None if rhs0 is None else np.ascontiguousarray(rhs0, dtype=np.float64)
        sid = C.c_int32()
        self._chk(self.L.ngp_add_marker_set(self.h, C.c_int64(col0), C.c_int64(ncol), C.c_int32(method), C.c_double(df),
                                            C.c_double(scale), _p(rs, C.c_int64), _p(re, C.c_int64), C.c_int64(len(rs)),
                                            _p(vb, C.c_double), C.c_double(pi0), C.c_int32(int(estPi)), _p(l0, C.c_double),
                                            _p(r0, C.c_double), C.byref(sid)))
        self.nsets += 1
        self.set_shapes.append((ncol, len(rs)))
        return sid.value

    def add_fixed_set(self, X, lhs0=None, rhs0=None):
        """Columns of one fixed-effect term / block (src/functions.jl:22-53), sampled after the intercept in the order added."""
        X = np.asfortranarray(X, dtype=np.float64)
        if X.ndim == 1:
            X = np.asfortranarray(X[:, None])
        l0 = None if lhs0 is None else np.ascontiguousarray(lhs0, dtype=np.float64)
        r0 = None if rhs0 is None else np.ascontiguousarray(rhs0, dtype=np.float64)
        sid = C.c_int32()
        self._chk(self.L.ngp_add_fixed_set(self.h, _p(X, C.c_double), C.c_int64(X.shape[0]), C.c_int64(X.shape[1]), C.c_int64(X.shape[0]),
                                           _p(l0, C.c_double), _p(r0, C.c_double), C.byref(sid)))
        self.nfixcol = getattr(self, "nfixcol", 0) + X.shape[1]
        return sid.value

    def add_fixed_set_sparse(self, N, ncol, col_ptr, row, val):
        """A fixed-effect set as a sparse N x ncol matrix in CSC form (rows strictly ascending inside a column, every column at least
        one entry, 2 <= ncol <= 2^20): a factor of many levels, or a block of crossed factors and covariates.  Bit for bit the dense
        set of the same design (add_fixed_set) wherever both exist; returns the set id."""
        cp = np.ascontiguousarray(col_ptr, dtype=np.int64)
        rw = np.ascontiguousarray(row, dtype=np.int32)
        vl = np.ascontiguousarray(val, dtype=np.float64)
        if len(cp) != int(ncol) + 1 or len(rw) != len(vl) or (len(cp) and int(cp[-1]) != len(rw)):
            raise ValueError("CSC arrays: col_ptr holds ncol + 1 offsets, row and val col_ptr[ncol] entries each")
        sid = C.c_int32()
        self._chk(self.L.ngp_add_fixed_set_sparse(self.h, C.c_int64(int(N)), C.c_int64(int(ncol)), _p(cp, C.c_int64), _p(rw, C.c_int32),
                                                  _p(vl, C.c_double), C.byref(sid)))
        self.nfixcol = getattr(self, "nfixcol", 0) + int(ncol)
        return sid.value

    def add_fixed_factors(self, codes, covariates=None):
        """One sparse fixed-effect set from factors and covariates.  codes: a list of int arrays (one per factor, N entries each), level
        codes 0, 1, ...; -1 is the base level, which gets no column.  covariates: None, or an N x k array (k columns, or one vector).
        The columns are the factors in order, each with its levels ascending, then the covariates.  Returns the set id."""
        N, ncol, cp, rw, vl = factors_csc(codes, covariates)
        return self.add_fixed_set_sparse(N, ncol, cp, rw, vl)

    def get_fixed(self):
        n = getattr(self, "nfixcol", 0)
        b = np.empty(max(n, 1)); sb = np.empty(max(n, 1)); nn = C.c_int64()
        self._chk(self.L.ngp_get_fixed(self.h, _p(b, C.c_double), _p(sb, C.c_double), C.byref(nn)))
        return dict(b=b[:nn.value].copy(), sum_b=sb[:nn.value].copy())

    def set_fixed(self, b=None, sum_b=None):
        a = None if b is None else np.ascontiguousarray(b, dtype=np.float64)
        c = None if sum_b is None else np.ascontiguousarray(sum_b, dtype=np.float64)
        self._chk(self.L.ngp_set_fixed(self.h, _p(a, C.c_double), _p(c, C.c_double), C.c_int64(getattr(self, "nfixcol", 0))))

    def add_random_set(self, level, q, K=None, df=4.0, scale=None, varU0=100.0):
        """(1|g) random-effect set (src/mme.jl:165-272): level[i] in 0..q-1 per record, K the structure's precision (None = identity; a
        scipy-free CSR triple (k_ptr, k_col, k_val), or a dense q x q array, sent as its nonzeros).  scale defaults to varU0 (df - 2) / df
        (src/mme.jl:265-272).  Sampled after the fixed-effect sets, in the order added; returns the set id."""
        lv = np.ascontiguousarray(level, dtype=np.int32)
        if scale is None:
            scale = varU0 * (df - 2.0) / df
        kp, kc, kv = k_csr(K) if K is not None else (None, None, None)
        sid = C.c_int32()
        self._chk(self.L.ngp_add_random_set(self.h, _p(lv, C.c_int32), C.c_int64(int(q)), _p(kp, C.c_int64), _p(kc, C.c_int32), _p(kv, C.c_double),
                                            C.c_double(df), C.c_double(scale), C.c_double(varU0), C.byref(sid)))
        self.rand_q = getattr(self, "rand_q", []) + [int(q)]
        return sid.value

    def add_random_set_dense(self, level, q, K=None, df=4.0, scale=None, varU0=100.0):
        """Random-effect set over a dense q x q precision (GBLUP's inv(G), or a large dense inv(Sigma)), sampled by the blocked engine.
        level: the record's level, or None for the identity incidence (record i is level i, q == N).  K: a dense symmetric array
        (copied to the device), (other_sampler, set_id) to share that set's matrix by reference, or None to take over this sampler's own
        inverted relationship matrix (grm_invert).  Everything else as add_random_set; returns the set id."""
        lv = None if level is None else np.ascontiguousarray(level, dtype=np.int32)
        if scale is None:
            scale = varU0 * (df - 2.0) / df
        Kh, src, src_set = None, None, 0
        if isinstance(K, tuple):
            src, src_set = K[0].h, int(K[1])
        elif K is not None:
            Kh = np.ascontiguousarray(K, dtype=np.float64)
            if Kh.shape != (int(q), int(q)):
                raise ValueError("K: a q x q matrix, (other_sampler, set_id) or None")
        sid = C.c_int32()
        self._chk(self.L.ngp_add_random_set_dense(self.h, _p(lv, C.c_int32), C.c_int64(int(q)), _p(Kh, C.c_double), src, C.c_int32(src_set),
                                                  C.c_double(df), C.c_double(scale), C.c_double(varU0), C.byref(sid)))
        self.rand_q = getattr(self, "rand_q", []) + [int(q)]
        return sid.value

    def add_random_set_hybrid(self, level, q, S, nd, D=None, df=4.0, scale=None, varU0=100.0):
        """Random-effect set over K = S + embed(D) (single-step GBLUP's H^-1): S the sparse q x q part as add_random_set takes K (a CSR
        triple or a dense array sent as its nonzeros), D a dense block over the LAST nd levels: a symmetric nd x nd array (copied),
        (other_sampler, set_id) to share that hybrid set's block by reference, or None to take over this sampler's own corner block
        (grm_single_step).  Everything else as add_random_set; returns the set id."""
        lv = np.ascontiguousarray(level, dtype=np.int32)
        if scale is None:
            scale = varU0 * (df - 2.0) / df
        kp, kc, kv = k_csr(S)
        if len(kp) != int(q) + 1:
            raise ValueError("S: a q x q matrix or a CSR triple with q + 1 row pointers")
        Dh, src, src_set = None, None, 0
        if isinstance(D, tuple):
            src, src_set = D[0].h, int(D[1])
        elif D is not None:
            Dh = np.ascontiguousarray(D, dtype=np.float64)
            if Dh.shape != (int(nd), int(nd)):
                raise ValueError("D: an nd x nd matrix, (other_sampler, set_id) or None")
        sid = C.c_int32()
        self._chk(self.L.ngp_add_random_set_hybrid(self.h, _p(lv, C.c_int32), C.c_int64(int(q)), _p(kp, C.c_int64), _p(kc, C.c_int32),
                                                   _p(kv, C.c_double), C.c_int64(int(nd)), _p(Dh, C.c_double), src, C.c_int32(src_set),
                                                   C.c_double(df), C.c_double(scale), C.c_double(varU0), C.byref(sid)))
        self.rand_q = getattr(self, "rand_q", []) + [int(q)]
        return sid.value

    # ---- GBLUP: relationship matrix on the device ------------------------------------------
    def set_records(self, N):
        """N records and no genotype panel (a model without marker sets); in place of set_panel."""
        self._chk(self.L.ngp_set_records(self.h, C.c_int64(int(N))))
        self.N, self.P = int(N), 64  # (one inert block of zero columns stands in for the panel: include/nextgp_hip.h)

    def grm_begin(self, N, method=1):
        self._chk(self.L.ngp_grm_begin(self.h, C.c_int64(int(N)), C.c_int32(int(method))))
        self.grm_N = int(N)

    def grm_columns(self, M):
        """Raw (uncentred) genotype columns, N x ncol: uint8 and float32 are sent as they are, anything else as float64.  The first N
        rows of a taller Fortran-ordered array (M = big[:N]) go over without a copy, with the parent's leading dimension."""
        M = np.asarray(M)
        t = {np.dtype(np.uint8): C.c_uint8, np.dtype(np.float32): C.c_float}.get(M.dtype, C.c_double)
        if t is C.c_double and M.dtype != np.float64:
            M = np.asfortranarray(M, dtype=np.float64)
        if M.ndim != 2 or M.shape[0] != self.grm_N:
            raise ValueError("grm_columns: an N x ncol matrix")
        if not (M.strides[0] == M.itemsize and M.strides[1] % M.itemsize == 0 and M.strides[1] >= M.shape[0] * M.itemsize):
            M = np.asfortranarray(M)
        f = {C.c_uint8: self.L.ngp_grm_columns_u8, C.c_float: self.L.ngp_grm_columns_f32, C.c_double: self.L.ngp_grm_columns_f64}[t]
        self._chk(f(self.h, _p(M, t), C.c_int64(M.shape[1]), C.c_int64(max(M.strides[1] // M.itemsize, M.shape[0]))))

    def grm_end(self):
        self._chk(self.L.ngp_grm_end(self.h))

    def grm_get(self):
        out = np.empty((self.grm_N, self.grm_N))
        self._chk(self.L.ngp_grm_get(self.h, _p(out, C.c_double)))
        return out  # (symmetric: row- and column-major are the same matrix)

    def grm_invert(self):
        self._chk(self.L.ngp_grm_invert(self.h))

    def grm_single_step(self, A22, w=0.05):
        """After grm_end, in place of grm_invert: the matrix becomes D = inv((1 - w) G + w A22) - inv(A22), the dense corner of single-step
        GBLUP's H^-1 (grm_get returns it; add_random_set_hybrid(..., D=None) takes it over).  A22: the pedigree relationships of the
        genotyped animals in the row order of the genotypes (pedigree_a22)."""
        A = np.ascontiguousarray(A22, dtype=np.float64)
        if A.shape != (self.grm_N, self.grm_N):
            raise ValueError("grm_single_step: A22 is N x N over the genotyped animals")
        self._chk(self.L.ngp_grm_single_step(self.h, _p(A, C.c_double), C.c_int64(self.grm_N), C.c_double(float(w))))

    def get_random(self, set_id):
        q = self.rand_q[set_id]
        u = np.empty(q); su = np.empty(q); v, sv = C.c_double(), C.c_double()
        self._chk(self.L.ngp_get_random(self.h, C.c_int32(set_id), _p(u, C.c_double), _p(su, C.c_double), C.byref(v), C.byref(sv)))
        return dict(u=u, sum_u=su, varU=v.value, sum_varU=sv.value)

    def set_random(self, set_id, u=None, sum_u=None, varU=100.0, sum_varU=0.0):
        a = None if u is None else np.ascontiguousarray(u, dtype=np.float64)
        b = None if sum_u is None else np.ascontiguousarray(sum_u, dtype=np.float64)
        for x in (a, b):
            if x is not None and len(x) != self.rand_q[set_id]:
                raise ValueError("u / sum_u need q entries")
        self._chk(self.L.ngp_set_random(self.h, C.c_int32(set_id), _p(a, C.c_double), _p(b, C.c_double), C.c_double(varU), C.c_double(sum_varU)))

    def sample_random_set(self, set_id, varE, ycorr, u, varU):
        """Fine seam (sampleZ!): ycorr and u are updated in place; returns the new varU."""
        assert ycorr.dtype == np.float64 and u.dtype == np.float64 and len(ycorr) == self.N and len(u) == self.rand_q[set_id]
        vu = C.c_double(varU)
        self._chk(self.L.ngp_sample_random_set(self.h, C.c_int32(set_id), C.c_double(varE), _p(ycorr, C.c_double), _p(u, C.c_double), C.byref(vu)))
        return vu.value

    # ---- correlated (Tuple) random-effect sets: (ID, Dam), direct and maternal effects over one pedigree ----
    def add_random_set_tuple(self, levels, q, K=None, df=None, scale=None, varU0=None):
        """Correlated random-effect set (src/mme.jl:207-239): levels is k x N, one row per component, -1 for a record without a level in
        that component (an unknown dam); K the shared precision as for add_random_set; varU0 the k x k starting covariance (symmetric
        positive definite); df defaults to 3 + k and scale to varU0 (df - k - 1) (src/mme.jl:265-271).  u is q x k, varU k x k.  The
        step draws the exact Gibbs conditional, not the reference's lines (include/nextgp_hip.h).  Returns the set id."""
        lv = np.ascontiguousarray(np.atleast_2d(np.asarray(levels)), dtype=np.int32)
        k = lv.shape[0]
        if lv.ndim != 2 or not 1 <= k <= 4 or lv.shape[1] != self.N:
            raise ValueError("levels: k x N with k in 1..4")
        V = np.ascontiguousarray(np.asarray(varU0, dtype=np.float64).reshape(k, k))
        if df is None:
            df = 3.0 + k
        S = V * (df - k - 1.0) if scale is None else np.asarray(scale, dtype=np.float64).reshape(k, k)
        S = np.ascontiguousarray(S)
        kp, kc, kv = k_csr(K) if K is not None else (None, None, None)
        sid = C.c_int32()
        self._chk(self.L.ngp_add_random_set_tuple(self.h, _p(lv, C.c_int32), C.c_int32(k), C.c_int64(int(q)), _p(kp, C.c_int64), _p(kc, C.c_int32),
                                                  _p(kv, C.c_double), C.c_double(df), _p(S, C.c_double), _p(V, C.c_double), C.byref(sid)))
        self.rand_q = getattr(self, "rand_q", []) + [int(q)]
        self.rand_k = getattr(self, "rand_k", {})
        self.rand_k[sid.value] = k
        return sid.value

    def _rand_k(self, set_id):
        return getattr(self, "rand_k", {}).get(set_id, 1)

    def get_random_tuple(self, set_id):
        """dict(u [q, k], sum_u [q, k], varU [k, k], sum_varU [k, k]) of any random-effect set (k = 1 for a (1|g) set)."""
        q, k = self.rand_q[set_id], self._rand_k(set_id)
        u, su, v, sv = np.empty((q, k)), np.empty((q, k)), np.empty((k, k)), np.empty((k, k))
        self._chk(self.L.ngp_get_random_tuple(self.h, C.c_int32(set_id), _p(u, C.c_double), _p(su, C.c_double), _p(v, C.c_double), _p(sv, C.c_double)))
        return dict(u=u, sum_u=su, varU=v, sum_varU=sv)

    def set_random_tuple(self, set_id, u=None, sum_u=None, varU=None, sum_varU=None):
        """Restore parts of a set's state (None: left as it is); shapes as get_random_tuple returns them."""
        q, k = self.rand_q[set_id], self._rand_k(set_id)
        arr = lambda x, shape: None if x is None else np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(shape))
        a, b, v, sv = arr(u, (q, k)), arr(sum_u, (q, k)), arr(varU, (k, k)), arr(sum_varU, (k, k))
        self._chk(self.L.ngp_set_random_tuple(self.h, C.c_int32(set_id), _p(a, C.c_double), _p(b, C.c_double), _p(v, C.c_double), _p(sv, C.c_double)))

    def sample_random_set_tuple(self, set_id, varE, ycorr, u, varU):
        """Fine seam (sampleZ!(::Tuple) with the exact conditional): ycorr (N), u (q x k) and varU (k x k) are updated in place."""
        q, k = self.rand_q[set_id], self._rand_k(set_id)
        for x, n in ((ycorr, self.N), (u, q * k), (varU, k * k)):
            assert x.dtype == np.float64 and x.flags.c_contiguous and x.size == n
        self._chk(self.L.ngp_sample_random_set_tuple(self.h, C.c_int32(set_id), C.c_double(varE), _p(ycorr, C.c_double), _p(u, C.c_double), _p(varU, C.c_double)))

    def set_random_schedule(self, set_id, mode):
        """Gauss-Seidel engine of a CSR set with off-diagonal K: 0 / "auto", 1 / "serial", 2 / "scheduled" (the bits do not depend on it)."""
        mode = {"auto": 0, "serial": 1, "scheduled": 2}.get(mode, mode)
        self._chk(self.L.ngp_set_random_schedule(self.h, C.c_int32(set_id), C.c_int32(int(mode))))

    def get_random_schedule(self, set_id):
        """dict(engine: 0 none / 1 serial / 2 scheduled -- the one in force, depths, launches per step)."""
        e, d, n = C.c_int32(), C.c_int64(), C.c_int64()
        self._chk(self.L.ngp_get_random_schedule(self.h, C.c_int32(set_id), C.byref(e), C.byref(d), C.byref(n)))
        return dict(engine=e.value, depths=d.value, launches=n.value)

    def add_marker_set_r(self, col0, ncol, df, scale, varBeta0, vClass, pi, estPi=False, lhs0=None, rhs0=None):
        """BayesR set: class multipliers vClass of the set's single variance, class probabilities pi (src/mme.jl:374-383)."""
        vc = np.ascontiguousarray(vClass, dtype=np.float64); pp = np.ascontiguousarray(pi, dtype=np.float64)
        if len(vc) != len(pp):
            raise ValueError("vClass and pi need one entry per class")
        l0 = None if lhs0 is None else np.ascontiguousarray(lhs0, dtype=np.float64)
        r0 = None if rhs0 is None else np.ascontiguousarray(rhs0, dtype=np.float64)
        sid = C.c_int32()
        self._chk(self.L.ngp_add_marker_set_r(self.h, C.c_int64(col0), C.c_int64(ncol), C.c_double(df), C.c_double(scale), C.c_double(varBeta0),
                                              _p(vc, C.c_double), _p(pp, C.c_double), C.c_int32(len(vc)), C.c_int32(int(estPi)), _p(l0, C.c_double),
                                              _p(r0, C.c_double), C.byref(sid)))
        self.nsets += 1
        self.set_shapes.append((ncol, 1))
        self.nclasses = getattr(self, "nclasses", 0) + len(vc)
        return sid.value

    def add_marker_set_rc(self, col0, ncol, df, scale, varBeta0, vClass, pi, annot, estPi=False, lhs0=None, rhs0=None):
        """BayesRCpi set (annotation-informed BayesR, src/mme.jl:384-403): annot is ncol x A with entries 0 / 1, every locus with at least
        one annotation; K classes vClass with probabilities pi for every annotation; one variance per annotation (A K <= 16, A <= 8)."""
        vc = np.ascontiguousarray(vClass, dtype=np.float64); pp = np.ascontiguousarray(pi, dtype=np.float64)
        if len(vc) != len(pp):
            raise ValueError("vClass and pi need one entry per class")
        an = np.asarray(annot)
        an = an.reshape(ncol, -1)
        if not np.all(an == np.round(an)):
            raise ValueError("annot: entries 0 / 1")
        an = np.asfortranarray(an, dtype=np.int32)
        l0 = None if lhs0 is None else np.ascontiguousarray(lhs0, dtype=np.float64)
        r0 = None if rhs0 is None else np.ascontiguousarray(rhs0, dtype=np.float64)
        sid = C.c_int32()
        self._chk(self.L.ngp_add_marker_set_rc(self.h, C.c_int64(col0), C.c_int64(ncol), C.c_double(df), C.c_double(scale), C.c_double(varBeta0),
                                               _p(vc, C.c_double), _p(pp, C.c_double), C.c_int32(len(vc)), _p(an, C.c_int32), C.c_int64(ncol),
                                               C.c_int32(an.shape[1]), C.c_int32(int(estPi)), _p(l0, C.c_double), _p(r0, C.c_double), C.byref(sid)))
        self.nsets += 1
        self.set_shapes.append((ncol, an.shape[1]))
        self.nclasses = getattr(self, "nclasses", 0) + len(vc) * an.shape[1]
        self.rc_shape = dict(getattr(self, "rc_shape", {}))
        self.rc_shape[sid.value] = (ncol, an.shape[1], len(vc))
        return sid.value

    def rc_state(self, set_id):
        """dict(piHat[A, K], sum_pi[A, K], annotProb[ncol, A], annotCat[ncol] (from 1), sum_annot[ncol, A]) of a BayesRCpi set."""
        ncol, A, K = self.rc_shape[set_id]
        pi = np.empty(A * K); sp = np.empty(A * K); ap = np.empty((ncol, A), order="F"); sa = np.empty((ncol, A), order="F")
        cat = np.empty(ncol, dtype=np.int32)
        self._chk(self.L.ngp_get_rc_state(self.h, C.c_int32(set_id), _p(pi, C.c_double), _p(sp, C.c_double), _p(ap, C.c_double), _p(cat, C.c_int32),
                                          _p(sa, C.c_double)))
        return dict(piHat=pi.reshape(A, K), sum_pi=sp.reshape(A, K), annotProb=ap, annotCat=cat, sum_annot=sa)

    def set_rc_state(self, set_id, st):
        """Resume / fine seam: st as rc_state returns it; a missing key is left as it is on the device."""
        f = lambda k, order: None if st.get(k) is None else np.require(np.asarray(st[k], dtype=np.float64), requirements=[order])
        pi, sp, ap, sa = f("piHat", "C"), f("sum_pi", "C"), f("annotProb", "F"), f("sum_annot", "F")
        cat = None if st.get("annotCat") is None else np.ascontiguousarray(st["annotCat"], dtype=np.int32)
        self._chk(self.L.ngp_set_rc_state(self.h, C.c_int32(set_id), _p(pi, C.c_double), _p(sp, C.c_double), _p(ap, C.c_double), _p(cat, C.c_int32),
                                          _p(sa, C.c_double)))

    def add_marker_set_tuple(self, col0, nloc, k, df, scale, regions, varBeta0):
        """Correlated sets (BayesPR's Tuple method, src/functions.jl:140-154): k sets, nloc loci, columns as tuple_columns(col0, nloc, k);
        scale and varBeta0 k x k, regions ranges of loci."""
        rs = np.ascontiguousarray([r[0] for r in regions], dtype=np.int64)
        re = np.ascontiguousarray([r[1] for r in regions], dtype=np.int64)
        sc = np.ascontiguousarray(np.asarray(scale, dtype=np.float64).reshape(k, k)); vb = np.ascontiguousarray(np.asarray(varBeta0, dtype=np.float64).reshape(k, k))
        sid = C.c_int32()
        self._chk(self.L.ngp_add_marker_set_tuple(self.h, C.c_int64(col0), C.c_int64(nloc), C.c_int32(k), C.c_double(df), _p(sc, C.c_double),
                                                  _p(rs, C.c_int64), _p(re, C.c_int64), C.c_int64(len(rs)), _p(vb, C.c_double), C.byref(sid)))
        self.nsets += 1
        self.set_shapes.append((tuple_span(nloc, k), len(rs) * k * k))
        return sid.value

    def add_marker_set_lv(self, col0, ncol, varBeta0, covariates, varZeta0, est_mode=0, est_fraction=0.0, zeta0=None, lhs0=None, rhs0=None):
        """BayesLV set (src/runTime.jl:116-133): one variance per locus whose logarithm is regressed on the covariates (ncol x ncov,
        the design matrix of the variance formula).  est_mode 0: varZeta fixed; 1: var(zeta); 2: est_fraction * var(logVar).  zeta0: ncol
        starting values of zeta, None for keyed uniforms.  Returns the set id."""
        Cm = np.asfortranarray(np.asarray(covariates, dtype=np.float64).reshape(ncol, -1))
        z0 = None if zeta0 is None else np.ascontiguousarray(zeta0, dtype=np.float64)
        if z0 is not None and len(z0) != ncol:
            raise ValueError("zeta0 needs one entry per locus")
        l0 = None if lhs0 is None else np.ascontiguousarray(lhs0, dtype=np.float64)
        r0 = None if rhs0 is None else np.ascontiguousarray(rhs0, dtype=np.float64)
        sid = C.c_int32()
        self._chk(self.L.ngp_add_marker_set_lv(self.h, C.c_int64(col0), C.c_int64(ncol), C.c_double(varBeta0), _p(Cm, C.c_double), C.c_int64(ncol),
                                               C.c_int32(Cm.shape[1]), C.c_double(varZeta0), C.c_int32(int(est_mode)), C.c_double(est_fraction),
                                               _p(z0, C.c_double), _p(l0, C.c_double), _p(r0, C.c_double), C.byref(sid)))
        self.nsets += 1
        self.set_shapes.append((ncol, ncol))
        self.lv_shape = dict(getattr(self, "lv_shape", {}))
        self.lv_shape[sid.value] = (ncol, Cm.shape[1])
        return sid.value

    def lv_state(self, set_id):
        """dict(c[ncov], sum_c[ncov], varZeta, sum_varZeta, zeta[ncol], iCpC[ncov, ncov], trapped) of a BayesLV set."""
        ncol, ncov = self.lv_shape[set_id]
        c = np.empty(ncov); sc = np.empty(ncov); z = np.empty(ncol); ic = np.empty((ncov, ncov))
        vz, svz, tr = C.c_double(), C.c_double(), C.c_int64()
        self._chk(self.L.ngp_get_lv_state(self.h, C.c_int32(set_id), _p(c, C.c_double), _p(sc, C.c_double), C.byref(vz), C.byref(svz),
                                          _p(z, C.c_double), _p(ic, C.c_double), C.byref(tr)))
        return dict(c=c, sum_c=sc, varZeta=vz.value, sum_varZeta=svz.value, zeta=z, iCpC=ic, trapped=tr.value)

    def set_lv_state(self, set_id, st):
        """Resume: st as lv_state returns it (c, sum_c and zeta may be missing: left as they are)."""
        a = {k: (None if st.get(k) is None else np.ascontiguousarray(st[k], dtype=np.float64)) for k in ("c", "sum_c", "zeta")}
        self._chk(self.L.ngp_set_lv_state(self.h, C.c_int32(set_id), _p(a["c"], C.c_double), _p(a["sum_c"], C.c_double), C.c_double(st["varZeta"]),
                                          C.c_double(st.get("sum_varZeta", 0.0)), _p(a["zeta"], C.c_double)))

    def get_class_state(self, set_id):
        pi = np.empty(16); sp = np.empty(16); K = C.c_int64()
        self._chk(self.L.ngp_get_class_state(self.h, C.c_int32(set_id), _p(pi, C.c_double), _p(sp, C.c_double), C.byref(K)))
        return dict(piHat=pi[:K.value].copy(), sum_pi=sp[:K.value].copy())

    def set_class_state(self, set_id, piHat=None, sum_pi=None):
        a = None if piHat is None else np.ascontiguousarray(piHat, dtype=np.float64)
        b = None if sum_pi is None else np.ascontiguousarray(sum_pi, dtype=np.float64)
        K = len(a) if a is not None else len(b)
        self._chk(self.L.ngp_set_class_state(self.h, C.c_int32(set_id), _p(a, C.c_double), _p(b, C.c_double), C.c_int64(K)))

    def set_y(self, y):
        y = np.ascontiguousarray(y, dtype=np.float64)
        self._chk(self.L.ngp_set_y(self.h, _p(y, C.c_double), C.c_int64(len(y))))

    # ---- held-out records: missing phenotypes, cross-validation folds ---------------------
    def set_holdout(self, rows):
        """Hold out the records `rows` (0-based, strictly increasing, fewer than N): after the panel and before set_y, whose values on
        these rows are then not read (NaN is fine).  Every iteration redraws their phenotypes from their conditional; every kept
        iteration accumulates their fitted values (holdout()).  None or an empty list removes the mask."""
        r = np.ascontiguousarray([] if rows is None else rows, dtype=np.int64)
        if r.ndim != 1:
            raise ValueError("set_holdout: a list of rows")
        self._chk(self.L.ngp_set_holdout(self.h, _p(r, C.c_int64) if len(r) else None, C.c_int64(len(r))))

    def holdout_rows(self):
        m = C.c_int64()
        self._chk(self.L.ngp_get_holdout_layout(self.h, C.byref(m)))
        r = np.empty(m.value, dtype=np.int64)
        if m.value:
            self._chk(self.L.ngp_get_holdout(self.h, _p(r, C.c_int64), None, None, None, None, m, C.c_int64(self.N)))
        return r

    def holdout_state(self):
        """{"rows", "yaug" (m entries), "sum_fit", "sum_fit2", "n_fit" (N entries, zero off the rows)} of a chain with a mask."""
        m = C.c_int64()
        self._chk(self.L.ngp_get_holdout_layout(self.h, C.byref(m)))
        r = np.empty(m.value, dtype=np.int64); ya = np.empty(m.value)
        s1 = np.empty(self.N); s2 = np.empty(self.N); nf = np.empty(self.N)
        self._chk(self.L.ngp_get_holdout(self.h, _p(r, C.c_int64), _p(ya, C.c_double), _p(s1, C.c_double), _p(s2, C.c_double), _p(nf, C.c_double),
                                         m, C.c_int64(self.N)))
        return dict(rows=r, yaug=ya, sum_fit=s1, sum_fit2=s2, n_fit=nf)

    def set_holdout_state(self, hs):
        """Put back what holdout_state() gave (resume beside set_state / set_posterior_sums); a missing key leaves that array as it is."""
        a = {k: (None if hs.get(k) is None else np.ascontiguousarray(hs[k], dtype=np.float64)) for k in ("yaug", "sum_fit", "sum_fit2", "n_fit")}
        m = C.c_int64()
        self._chk(self.L.ngp_get_holdout_layout(self.h, C.byref(m)))
        for k, n in (("yaug", m.value), ("sum_fit", self.N), ("sum_fit2", self.N), ("n_fit", self.N)):
            if a[k] is not None and a[k].shape != (n,):
                raise ValueError(f"set_holdout_state: {k} must have {n} entries")
        self._chk(self.L.ngp_set_holdout_state(self.h, _p(a["yaug"], C.c_double), _p(a["sum_fit"], C.c_double), _p(a["sum_fit2"], C.c_double),
                                               _p(a["n_fit"], C.c_double), m, C.c_int64(self.N)))

    def holdout(self):
        """Posterior mean and SD of the fitted value (intercept, fixed, random and marker terms) of the records with hold-out sums:
        {"rows", "n", "mean", "sd"}; after allreduce_posterior over fold-chains, of every validated record."""
        return holdout_summary(self.holdout_state())

    # ---- liability traits: binary / ordered classes, censored records ---------------------
    def set_classes(self, cls, C_=None):
        """Threshold (probit) trait: cls[N] in 1..C, 2 <= C <= 8 (C defaults to the largest class).  After the panel and the hold-out
        mask, before set_y, which then reads y nowhere; entries of held-out rows are not read.  The residual variance is held at 1.
        None removes the classes."""
        if cls is None:
            self._chk(self.L.ngp_set_liability_classes(self.h, None, C.c_int32(0)))
            return
        c = check_classes(cls, self.N, C_)
        self._chk(self.L.ngp_set_liability_classes(self.h, _p(c, C.c_int32), C.c_int32(int(c.max()) if C_ is None else int(C_))))

    def set_censored(self, rows, lo, hi):
        """Censored (Tobit) records: the response of record rows[k] is only known to lie in (lo[k], hi[k]), lo < hi, one of them
        possibly infinite.  rows 0-based and strictly increasing, none held out; after the panel and the hold-out mask, before set_y,
        which reads y off these rows only.  rows=None removes the bounds."""
        if rows is None:
            self._chk(self.L.ngp_set_liability_bounds(self.h, None, None, None, C.c_int64(0)))
            return
        r, lo, hi = check_bounds(rows, lo, hi, self.N)
        self._chk(self.L.ngp_set_liability_bounds(self.h, _p(r, C.c_int64), _p(lo, C.c_double), _p(hi, C.c_double), C.c_int64(len(r))))

    def liability_layout(self):
        """(m, C): the augmented records (0 without liabilities) and the classes (0 for censored records)."""
        m = C.c_int64(); c = C.c_int32()
        self._chk(self.L.ngp_get_liability_layout(self.h, C.byref(m), C.byref(c)))
        return m.value, c.value

    def liability_state(self):
        """{"rows", "liab" (m entries), "thr", "sum_thr", "sum_thr2" (the C - 1 thresholds t_1 .. t_{C-1}, t_1 = 0, and their sums over
        kept iterations; empty for censored records)} of a chain with liabilities."""
        m, c = self.liability_layout()
        nt = max(c - 1, 0)
        r = np.empty(m, dtype=np.int64); l = np.empty(m)
        t = np.empty(nt); s1 = np.empty(nt); s2 = np.empty(nt)
        self._chk(self.L.ngp_get_liability(self.h, _p(r, C.c_int64), _p(l, C.c_double), _p(t, C.c_double), _p(s1, C.c_double), _p(s2, C.c_double),
                                           C.c_int64(m), C.c_int32(c)))
        return dict(rows=r, liab=l, thr=t, sum_thr=s1, sum_thr2=s2)

    def set_liability_state(self, ls):
        """Put back what liability_state() gave (resume beside set_state / set_posterior_sums); a missing key leaves that array as it is."""
        a = {k: (None if ls.get(k) is None else np.ascontiguousarray(ls[k], dtype=np.float64)) for k in ("liab", "thr", "sum_thr", "sum_thr2")}
        m, c = self.liability_layout()
        for k, n in (("liab", m), ("thr", max(c - 1, 0)), ("sum_thr", max(c - 1, 0)), ("sum_thr2", max(c - 1, 0))):
            if a[k] is not None and a[k].shape != (n,):
                raise ValueError(f"set_liability_state: {k} must have {n} entries")
        self._chk(self.L.ngp_set_liability_state(self.h, _p(a["liab"], C.c_double), _p(a["thr"], C.c_double), _p(a["sum_thr"], C.c_double),
                                                 _p(a["sum_thr2"], C.c_double), C.c_int64(m), C.c_int32(c)))

    def liability_fallthrough(self):
        """Truncated-normal draws of this handle whose rejection loop ran out of rounds (0 in any sane chain)."""
        n = C.c_int64()
        self._chk(self.L.ngp_get_liability_stats(self.h, C.byref(n)))
        return n.value

    # ---- ordered traits: Cowles' threshold step, class probabilities of held-out records ----
    def set_threshold_step(self, mode="cowles", sigma=0.0):
        """How the thresholds of C >= 3 classes move: "albert-chib" (the default of a handle: uniform between the liabilities of the
        two classes) or "cowles" (one joint Metropolis-Hastings move per iteration, decided on the fitted values alone; it mixes where
        a class holds many records).  sigma > 0 is a fixed proposal SD, 0 one that starts at 1 / sqrt(m) and follows the acceptance
        rate during burn-in.  After set_classes, before set_y."""
        if mode not in THRESHOLD_STEPS:
            raise ValueError(f"set_threshold_step: mode is one of {sorted(THRESHOLD_STEPS)}")
        self._chk(self.L.ngp_set_threshold_step(self.h, C.c_int32(THRESHOLD_STEPS[mode]), C.c_double(float(sigma))))

    def threshold_step(self):
        """{"mode" ("albert-chib" / "cowles"), "sigma" (the proposal SD in force, 0 under Albert-Chib), "tries", "accepted"}."""
        mode = C.c_int32(); sigma = C.c_double(); tries = C.c_int64(); acc = C.c_int64()
        self._chk(self.L.ngp_get_threshold_step(self.h, C.byref(mode), C.byref(sigma), C.byref(tries), C.byref(acc)))
        return dict(mode={v: k for k, v in THRESHOLD_STEPS.items()}[mode.value], sigma=sigma.value, tries=tries.value, accepted=acc.value)

    def set_threshold_step_state(self, ts):
        """Put back what threshold_step() gave (resume beside set_liability_state)."""
        self._chk(self.L.ngp_set_threshold_step_state(self.h, C.c_double(float(ts["sigma"])), C.c_int64(int(ts["tries"])), C.c_int64(int(ts["accepted"]))))

    def enable_class_probabilities(self, on=True):
        """Accumulate P(class) of every held-out record in every kept iteration (class_probabilities()).  Needs classes and a hold-out
        mask; before set_y."""
        self._chk(self.L.ngp_enable_class_probabilities(self.h, C.c_int32(int(bool(on)))))

    def class_probability_sums(self):
        """sum_prob[C][m]: the sums over kept draws as the library holds them (class-major, rows in the order of the hold-out set)."""
        m = C.c_int64()
        self._chk(self.L.ngp_get_holdout_layout(self.h, C.byref(m)))
        _, c = self.liability_layout()
        out = np.empty((c, m.value))
        self._chk(self.L.ngp_get_class_probabilities(self.h, _p(out, C.c_double), m, C.c_int32(c)))
        return out

    def set_class_probability_sums(self, sum_prob):
        """Put back what class_probability_sums() gave (resume beside set_holdout_state)."""
        a = np.ascontiguousarray(sum_prob, dtype=np.float64)
        self._chk(self.L.ngp_set_class_probabilities(self.h, _p(a, C.c_double), C.c_int64(a.shape[1]), C.c_int32(a.shape[0])))

    def class_probabilities(self):
        """{"rows", "n", "prob" (m x C)}: the posterior mean of P(class) of every held-out record with at least one kept draw; after
        allreduce_posterior over fold-chains that share one mask, of their pooled draws."""
        hs = self.holdout_state()
        n = hs["n_fit"][hs["rows"]]
        if not (n > 0).any():
            raise ValueError("no kept draw yet: the class probabilities are empty")
        sp = self.class_probability_sums()
        keep = n > 0
        return dict(rows=hs["rows"][keep], n=n[keep].astype(np.int64), prob=np.ascontiguousarray((sp[:, keep] / n[keep]).T))

    def debug_pnorm(self, which, a, b=None):
        """Test probe of the normal distribution function: which 0: Phi(a), 1: log(Phi(b) - Phi(a))."""
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = None if b is None else np.ascontiguousarray(b, dtype=np.float64)
        if b is not None and b.shape != a.shape:
            raise ValueError("debug_pnorm: a and b are vectors of one length")
        out = np.empty(len(a))
        self._chk(self.L.ngp_debug_pnorm(self.h, C.c_int32(int(which)), _p(a, C.c_double), _p(b, C.c_double), C.c_int64(len(a)), _p(out, C.c_double)))
        return out

    def fix_residual_variance(self, v):
        """v > 0 holds varE = v from set_y on (no draw; the trace reports v); 0 returns to sampling."""
        self._chk(self.L.ngp_fix_residual_variance(self.h, C.c_double(float(v))))

    def set_residual_prior(self, df, scale):
        self._chk(self.L.ngp_set_residual_prior(self.h, C.c_double(df), C.c_double(scale)))

    def set_intercept(self, on):
        self._chk(self.L.ngp_set_intercept(self.h, C.c_int32(int(on))))

    def set_residual_weights(self, w):
        """Weighted residuals (E.str == "D"): w = E.iVarStr = 1 ./ d, N entries, before the panel; None removes them."""
        if w is None:
            self._chk(self.L.ngp_set_residual_weights(self.h, None, C.c_int64(0)))
            return
        w = np.ascontiguousarray(w, dtype=np.float64)
        self._chk(self.L.ngp_set_residual_weights(self.h, _p(w, C.c_double), C.c_int64(len(w))))

    def residual_weights(self):
        """The weights set on this handle (or taken from the panel's owner), None when it has none."""
        n = getattr(self, "N", None)
        if n is None:
            return None
        out = np.zeros(n)
        rc = self.L.ngp_get_residual_weights(self.h, _p(out, C.c_double), C.c_int64(n))
        if rc == -2:
            return None
        self._chk(rc)
        return out

    def set_schedule(self, chainLength, burnIn, thin):
        self._chk(self.L.ngp_set_schedule(self.h, C.c_int64(chainLength), C.c_int64(burnIn), C.c_int64(thin)))

    # ---- run / read back ---------------------------------------------------------------
    def run(self, niter):
        self._chk(self.L.ngp_run(self.h, C.c_int64(niter)))

    @property
    def nvb(self):
        return sum(s[1] for s in self.set_shapes)

    def get_state(self):
        yc = np.empty(self.N); beta = np.empty(self.P); delta = np.empty(self.P, dtype=np.int64)
        vb = np.empty(max(self.nvb, 1)); pi = np.empty(2 * max(self.nsets, 1))
        varE, b, it = C.c_double(), C.c_double(), C.c_int64()
        self._chk(self.L.ngp_get_state(self.h, _p(yc, C.c_double), _p(beta, C.c_double), _p(delta, C.c_int64), _p(vb, C.c_double),
                                       _p(pi, C.c_double), C.byref(varE), C.byref(b), C.byref(it)))
        return dict(ycorr=yc, beta=beta, delta=delta, varBeta=vb[:self.nvb], piHat=pi[:2 * self.nsets], varE=varE.value,
                    b=b.value, iter=it.value)

    def set_state(self, st):
        yc = np.ascontiguousarray(st["ycorr"], dtype=np.float64); beta = np.ascontiguousarray(st["beta"], dtype=np.float64)
        delta = np.ascontiguousarray(st["delta"], dtype=np.int64); vb = np.ascontiguousarray(st["varBeta"], dtype=np.float64)
        pi = np.ascontiguousarray(st["piHat"], dtype=np.float64)
        self._chk(self.L.ngp_set_state(self.h, _p(yc, C.c_double), _p(beta, C.c_double), _p(delta, C.c_int64), _p(vb, C.c_double),
                                       _p(pi, C.c_double), C.c_double(st["varE"]), C.c_double(st["b"]), C.c_int64(st["iter"])))

    def get_trace(self, n):
        v = np.empty(n); b = np.empty(n)
        self._chk(self.L.ngp_get_trace(self.h, _p(v, C.c_double), _p(b, C.c_double), C.c_int64(n)))
        return dict(varE=v, b=b)

    def get_posterior_sums(self):
        sb = np.empty(self.P); sb2 = np.empty(self.P); sd = np.empty(self.P); sv = np.empty(max(self.nvb, 1))
        sp = np.empty(2 * max(self.nsets, 1)); se, sbb, nk = C.c_double(), C.c_double(), C.c_int64()
        self._chk(self.L.ngp_get_posterior_sums(self.h, _p(sb, C.c_double), _p(sb2, C.c_double), _p(sd, C.c_double),
                                                _p(sv, C.c_double), _p(sp, C.c_double), C.byref(se), C.byref(sbb), C.byref(nk)))
        return dict(sum_beta=sb, sum_beta2=sb2, sum_delta=sd, sum_varBeta=sv[:self.nvb], sum_pi=sp[:2 * self.nsets],
                    sum_varE=se.value, sum_b=sbb.value, nKept=nk.value)

    def posterior_len(self):
        n = C.c_int64()
        self._chk(self.L.ngp_posterior_len(self.h, C.byref(n)))
        return n.value

    def export_posterior_device(self, device_ptr, length):
        self._chk(self.L.ngp_export_posterior_device(self.h, C.c_void_p(device_ptr), C.c_int64(length)))

    def sweep_set(self, set_id, varE, ycorr, beta, varBeta, piHat=None):
        """Fine seam (M[set].funct): arrays are updated in place; returns delta."""
        assert ycorr.dtype == np.float64 and beta.dtype == np.float64 and varBeta.dtype == np.float64
        delta = np.empty(len(beta), dtype=np.int64)
        self._chk(self.L.ngp_sweep_set(self.h, C.c_int32(set_id), C.c_double(varE), _p(ycorr, C.c_double), _p(beta, C.c_double),
                                       _p(delta, C.c_int64), _p(varBeta, C.c_double), _p(piHat, C.c_double)))
        return delta

    def sweep_set_dev(self, set_id, varE, d_ycorr, d_beta, d_varBeta, d_delta=0, d_piHat=0):
        """The fine seam over DEVICE arrays (addresses, e.g. torch.Tensor.data_ptr(): ycorr N, beta ncol, varBeta nreg float64; delta
        ncol int64 or 0; piHat 2 float64 or 0), updated in place on the device."""
        self._chk(self.L.ngp_sweep_set_dev(self.h, C.c_int32(set_id), C.c_double(varE), C.c_void_p(d_ycorr), C.c_void_p(d_beta),
                                           C.c_void_p(d_delta or None), C.c_void_p(d_varBeta), C.c_void_p(d_piHat or None)))

    def get_timing(self):
        it = C.c_double()
        sl, ni = C.c_int64(), C.c_int64()
        self._chk(self.L.ngp_get_timing(self.h, C.byref(sl), C.byref(it), C.byref(ni)))
        return dict(sweep_launches=sl.value, iter_ms=it.value, iters=ni.value)

    def set_posterior_sums(self, ps):
        a = {k: np.ascontiguousarray(ps[k], dtype=np.float64) for k in ("sum_beta", "sum_beta2", "sum_delta", "sum_varBeta", "sum_pi")}
        self._chk(self.L.ngp_set_posterior_sums(self.h, _p(a["sum_beta"], C.c_double), _p(a["sum_beta2"], C.c_double),
                                                _p(a["sum_delta"], C.c_double), _p(a["sum_varBeta"], C.c_double), _p(a["sum_pi"], C.c_double),
                                                C.c_double(ps["sum_varE"]), C.c_double(ps["sum_b"]), C.c_int64(ps["nKept"])))

    def set_sample_file(self, path):
        """Every kept iteration of the following runs leaves a binary record in `path` without stopping the chain; None closes the file."""
        self._chk(self.L.ngp_set_sample_file(self.h, None if path is None else os.fsencode(path)))

    def save_snapshot(self, path):
        self._chk(self.L.ngp_save_snapshot(self.h, os.fsencode(path)))

    def load_snapshot(self, path):
        self._chk(self.L.ngp_load_snapshot(self.h, os.fsencode(path)))

    def set_trace_loci(self, loci, n_varBeta=0):
        loci = np.ascontiguousarray(loci, dtype=np.int64)
        self._chk(self.L.ngp_set_trace_loci(self.h, _p(loci, C.c_int64) if len(loci) else None, C.c_int64(len(loci)), C.c_int64(n_varBeta)))
        self.ntl, self.ntvb = len(loci), n_varBeta

    def get_trace_ext(self, n):
        bt = np.empty((n, max(self.ntl, 1))); vt = np.empty((n, max(self.ntvb, 1))); pt = np.empty((n, max(self.nsets, 1)))
        self._chk(self.L.ngp_get_trace_ext(self.h, _p(bt, C.c_double), _p(vt, C.c_double), _p(pt, C.c_double), C.c_int64(n)))
        return dict(beta=bt[:, :self.ntl], varBeta=vt[:, :self.ntvb], pi=pt[:, :self.nsets])

    def census(self):
        """Placement of the workgroups of the last persistent-sweep launch (ngp_get_census): dict(grid, retries, exclusive,
        xcc[grid] (0-7, -1 = never resident), hw_id[grid], direct[grid] (quads of that launch which wave 0 of a row-owning streamer
        loaded itself and fed to its GEMV chain; 0 where the loader brings every quad))."""
        g, r, e = C.c_int64(), C.c_int64(), C.c_int32()
        self._chk(self.L.ngp_get_census(self.h, None, C.c_int64(0), C.byref(g), C.byref(r), C.byref(e)))
        tb = np.zeros(g.value, dtype=np.uint64)
        self._chk(self.L.ngp_get_census(self.h, _p(tb, C.c_uint64), C.c_int64(g.value), None, None, None))
        return dict(grid=g.value, retries=r.value, exclusive=bool(e.value), xcc=((tb >> np.uint64(32)) & np.uint64(0xFF)).astype(np.int64) - 1,
                    hw_id=(tb & np.uint64(0xFFFFFFFF)).astype(np.int64), direct=(tb >> np.uint64(40)).astype(np.int64))

    def warmer(self):
        """The warmer of the last persistent-sweep launch (ngp_get_warmer): dict(active, blocks)."""
        a, b = C.c_int32(), C.c_int64()
        self._chk(self.L.ngp_get_warmer(self.h, C.byref(a), C.byref(b)))
        return dict(active=a.value, blocks=b.value)

    def debug_fail_census(self, iteration):
        self._chk(self.L.ngp_debug_fail_census(self.h, C.c_int64(iteration)))

    def debug_set_virtual_device(self, vdev):
        self._chk(self.L.ngp_debug_set_virtual_device(self.h, C.c_int32(vdev)))

    @staticmethod
    def allreduce_posterior(samplers):
        """Pooled posterior sums over the chains of `samplers` (ngp_allreduce_posterior): every sampler then holds them."""
        L = samplers[0].L
        arr = (C.c_void_p * len(samplers))(*[s.h for s in samplers])
        samplers[0]._chk(L.ngp_allreduce_posterior(arr, C.c_int32(len(samplers))))

    @staticmethod
    def run_many(samplers, niter):
        """niter iterations of every chain of `samplers` at once, one thread per chain inside the library (ngp_run_many)."""
        L = samplers[0].L
        arr = (C.c_void_p * len(samplers))(*[s.h for s in samplers])
        rc = L.ngp_run_many(arr, C.c_int32(len(samplers)), C.c_int64(niter))
        if rc != 0:
            msgs = [(s.L.ngp_last_error(s.h) or b"").decode() for s in samplers]
            raise NextGPHipError(f"libnextgp_hip error {rc}: " + " | ".join(m for m in msgs if m))

    def profile_iteration(self):
        ms, by = C.c_double(), C.c_double()
        n = C.c_int64()
        self._chk(self.L.ngp_profile_iteration(self.h, C.byref(ms), C.byref(n), C.byref(by)))
        return dict(avg_ms=ms.value, launches=n.value, bytes_per_launch=by.value)

    # ---- probes ------------------------------------------------------------------------
    def draws_indexed(self, it, kind, index0, what, n, p1=0.0, p2=0.0):
        out = np.empty(n)
        self._chk(self.L.ngp_draws_indexed(self.h, C.c_uint64(it), C.c_uint64(kind), C.c_uint64(index0), C.c_int32(what),
                                           C.c_double(p1), C.c_double(p2), C.c_int64(n), _p(out, C.c_double)))
        return out

    def tnormal_indexed(self, it, kind, index0, a, b):
        """Truncated standard normals: draw i on (a[i], b[i]) from stream (seed, chain, it, kind, index0 + i)."""
        a = np.ascontiguousarray(a, dtype=np.float64); b = np.ascontiguousarray(b, dtype=np.float64)
        if a.shape != b.shape or a.ndim != 1:
            raise ValueError("tnormal_indexed: a and b are vectors of one length")
        out = np.empty(len(a))
        self._chk(self.L.ngp_tnormal_indexed(self.h, C.c_uint64(it), C.c_uint64(kind), C.c_uint64(index0), _p(a, C.c_double), _p(b, C.c_double),
                                             C.c_int64(len(a)), _p(out, C.c_double)))
        return out

    def eval_math(self, which, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        out = np.empty(len(x))
        self._chk(self.L.ngp_eval_math(self.h, C.c_int32(which), _p(x, C.c_double), C.c_int64(len(x)), _p(out, C.c_double)))
        return out
