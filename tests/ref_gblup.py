"""GBLUP (TEST INFRASTRUCTURE): numpy restatements written from the reference's formulas and from DESIGN.md section 2, "Dense
random-effect sets and the GRM" -- not from the HIP code, and with no reference program text.

    /root/reference/src/misc.jl:145-160        makeG: VanRaden's G, method 1 / 2, + 0.001 I
    /root/reference/src/prepMatVec.jl:122-126  a SNP term under a Random("G", v) prior: iVarStr = inv(makeG(M)), Z = I
    /root/reference/src/functions.jl:57-72     sampleU: Gauss-Seidel over iVarStr (reference order: ref_random.RandomRefChain)

make_g is plain fp64 numpy in the reference's order of operations.  dense_step_blocked is the device's documented order of ONE step
of a dense random-effect set, operation by operation (no FMA anywhere: every product and every sum is one IEEE double operation, which
is what numpy's elementwise arithmetic gives): bit for bit what ngp_sample_random_set computes for a set added with
ngp_add_random_set_dense.  Draws come from oracle.draws on kinds 12 / 13 exactly as ref_random.random_step_blocked takes them: a dense set
and a CSR set with the same id consume the same random numbers.
"""
import numpy as np

from ref_random import KIND_U_CHI2, KIND_U_NORMAL, draw, level_records


def make_g(M, method=1, ridge=0.001):
    """G of src/misc.jl:145-160 from raw genotypes M (N x P): p = colmean / 2, centre; method 1: M M' / sum(2 p q); method 2: columns
    divided by sqrt(2 p q), M M' / P; then + 0.001 I.  Returns (G, |Xc| |Xc|' / denom) -- the second is the scale of the forward-error
    bound of the product."""
    M = np.array(M, dtype=np.float64)
    mean = M.mean(axis=0)
    p = mean / 2.0
    q = 1.0 - p
    Xc = M - mean
    if method == 1:
        denom = float(np.sum(2.0 * p * q))
    elif method == 2:
        Xc = Xc / np.sqrt(2.0 * p * q)
        denom = float(M.shape[1])
    else:
        raise ValueError("enter a valid method")
    G = (Xc @ Xc.T) / denom
    G = G + ridge * np.eye(M.shape[0])
    return G, (np.abs(Xc) @ np.abs(Xc).T) / denom


def hw_genotypes(O, N, P, seed=20250509):
    """Allele counts 0 / 1 / 2 in Hardy-Weinberg proportions from the project's generator (the panel it returns is centred: the column
    means go back on)."""
    X, mu = O.generate_panel(N, P, seed=seed)
    return np.rint(X.astype(np.float64) + mu).astype(np.uint8)


def _fold(v):
    """The butterfly acc = acc + shfl_xor(acc, off), off = 32 .. 1, of 64 lanes (last axis), lane 0's value: halving the vector, the
    upper half added to the lower one, is the same additions in the same pairing."""
    n = 64
    while n > 1:
        n //= 2
        v = v[..., :n] + v[..., n:2 * n]
    return v[..., 0]


def dense_step_blocked(O, seed, chain, it, rset, yt, rs, level, q, K, zpz, u, varU, varE, df, scale):
    """One step of a dense random-effect set in the device's order (k_rand_levels, k_dense_dhi, k_dense_block for every block of 64
    levels, k_rand_update, k_dense_var).  yt: the device's residual (y~ = s ycorr under weights, rs = s; else ycorr, rs None).
    level None: the identity incidence.  Returns (yt, u, varU) as new arrays / a float; inputs are not changed."""
    K = np.asarray(K, dtype=np.float64)
    yt = np.array(yt, dtype=np.float64)
    u = np.array(u, dtype=np.float64)
    zpz = np.asarray(zpz, dtype=np.float64)
    N = len(yt)
    level = np.arange(N) if level is None else np.asarray(level, dtype=np.int64)
    iVarE = 1.0 / varE
    iVarU = 1.0 / varU
    # level sums: lane j of a level's wave adds the level's records j, j + 64, ... (ascending record order), then the butterfly
    term = yt * np.asarray(rs, dtype=np.float64) if rs is not None else yt
    lanes = np.zeros((q, 64))
    for l, recs in enumerate(level_records(level, q)):
        for k, i in enumerate(recs):
            lanes[l, k % 64] = lanes[l, k % 64] + term[i]
    acc = _fold(lanes)
    tu = zpz * u
    tot = acc + tu
    Yi = tot * iVarE
    kd = np.diag(K).copy()
    lhs = zpz * iVarE + kd * iVarU
    inv = 1.0 / lhs
    z = O.draws(seed, chain, it, KIND_U_NORMAL, (rset << 40), 1, q, 0.0, 0.0, indexed=True)
    tz = np.sqrt(inv) * z
    # dhi_l = sum over c > l of K_lc u_c (old u): lane j adds the columns 64 m + j, m ascending, then the butterfly
    nb = (q + 63) // 64
    prod = np.zeros((q, nb * 64))
    prod[:, :q] = np.triu(K, 1) * u[None, :]
    lane = np.zeros((q, 64))
    for m in range(nb):
        lane = lane + prod[:, 64 * m:64 * m + 64]      # (adding + 0.0 where a lane has no column changes nothing)
    dhi = _fold(lane)
    # blocks of 64 levels: the 64-step chain of the block, then acc of the rows below it += butterfly(K[r, block] * u_new[block])
    accd = np.zeros(q)
    dlo = np.zeros(q)
    un = u.copy()
    for t in range(nb):
        b0, b1 = 64 * t, min(64 * t + 64, q)
        d = accd[b0:b1].copy()
        for s in range(b1 - b0):
            l = b0 + s
            dd = d[s] + dhi[l]
            tt = dd * iVarU
            rhs = Yi[l] - tt
            mean = inv[l] * rhs
            un[l] = mean + tz[l]
            d[s + 1:] = d[s + 1:] + K[b0 + s + 1:b1, l] * un[l]
        dlo[b0:b1] = d
        if b1 < q:
            accd[b1:] = accd[b1:] + _fold(K[b1:, b0:b1] * un[None, b0:b1])
    du = un - u
    t = du[level]
    if rs is not None:
        t = np.asarray(rs, dtype=np.float64) * t
    yt = yt - t
    # u'Ku = sum_l u_l (K_ll u_l + 2 dlo_l): thread l % 1024 adds its levels in ascending order, butterfly per wave, 16 wave sums in order
    p = un * (kd * un + 2.0 * dlo)
    thr = np.zeros(1024)
    for l0 in range(0, q, 1024):
        seg = p[l0:l0 + 1024]
        thr[:len(seg)] = thr[:len(seg)] + seg
    waves = _fold(thr.reshape(16, 64))
    quad = waves[0]
    for w in range(1, 16):
        quad = quad + waves[w]
    chi = draw(O, seed, chain, it, KIND_U_CHI2, rset, 2, df + q)
    tt = scale * df
    tt = tt + quad
    return yt, un, float(tt / chi)
