"""Prediction of new individuals (TEST INFRASTRUCTURE): the normative arithmetic of DESIGN.md section 2, "Prediction", restated in
numpy operation by operation -- written from that section, not from the HIP code.

    chunk c of set s   the panel's 64-column blocks [tb0 + 32 c, tb0 + 32 (c + 1)), tb0 = col0 // 64, cut to the set's columns
    inside a chunk     acc = fma((double) x_ij, beta_j, acc), j ascending, from 0.0
    g_s(i)             the chunk sums added in ascending c, from 0.0
    byte tiles         the code sums as above, sum_j m_j beta_j formed the same way (chains per chunk, chunk sums added), subtracted once
    g(i)               the g_s(i) added in set order, from 0.0
    sums               sum[s] += g_s, sum2[s] += g_s * g_s (a product, then an addition), row nsets: g

The fused multiply-add is ref_random_tuple.fma (one rounding, exact).  fma_vec is that function over arrays: where two error-free
transformations PROVE the single rounding it is computed in numpy, and every other element goes through the scalar function.
"""
import numpy as np

from ref_random_tuple import fma

BLK = 64
CHUNK_BLOCKS = 32


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def fma_vec(a, b, c):
    """fma(a[i], b, c[i]) for arrays a, c and a scalar b.  a b = p + e exactly (Dekker), p + c = s + t exactly (Knuth); when t + e is
    exact too (u, checked by a third transformation), a b + c = s + u with s and u doubles and s + u rounds it once.  Elements where
    that is not proven, or whose magnitudes leave the range in which the splits are exact, take the scalar fma."""
    a = np.asarray(a, dtype=np.float64)
    c = np.asarray(c, dtype=np.float64)
    b = float(b)
    with np.errstate(all="ignore"):
        p = a * b
        t = 134217729.0 * a
        ah = t - (t - a)
        al = a - ah
        tb = 134217729.0 * b
        bh = tb - (tb - b)
        bl = b - bh
        e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
        s, t2 = _two_sum(p, c)
        u, uerr = _two_sum(t2, e)
        out = s + u
        proven = (uerr == 0.0) & (((np.abs(p) > 1e-140) & (np.abs(p) < 1e140)) | (a == 0.0) | (b == 0.0)) & (np.abs(c) < 1e290) & np.isfinite(out)
    if not proven.all():
        for i in np.flatnonzero(~proven):
            out[i] = fma(float(a[i]), b, float(c[i]))
    return out


def chunks(col0, ncol):
    """[j0, j1) of every chunk of the set on columns [col0, col0 + ncol), ascending."""
    tb0, tb1 = col0 // BLK, (col0 + ncol + BLK - 1) // BLK
    return [(max(col0, t * BLK), min(col0 + ncol, (t + CHUNK_BLOCKS) * BLK)) for t in range(tb0, tb1, CHUNK_BLOCKS)]


def stored_f32(V, mu):
    """fp32 storage: the values the prediction tiles hold, x_ij = (float)((double) v_ij - mu_j), as Float64."""
    return (np.asarray(V, dtype=np.float64) - np.asarray(mu, dtype=np.float64)[None, :]).astype(np.float32).astype(np.float64)


def predict_draw(X, beta, sets, mean=None):
    """g of one draw: [nsets + 1][Np], the last row all sets together.  X: the stored values (Np x P; fp32 storage: stored_f32, byte
    tiles: the codes), sets: (col0, ncol) of every marker set in set order (a Tuple set: its column span), mean: the column means the
    byte tiles are centred with (None: fp32 storage)."""
    X = np.asarray(X, dtype=np.float64)
    Np = X.shape[0]
    G = np.zeros((len(sets) + 1, Np))
    tot = np.zeros(Np)
    for s, (col0, ncol) in enumerate(sets):
        g = np.zeros(Np)
        gm = 0.0
        for j0, j1 in chunks(col0, ncol):
            acc = np.zeros(Np)
            for j in range(j0, j1):
                acc = fma_vec(X[:, j], beta[j], acc)
            g = g + acc
            if mean is not None:
                am = 0.0
                for j in range(j0, j1):
                    am = fma(float(mean[j]), float(beta[j]), am)
                gm = gm + am
        if mean is not None:
            g = g - gm
        G[s] = g
        tot = tot + g
    G[len(sets)] = tot
    return G


def accumulate(sum1, sum2, G):
    """One kept draw into the sums (in place)."""
    sum1 += G
    sum2 += G * G


def bound(X, beta, sets, mean=None):
    """|g_s(i) - exact| <= (n_cols + 2) 2^-53 sum_j |x_ij| |beta_j| per set (n_cols: the set's columns), and for the last row the same
    with every owned column and the additions of the sets counted: a sum of n products, in any order and with any fusing, rounds each
    product's path at most n times by a relative 2^-53 (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1).  Byte
    tiles (mean given): the code sum and the mean term are two such sums and one subtraction, so |x_ij| is |g_ij| + |m_j| there."""
    X = np.abs(np.asarray(X, dtype=np.float64))
    if mean is not None:
        X = X + np.abs(np.asarray(mean, dtype=np.float64))[None, :]
    u = 2.0 ** -53
    B = np.zeros((len(sets) + 1, X.shape[0]))
    A = np.zeros(X.shape[0])
    ntot = 0
    for s, (col0, ncol) in enumerate(sets):
        a = X[:, col0:col0 + ncol] @ np.abs(beta[col0:col0 + ncol])
        B[s] = (ncol + 2 + (2 if mean is not None else 0)) * u * a
        A += a
        ntot += ncol
    B[len(sets)] = (ntot + len(sets) + 2 + (2 if mean is not None else 0)) * u * A
    return B
