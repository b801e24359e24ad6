"""Genomic variance per kept draw (TEST INFRASTRUCTURE): the normative arithmetic of DESIGN.md section 2, "Genomic variance", restated
in numpy and Python integers step by step -- written from that section, not from the HIP code.

    segments of a set  its windows and the gaps between and around them, ascending; a gap cut into pieces of 2048 columns from its start
    inside a segment   acc = fma((double) x_ij, beta_j, acc), j ascending, from 0.0; byte tiles: minus am = fma(m_j, beta_j, am), once
    items              whole segments, greedily, while first-to-last column stays <= 2048; item value = its segments added in order
    g_s(i), g(i)       the item values added in ascending order from 0.0; the sets added in set order from 0.0
    E of a slot        ex + ilog(sum |beta_j|) + 1 (clamped to +-400), ex = ilog(max |x_ij| over the live rows; byte tiles: |code - m_j|)
    integer sums       Q1 = sum_i rint(g 2^(45 - E)), Q2 = sum_i rint((g g) 2^(46 - 2E))
    V                  S1 = (double) Q1 2^(E - 45), S2 = (double) Q2 2^(2E - 46); max(0, (S2 - (S1 S1) / N) / (N - 1))

The fused multiply-add is ref_random_tuple.fma (through ref_predict.fma_vec); stored_f32 is ref_predict's.
"""
import math
from fractions import Fraction

import numpy as np

from ref_predict import fma_vec, stored_f32  # noqa: F401  (stored_f32: what the fp32 tiles hold)
from ref_random_tuple import fma

IC = 2048
EMAX = 400


def segments(col0, ncol, windows):
    """[(j0, j1, window index or -1)] of the set on panel columns [col0, col0 + ncol): step 1."""
    out = []

    def gap(a, b):
        for j in range(a, b, IC):
            out.append((col0 + j, col0 + min(j + IC, b), -1))

    at = 0
    for k, (a, b) in enumerate(windows):
        gap(at, a)
        out.append((col0 + a, col0 + b, k))
        at = b
    gap(at, ncol)
    return out


def items(segs):
    """Runs of whole segments (lists of indices into segs): step 4."""
    out, e = [], 0
    while e < len(segs):
        f = e + 1
        while f < len(segs) and segs[f][1] - segs[e][0] <= IC:
            f += 1
        out.append(list(range(e, f)))
        e = f
    return out


def ilog(x):
    """Smallest k with |x| < 2^k for a normal x; -1022 for zero and subnormals: step 8."""
    x = abs(float(x))
    if not math.isfinite(x):
        return 4000
    if x < 2.0 ** -1022:
        return -1022
    return math.frexp(x)[1]


def xmax(X, mean=None):
    """The largest |x_ij| of the stored values of the live rows (byte tiles: |code_ij - m_j|): step 8."""
    X = np.asarray(X, dtype=np.float64)
    return float(np.abs(X if mean is None else X - np.asarray(mean, dtype=np.float64)[None, :]).max())


def xexp(x_max):
    return ilog(x_max)


def exponent(ex, a):
    return max(-EMAX, min(EMAX, ex + ilog(a) + 1))


def variance_fx(g, E, N):
    """Steps 9-11 for the values g of the N live rows."""
    g = np.asarray(g, dtype=np.float64)
    t1 = np.rint(g * 2.0 ** (45 - E))
    t2 = np.rint((g * g) * 2.0 ** (46 - 2 * E))
    assert np.all(np.abs(t1) <= 2.0 ** 44) and np.all(t2 <= 2.0 ** 44)
    Q1 = sum(int(v) for v in t1)
    Q2 = sum(int(v) for v in t2)
    S1 = float(Q1) * 2.0 ** (E - 45)
    S2 = float(Q2) * 2.0 ** (2 * E - 46)
    t = S1 * S1
    t = t / float(N)
    d = S2 - t
    v = d / float(N - 1)
    return v if v > 0.0 else 0.0


def rows(X, beta, sets, windows, mean=None):
    """Steps 1-7: (gw [nwin][N], gs [nsets + 1][N], a [nslots]) -- the per-row values of every window, set and the total, and sum |beta|
    of every slot.  X: the stored values of the N live rows (N x P; byte tiles: the codes, mean: their column means)."""
    X = np.asarray(X, dtype=np.float64)
    N = X.shape[0]
    gw, aw, gs, as_ = [], [], [], []
    tot, atot = np.zeros(N), 0.0
    for (col0, ncol), wins in zip(sets, windows):
        segs = segments(col0, ncol, wins)
        vals, sa = [], []
        for j0, j1, k in segs:
            acc = np.zeros(N)
            am, a = 0.0, 0.0
            for j in range(j0, j1):
                acc = fma_vec(X[:, j], beta[j], acc)
                if mean is not None:
                    am = fma(float(mean[j]), float(beta[j]), am)
                a = a + abs(float(beta[j]))
            v = acc - am if mean is not None else acc
            vals.append(v); sa.append(a)
            if k >= 0:
                gw.append(v); aw.append(a)
        g = np.zeros(N)
        for it in items(segs):
            iv = np.zeros(N)
            for e in it:
                iv = iv + vals[e]
            g = g + iv
        a = 0.0
        for x in sa:
            a = a + x
        gs.append(g); as_.append(a)
        tot = tot + g
        atot = atot + a
    gs.append(tot); as_.append(atot)
    return gw, gs, np.array(aw + as_)


def draw(X, beta, sets, windows, mean=None):
    """V of every slot for one draw (steps 1-11) and the slot exponents."""
    gw, gs, a = rows(X, beta, sets, windows, mean)
    N = np.asarray(X).shape[0]
    ex = xexp(xmax(X, mean))
    E = [exponent(ex, x) for x in a]
    V = np.array([variance_fx(g, e, N) for g, e in zip(gw + gs, E)])
    return V, E


class Sums:
    """Step 12 over the kept draws."""

    def __init__(self, nslots, threshold, trace_rows=0):
        self.a = np.zeros((6, nslots)); self.ratio = np.zeros(2); self.n = 0
        self.thr, self.cap, self.trV, self.trR = threshold, trace_rows, [], []

    def add(self, V, varE):
        Vg = V[-1]
        q = V / Vg if Vg > 0.0 else np.zeros_like(V)
        den = Vg + varE
        r = Vg / den if den > 0.0 else 0.0
        self.a[0] += V; self.a[1] += V * V; self.a[2] += q; self.a[3] += q * q; self.a[4] += (q > self.thr); self.a[5] = V
        self.ratio[0] += r; self.ratio[1] += r * r
        if self.n < self.cap:
            self.trV.append(V.copy()); self.trR.append(r)
        self.n += 1
        return q, r


def exact_variance(X, beta, cols, mean=None):
    """var_i sum_{j in cols} (x_ij - m_j) beta_j with N - 1, in rational arithmetic."""
    N = X.shape[0]
    g = []
    for i in range(N):
        s = Fraction(0)
        for j in cols:
            x = Fraction(float(X[i, j])) - (Fraction(float(mean[j])) if mean is not None else 0)
            s += x * Fraction(float(beta[j]))
        g.append(s)
    S1 = sum(g); S2 = sum(v * v for v in g)
    return (S2 - S1 * S1 / N) / (N - 1)


def bound(X, beta, cols, E, V, mean=None):
    """|V - exact| of a slot over the columns cols with exponent E ("Error of V"): the fixed-point terms, the fp64 error of
    every row's sum (Higham section 3.1: n + 4 roundings cover any order, the mean term and its subtraction) and the final operations."""
    X = np.abs(np.asarray(X, dtype=np.float64)[:, cols])
    if mean is not None:
        X = X + np.abs(np.asarray(mean, dtype=np.float64)[cols])[None, :]
    N = X.shape[0]
    u = 2.0 ** -53
    G = 2.0 ** (E - 1)
    delta = (len(cols) + 4) * u * (X @ np.abs(np.asarray(beta)[cols]))
    d1 = N * 2.0 ** (E - 46) + delta.sum() + u * N * G
    d2 = N * 2.0 ** (2 * E - 47) + (2 * G * delta + delta * delta).sum() + 2 * u * N * G * G
    return (d2 + 2 * G * d1 + d1 * d1 / N + 4 * u * N * G * G) / (N - 1) + 4 * u * V
