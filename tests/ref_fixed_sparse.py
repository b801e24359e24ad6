"""Sparse fixed-effect sets (TEST INFRASTRUCTURE): a restatement of ONE step of a set given as a sparse matrix, written from DESIGN.md
section 2, "Sparse fixed-effect sets" (and so from the dense step it must reproduce: sampleb!, src/functions.jl:22-36; X'X + ridge,
src/mme.jl:149-152), not from the HIP code.  Plain Python loops, every operation one IEEE double operation or one fused multiply-add
(ref_random_tuple.fma).  Draws come from oracle.draws on kind FIXED_NORMAL with the key (set + 1) << 20 | column.

Builders (the host set-up of ngp_add_fixed_set_sparse):
    csr_of_csc   per record its (column, value) pairs, columns ascending
    xpx_rows     X'X by rows, columns ascending; entry (a, c) fma-accumulated over the records in ascending order from 0.0
    ridge_diag   X'X[a][a] + min_a |X'X[a][a]| / 10000
    depths       depth(a) = 1 + max depth(c) over the stored c < a of row a, or 0 if there is none
sparse_step      (ycorr, b, varE) -> (b', ycorr')
"""
import math

import numpy as np

from ref_random import _butterfly, draw
from ref_random_tuple import fma

KIND_FIXED_NORMAL = 2


def csr_of_csc(N, ncol, cp, row, val):
    recs = [[] for _ in range(N)]
    for a in range(ncol):                                   # columns ascending: every record's columns come out ascending
        for k in range(int(cp[a]), int(cp[a + 1])):
            recs[int(row[k])].append((a, float(val[k])))
    return recs


def xpx_rows(N, ncol, cp, row, val):
    recs = csr_of_csc(N, ncol, cp, row, val)
    lower = []
    for a in range(ncol):
        w = {}
        for k in range(int(cp[a]), int(cp[a + 1])):         # the records of column a, ascending
            xa = float(val[k])
            for c, xc in recs[int(row[k])]:
                if c > a:
                    break
                w[c] = fma(xa, xc, w.get(c, 0.0))
        lower.append(sorted(w.items()))
    rows = [list(r) for r in lower]                         # row r: its entries c <= r, then (r, a) = (a, r) of the rows a > r, a ascending
    for a in range(ncol):
        for c, v in lower[a]:
            if c != a:
                rows[c].append((a, v))
    return rows


def ridge_diag(rows):
    diag = [[v for c, v in r if c == a][0] for a, r in enumerate(rows)]
    mn = abs(diag[0])
    for d in diag[1:]:
        mn = min(mn, abs(d))
    return [d + mn / 10000.0 for d in diag]


def depths(rows):
    dep = []
    for a, r in enumerate(rows):
        d = 0
        for c, _ in r:
            if c < a:
                d = max(d, dep[c] + 1)
        dep.append(d)
    return dep


def sparse_step(O, seed, chain, it, fset, N, ncol, cp, row, val, ycorr, b, varE, built=None):
    """One step of the set in the device's order.  ycorr: the device's residual (y~ = s ycorr under weights, val then s_i val).
    built: (recs, rows, diagR) of the builders, to form them once for several steps.  Inputs are not changed."""
    y = [float(x) for x in ycorr]
    b = [float(x) for x in b]
    recs, rows, diagR = built if built is not None else (csr_of_csc(N, ncol, cp, row, val), xpx_rows(N, ncol, cp, row, val), None)
    if diagR is None:
        diagR = ridge_diag(rows)
    iVarE = 1.0 / varE
    Yi = [0.0] * ncol
    for a in range(ncol):
        acc = [0.0] * 1024                                  # accumulator t: the records t, t + 1024, ... of the column, ascending
        for k in range(int(cp[a]), int(cp[a + 1])):
            i = int(row[k])
            acc[i % 1024] = fma(float(val[k]), y[i], acc[i % 1024])
        d = 0.0
        for w in range(16):
            s = _butterfly(acc[64 * w:64 * w + 64])
            d = s if w == 0 else d + s
        xb = 0.0
        for c, v in rows[a]:
            xb = fma(v, b[c], xb)
        tot = d + xb
        Yi[a] = tot * iVarE
    bold, bnew = list(b), list(b)
    for a in range(ncol):                                   # column order IS the level schedule's result: c < a new, c > a old
        d = 0.0
        for c, v in rows[a]:
            if c == a:
                continue
            d = fma(v, bnew[c] if c < a else bold[c], d)
        t1 = d * iVarE
        rhsb = Yi[a] - t1
        lhsb = diagR[a] * iVarE
        inv = 1.0 / lhsb
        meanb = inv * rhsb
        z = draw(O, seed, chain, it, KIND_FIXED_NORMAL, ((fset + 1) << 20) | a, 1)
        sd = math.sqrt(inv)
        tz = sd * z
        bnew[a] = meanb + tz
    db = [bnew[a] - bold[a] for a in range(ncol)]
    for i in range(N):
        t = 0.0
        for a, x in recs[i]:
            t = fma(x, db[a], t)
        y[i] = y[i] - t
    return np.array(bnew), np.array(y)


def dense_of_csc(N, ncol, cp, row, val):
    X = np.zeros((N, ncol))
    for a in range(ncol):
        for k in range(int(cp[a]), int(cp[a + 1])):
            X[int(row[k]), a] = val[k]
    return X
