"""Pedigree BLUP (TEST INFRASTRUCTURE): the test pedigrees, and a restatement of the level schedule of a CSR random-effect set written
from DESIGN.md ("Random-effect sets", the schedule), not from the HIP code.

    depth(l) = 0 for a row of K without an entry left of its diagonal, else 1 + max depth(c) over its columns c < l
    order    = the rows sorted by (depth, l);  dptr[d] .. dptr[d + 1] = the rows of depth d
    plan     = a depth of more than 1024 rows is a launch of its own ("wide"), a run of consecutive narrower depths ONE launch ("fused")

random_step_scheduled is ref_random.random_step_blocked with the Gauss-Seidel walked depth by depth: every row of a depth reads u as it
was when the depth began (the rows of a depth run side by side on the device, in no defined order), so equality with the serial walk,
bit for bit, is the argument that the reordering is exact.  Rows are lists of (column, value), columns ascending (ref_random.csr_of).
"""
import math

import numpy as np

import ref_random as RR

FUSE_ROWS = 1024

# the 14 animals of docs/src/PBLUP/PBLUP.md, and its phenotypes (ID, Sire, Dam, Herds, Pen, BW)
PBLUP_PED = [("QGG1", "0", "0"), ("QGG2", "0", "0"), ("QGG3", "0", "0"), ("QGG4", "0", "0"), ("QGG5", "QGG1", "QGG2"),
             ("QGG6", "QGG3", "QGG2"), ("QGG7", "QGG4", "QGG6"), ("QGG8", "QGG3", "QGG5"), ("QGG9", "QGG1", "QGG6"),
             ("QGG10", "QGG3", "QGG2"), ("QGG11", "QGG3", "QGG7"), ("QGG12", "QGG8", "QGG7"), ("QGG13", "QGG9", "QGG2"),
             ("QGG14", "QGG3", "QGG6")]
PBLUP_DATA = [("QGG5", "QGG1", "QGG2", 1, 1, 35.0), ("QGG6", "QGG3", "QGG2", 1, 2, 20.0), ("QGG7", "QGG4", "QGG6", 1, 2, 25.0),
              ("QGG8", "QGG3", "QGG5", 1, 1, 40.0), ("QGG9", "QGG1", "QGG6", 2, 1, 42.0), ("QGG10", "QGG3", "QGG2", 2, 2, 22.0),
              ("QGG11", "QGG3", "QGG7", 2, 2, 35.0), ("QGG12", "QGG8", "QGG7", 3, 2, 34.0), ("QGG13", "QGG9", "QGG2", 3, 1, 20.0),
              ("QGG14", "QGG3", "QGG6", 3, 2, 40.0)]


def pblup_sire_dam():
    pos = {a: i + 1 for i, (a, _, _) in enumerate(PBLUP_PED)}
    pos["0"] = 0
    return (np.array([pos[s] for _, s, _ in PBLUP_PED], dtype=np.int32), np.array([pos[d] for _, _, d in PBLUP_PED], dtype=np.int32))


def inbred_pedigree(n=60, founders=3, window=6, seed=1):
    """Both parents of every non-founder drawn (with replacement: selfings happen) from the `window` animals in front of it."""
    rng = np.random.default_rng(seed)
    s, d = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    for i in range(founders, n):
        lo = max(0, i - window)
        s[i], d[i] = rng.integers(lo, i) + 1, rng.integers(lo, i) + 1
    return s, d


def random_pedigree(n, founders, seed=2, window=None):
    """Founders first; every later animal has two different parents drawn from the animals in front of it (the last `window` of them)."""
    rng = np.random.default_rng(seed)
    s, d = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
    for i in range(founders, n):
        lo = 0 if window is None else max(0, i - window)
        a, b = int(rng.integers(lo, i)), int(rng.integers(lo, i - 1))
        s[i], d[i] = a + 1, (b + 1 if b >= a else b) + 1
    return s, d


def csr_rows(kp, kc, kv):
    return [[(int(kc[k]), float(kv[k])) for k in range(int(kp[l]), int(kp[l + 1]))] for l in range(len(kp) - 1)]


def csr_dense(kp, kc, kv):
    q = len(kp) - 1
    K = np.zeros((q, q))
    for l in range(q):
        K[l, kc[kp[l]:kp[l + 1]]] = kv[kp[l]:kp[l + 1]]
    return K


def depths(rows):
    dep = [0] * len(rows)
    for l, row in enumerate(rows):
        for c, _ in row:
            if c < l:
                dep[l] = max(dep[l], dep[c] + 1)
    return dep


def schedule(rows):
    """(order, dptr): the rows by (depth, row); the rows of depth d are order[dptr[d]:dptr[d + 1]]."""
    dep = depths(rows)
    order = sorted(range(len(rows)), key=lambda l: (dep[l], l))
    nd = max(dep) + 1
    dptr = [0] * (nd + 1)
    for l in range(len(rows)):
        dptr[dep[l] + 1] += 1
    for d in range(nd):
        dptr[d + 1] += dptr[d]
    return order, dptr


def plan(dptr):
    """[("wide", d, d + 1) | ("fused", d0, d1)]: the launches of one step, in order."""
    out, run0 = [], None
    nd = len(dptr) - 1
    for d in range(nd):
        if dptr[d + 1] - dptr[d] > FUSE_ROWS:
            if run0 is not None:
                out.append(("fused", run0, d))
                run0 = None
            out.append(("wide", d, d + 1))
        elif run0 is None:
            run0 = d
    if run0 is not None:
        out.append(("fused", run0, nd))
    return out


def random_step_scheduled(O, seed, chain, it, rset, yt, rs, level, q, rows, zpz, u, varU, varE, df, scale):
    """ref_random.random_step_blocked for a K with off-diagonal entries given as rows, the Gauss-Seidel walked launch by launch and
    depth by depth.  Returns (yt, u, varU) new."""
    yt = [float(x) for x in yt]
    u = [float(x) for x in u]
    recs = RR.level_records(level, q)
    iVarE, iVarU = 1.0 / varE, 1.0 / varU
    Yi, inv, tz, dhi, du = [0.0] * q, [0.0] * q, [0.0] * q, [0.0] * q, [0.0] * q
    for l in range(q):                                   # k_rand_levels, as random_step_blocked has it
        lanes = [0.0] * 64
        for k, i in enumerate(recs[l]):
            t = rs[i] * yt[i] if rs is not None else yt[i]
            lanes[k % 64] = lanes[k % 64] + t
        acc = RR._butterfly(lanes)
        tu = zpz[l] * u[l]
        tot = acc + tu
        Yi[l] = tot * iVarE
        t1 = zpz[l] * iVarE
        t2 = [v for c, v in rows[l] if c == l][0] * iVarU
        lhs = t1 + t2
        inv[l] = 1.0 / lhs
        tz[l] = math.sqrt(inv[l]) * RR.draw(O, seed, chain, it, RR.KIND_U_NORMAL, (rset << 40) | l, 1)
        d = 0.0
        for c, v in rows[l]:
            if c > l:
                d = d + v * u[c]
        dhi[l] = d
    order, dptr = schedule(rows)
    for _, d0, d1 in plan(dptr):
        for d in range(d0, d1):
            frozen = list(u)                             # what any row of this depth may read: nothing a row of the same depth writes
            for l in reversed(order[dptr[d]:dptr[d + 1]]):
                dlo = 0.0
                for c, v in rows[l]:
                    if c < l:
                        dlo = dlo + v * frozen[c]
                dd = dlo + dhi[l]
                t = dd * iVarU
                rhs = Yi[l] - t
                mean = inv[l] * rhs
                un = mean + tz[l]
                du[l] = un - frozen[l]
                u[l] = un
    for i in range(len(yt)):
        t = du[level[i]]
        if rs is not None:
            t = rs[i] * t
        yt[i] = yt[i] - t
    thr = [0.0] * 1024
    for l in range(q):
        r = 0.0
        for c, v in rows[l]:
            r = r + v * u[c]
        thr[l % 1024] = thr[l % 1024] + u[l] * r
    waves = [RR._butterfly(thr[64 * w:64 * w + 64]) for w in range(16)]
    quad = waves[0]
    for w in range(1, 16):
        quad = quad + waves[w]
    chi = RR.draw(O, seed, chain, it, RR.KIND_U_CHI2, rset, 2, df + q)
    t = scale * df
    t = t + quad
    return yt, u, t / chi
