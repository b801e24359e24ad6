"""Single-step GBLUP (TEST INFRASTRUCTURE): restatements written from the model's formula and from DESIGN.md section 2, "Hybrid
random-effect sets (single-step GBLUP)" -- not from the HIP code.  The reference has no single-step model; the specification is

    H^-1 = A^-1 + [ 0 0 ; 0  G_w^-1 - A22^-1 ],   G_w = (1 - w) G + w A22          (Aguilar et al. 2010; Christensen & Lund 2010)

plus the project's own normative orders.  hybrid_step is ONE step of a hybrid random-effect set in the device's order, plain loops
and one IEEE double operation per product and sum.  It is put together from the parts the two existing restatements are made of --
the level terms and the level schedule of ref_pedigree.random_step_scheduled for the head rows, the dhi lanes, the 64-step chain and
the below-block butterfly of ref_gblup.dense_step_blocked for the trailing block (their helpers are called, their loops repeated on
the sub-ranges) -- and adds what is new: the fold T = D + S_tt, the seed of every trailing row, the second (unseeded) accumulator and
the quadratic form that counts the cross block exactly twice.
"""
import math

import numpy as np

import ref_pedigree as RP
import ref_random as RR


def split_k(rows, q, nd, D):
    """(folded rows, T): the entries of S (rows of (column, value), columns ascending) with row and column both among the last nd levels
    are added into the dense block, one sum per stored entry; the CSR keeps the rest."""
    hd = q - nd
    T = np.array(D, dtype=np.float64).reshape(nd, nd).copy()
    out = []
    for l, row in enumerate(rows):
        keep = []
        for c, v in row:
            if l >= hd and c >= hd:
                T[l - hd, c - hd] = T[l - hd, c - hd] + v
            else:
                keep.append((c, v))
        out.append(keep)
    return out, T


def hybrid_step(O, seed, chain, it, rset, yt, rs, level, q, rows, nd, D, zpz, u, varU, varE, df, scale):
    """One step of a hybrid set: S as rows of (column, value) over q levels, D dense nd x nd over the last nd levels.  yt: the device's
    residual (y~ = s ycorr under weights, rs = s; else ycorr, rs None).  Returns (yt, u, varU) new; inputs are not changed."""
    hd = q - nd
    S = rows                                                 # (the full stored rows: the quadratic form of a head row uses them)
    rows, T = split_k(rows, q, nd, D)
    yt = [float(x) for x in yt]
    u = [float(x) for x in u]
    uold = list(u)
    recs = RR.level_records(level, q)
    iVarE, iVarU = 1.0 / varE, 1.0 / varU
    kdiag = [[v for c, v in S[l] if c == l][0] for l in range(hd)] + [float(T[j, j]) for j in range(nd)]
    Yi, inv, tz, dhi, du = [0.0] * q, [0.0] * q, [0.0] * q, [0.0] * q, [0.0] * q
    for l in range(q):                                       # k_rand_levels, all q levels, over the folded CSR
        lanes = [0.0] * 64
        for k, i in enumerate(recs[l]):
            t = rs[i] * yt[i] if rs is not None else yt[i]
            lanes[k % 64] = lanes[k % 64] + t
        acc = RR._butterfly(lanes)
        tu = zpz[l] * u[l]
        tot = acc + tu
        Yi[l] = tot * iVarE
        t1 = zpz[l] * iVarE
        t2 = kdiag[l] * iVarU
        lhs = t1 + t2
        inv[l] = 1.0 / lhs
        tz[l] = math.sqrt(inv[l]) * RR.draw(O, seed, chain, it, RR.KIND_U_NORMAL, (rset << 40) | l, 1)
        d = 0.0
        for c, v in rows[l]:                                 # (a trailing row has no stored column > l after the fold)
            if c > l:
                d = d + v * u[c]
        dhi[l] = d
    for j in range(nd):                                      # k_hyb_dhi: the dense dhi of the trailing rows, old u
        lanes = [0.0] * 64
        for c in range(j + 1, nd):
            lanes[c % 64] = lanes[c % 64] + float(T[j, c]) * uold[hd + c]
        dhi[hd + j] = RR._butterfly(lanes)
    if hd > 0:                                               # the head rows, depth by depth (the serial walk gives the same bits)
        order, dptr = RP.schedule(rows[:hd])
        for _, d0, d1 in RP.plan(dptr):
            for d in range(d0, d1):
                frozen = list(u)
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
    seedv = [0.0] * nd                                       # k_hyb_seed: this sweep's head values
    for j in range(nd):
        a = 0.0
        for c, v in rows[hd + j]:
            a = a + v * u[c]
        seedv[j] = a
    acc = list(seedv)                                        # the seeded accumulator, and the dense part from 0.0
    acc0 = [0.0] * nd
    ddl = [0.0] * nd
    for b0 in range(0, nd, 64):                              # k_hyb_block, block by block
        b1 = min(b0 + 64, nd)
        dlo = acc[b0:b1]
        dd0 = acc0[b0:b1]
        for s in range(b1 - b0):
            l = hd + b0 + s
            d = dlo[s] + dhi[l]
            t = d * iVarU
            rhs = Yi[l] - t
            mean = inv[l] * rhs
            un = mean + tz[l]
            du[l] = un - u[l]
            u[l] = un
            for j in range(s + 1, b1 - b0):
                p = float(T[b0 + j, b0 + s]) * un
                dlo[j] = dlo[j] + p
                dd0[j] = dd0[j] + p
        ddl[b0:b1] = dd0
        for r in range(b1, nd):
            lanes = [0.0] * 64
            for j in range(b1 - b0):
                lanes[j] = float(T[r, b0 + j]) * u[hd + b0 + j]
            p = RR._butterfly(lanes)
            acc[r] = acc[r] + p
            acc0[r] = acc0[r] + p
    for i in range(len(yt)):                                 # k_rand_update
        t = du[level[i]]
        if rs is not None:
            t = rs[i] * t
        yt[i] = yt[i] - t
    thr = [0.0] * 1024                                       # k_hyb_var
    for l in range(q):
        if l < hd:
            r = 0.0
            for c, v in S[l]:
                r = r + v * u[c]
            p = u[l] * r
        else:
            j = l - hd
            a = float(T[j, j]) * u[l]
            b = 2.0 * ddl[j]
            s = a + b
            s = s + seedv[j]
            p = u[l] * s
        thr[l % 1024] = thr[l % 1024] + p
    waves = [RR._butterfly(thr[64 * w:64 * w + 64]) for w in range(16)]
    quad = waves[0]
    for w in range(1, 16):
        quad = quad + waves[w]
    chi = RR.draw(O, seed, chain, it, RR.KIND_U_CHI2, rset, 2, df + q)
    t = scale * df
    t = t + quad
    return np.array(yt), np.array(u), t / chi


def embed(rows, q, nd, D):
    """The dense q x q K = S + embed(D)."""
    K = np.zeros((q, q))
    for l, row in enumerate(rows):
        for c, v in row:
            K[l, c] = v
    K[q - nd:, q - nd:] = K[q - nd:, q - nd:] + np.asarray(D, dtype=np.float64)
    return K


def colleau_a22(sire, dam, F, idx):
    """A[idx, idx] by Colleau's indirect method, A = T diag(d) T': per listed animal one backward pass, the Mendelian variances, one
    forward pass (include/nextgp_hip.h, ngp_pedigree_a22)."""
    n = len(sire)
    d = np.ones(n)
    for i in range(n):
        s, m = int(sire[i]), int(dam[i])
        if s and m:
            d[i] = 0.5 - (F[s - 1] + F[m - 1]) / 4.0
        elif s or m:
            d[i] = 0.75 - F[(s or m) - 1] / 4.0
    out = np.zeros((len(idx), len(idx)))
    for j, g in enumerate(idx):
        x = np.zeros(n)
        x[g] = 1.0
        for i in range(int(g), -1, -1):
            if sire[i]:
                x[sire[i] - 1] += x[i] / 2.0
            if dam[i]:
                x[dam[i] - 1] += x[i] / 2.0
        x = x * d
        w = np.zeros(n)
        for i in range(n):
            ws = w[sire[i] - 1] if sire[i] else 0.0
            wd = w[dam[i] - 1] if dam[i] else 0.0
            w[i] = x[i] + (ws + wd) / 2.0
        out[j] = w[np.asarray(idx)]
    return out


def renumber(n, geno_pos):
    """perm[new] = old: the non-genotyped animals first, in pedigree order, then the genotyped ones in the order given."""
    g = set(int(a) for a in geno_pos)
    return np.array([i for i in range(n) if i not in g] + [int(a) for a in geno_pos], dtype=np.int64)


def h_inverse(A, G, idx, w):
    """The dense H^-1 in PEDIGREE order from A (api.makeA), G (with its ridge) over the animals idx, and the blending weight w."""
    A = np.asarray(A, dtype=np.float64)
    idx = np.asarray(idx, dtype=np.int64)
    A22 = A[np.ix_(idx, idx)]
    Gw = (1.0 - w) * np.asarray(G, dtype=np.float64) + w * A22
    H = np.linalg.inv(A)
    H[np.ix_(idx, idx)] += np.linalg.inv(Gw) - np.linalg.inv(A22)
    return (H + H.T) / 2.0
