"""Correlated (Tuple) random-effect sets (TEST INFRASTRUCTURE): restatements written from the Julia source and from DESIGN.md
("Correlated random-effect sets"), not from the HIP code.

    /root/reference/src/functions.jl:75-89     sampleU(::Tuple): Yi = Zp[i] ycorr, rhs = Yi / varE - kron(K[i, :], inv(varU)) vec(u)
    /root/reference/src/functions.jl:100-110   sampleZ!(::Tuple): ycorr += Z_m u_m for every component, sampleU, sampleCoVarU, ycorr -= Z_m u_m
    /root/reference/src/functions.jl:503-506   sampleCoVarU = InverseWishart(df + q, U K U' + scale)
    /root/reference/src/mme.jl:207-239, 265-271  data[i] = the k columns of level i, zpz[i] = data[i]'data[i]; df = 3 + k, scale = v (df - k - 1)

THE ONE CHANGE.  The reference's Yi is formed on a ycorr that holds every component's Z u, and only the K (x) inv(varU) couplings
are subtracted: Z_a[:, l]'Z_b[:, c] u_b[c] for c != l (a record of animal l with dam c) stays in level l's right-hand side, so the
literal lines are not the Gibbs conditional of the model.  TupleRefChain subtracts W_lc u_c / varE for c != l too
(W_lc = data[l]'data[c]); TupleRefChain(literal=True) is the reference's lines as they stand, used only where the two must coincide
(no record links two different levels) and to show that they differ otherwise.

tuple_step_blocked is the device's documented order of ONE step in plain Python loops, bit for bit what ngp_sample_random_set_tuple
computes.  Its own arithmetic has no FMA; the k x k helpers (t_chol, t_spd_inv) and the Bartlett factor use fused multiply-adds where
DESIGN.md writes them, restated here exactly with rationals.  Draws come from oracle.draws: kind 12 (normal of component m of
level l of set r: key (r << 40) | (l k + m)), kind 13 (element (0, 0) of the Bartlett factor: key r), kind 17 (its other elements:
key (r << 40) | (i << 4) | j).
"""
import math
from fractions import Fraction

import numpy as np

import ref_random as RR
from ref_random import KIND_U_CHI2, KIND_U_NORMAL, RandomRefChain, _butterfly, draw

KIND_U_WISHART = 17
FUSE_ROWS = 1024


def fma(a, b, c):
    """round(a b + c), one rounding: a b = p + e exactly (Dekker's product on Veltkamp's split), and math.fsum rounds the exact sum
    of its terms once.  Magnitudes near overflow / underflow, where the split is not exact, go through rationals."""
    p = a * b
    if not 1e-140 < abs(p) < 1e140:
        return float(Fraction(a) * Fraction(b) + Fraction(c)) if math.isfinite(p) and math.isfinite(c) else p + c
    t = 134217729.0 * a
    ah = t - (t - a)
    al = a - ah
    t = 134217729.0 * b
    bh = t - (t - b)
    bl = b - bh
    e = ((ah * bh - p) + ah * bl + al * bh) + al * bl
    return math.fsum((p, e, c))


def t_chol(S, k):
    """Lower Cholesky factor of the row-major k x k S (the k x k helpers); None when not positive definite."""
    L = [0.0] * (k * k)
    for i in range(k):
        for j in range(i + 1):
            s = S[i * k + j]
            for m in range(j):
                s = fma(-L[i * k + m], L[j * k + m], s)
            if i == j:
                if not s > 0.0:
                    return None
                L[i * k + i] = math.sqrt(s)
            else:
                L[i * k + j] = s / L[j * k + j]
    return L


def t_spd_inv(S, k):
    if k == 1:
        return [1.0 / S[0]] if S[0] > 0.0 else None
    L = t_chol(S, k)
    if L is None:
        return None
    Li = [0.0] * (k * k)
    for c in range(k):
        for i in range(c, k):
            s = 1.0 if i == c else 0.0
            for m in range(c, i):
                s = fma(-L[i * k + m], Li[m * k + c], s)
            Li[i * k + c] = s / L[i * k + i]
    out = [0.0] * (k * k)
    for i in range(k):
        for j in range(k):
            s = 0.0
            for m in range(k):
                s = fma(Li[m * k + i], Li[m * k + j], s)
            out[i * k + j] = s
    return out


def inverse_wishart_blocked(O, seed, chain, it, rset, nu, Psi, k):
    """InverseWishart(nu, Psi) by the Bartlett construction, the device's order (k >= 2)."""
    L = t_chol(t_spd_inv(Psi, k), k)
    A = [0.0] * (k * k)
    for i in range(k):
        for j in range(i + 1):
            kind, key = (KIND_U_CHI2, rset) if i == 0 else (KIND_U_WISHART, (rset << 40) | (i << 4) | j)
            A[i * k + j] = math.sqrt(draw(O, seed, chain, it, kind, key, 2, nu - i)) if i == j else draw(O, seed, chain, it, kind, key, 1)
    LA, W = [0.0] * (k * k), [0.0] * (k * k)
    for i in range(k):
        for j in range(k):
            s = 0.0
            for m in range(k):
                s = fma(L[i * k + m], A[m * k + j], s)
            LA[i * k + j] = s
    for i in range(k):
        for j in range(k):
            s = 0.0
            for m in range(k):
                s = fma(LA[i * k + m], LA[j * k + m], s)
            W[i * k + j] = s
    return t_spd_inv(W, k)


def tuple_setup(levels, q, w=None):
    """levels: k x N, -1 = no level.  (recs[m][l] = records of level l in component m, ascending; Wd[l] = W_ll, k k row-major;
    Wrows[l] = [(c, W_lc)] for c != l, c ascending): W_lc[a k + b] = sum over the records i (ascending) with level_a(i) = l and
    level_b(i) = c of w_i (1 without weights)."""
    levels = np.asarray(levels)
    k, N = levels.shape
    recs = [[[] for _ in range(q)] for _ in range(k)]
    Wd = [[0.0] * (k * k) for _ in range(q)]
    Wo = [dict() for _ in range(q)]
    for i in range(N):
        wi = 1.0 if w is None else float(w[i])
        for a in range(k):
            la = int(levels[a, i])
            if la < 0:
                continue
            recs[a][la].append(i)
            for b in range(k):
                lb = int(levels[b, i])
                if lb < 0:
                    continue
                blk = Wd[la] if la == lb else Wo[la].setdefault(lb, [0.0] * (k * k))
                blk[a * k + b] = blk[a * k + b] + wi
    return recs, Wd, [sorted(d.items()) for d in Wo]


def union_depths(rows, Wrows):
    """depth(l) = 0 for a row with no entry of K or of the off-diagonal W blocks left of its diagonal, else 1 + max depth(c) over them."""
    dep = [0] * len(rows)
    for l in range(len(rows)):
        for c in [c for c, _ in rows[l]] + [c for c, _ in Wrows[l]]:
            if c < l:
                dep[l] = max(dep[l], dep[c] + 1)
    return dep


def schedule_of(dep):
    """(order, dptr) as ref_pedigree.schedule gives them, from the depths."""
    order = sorted(range(len(dep)), key=lambda l: (dep[l], l))
    nd = max(dep) + 1
    dptr = [0] * (nd + 1)
    for d in dep:
        dptr[d + 1] += 1
    for d in range(nd):
        dptr[d + 1] += dptr[d]
    return order, dptr


def tuple_step_blocked(O, seed, chain, it, rset, yt, rs, levels, q, rows, setup, u, varU, varE, df, scale, dep=None):
    """One step of a tuple set in the device's order.  yt: the device's residual (y~ = s ycorr under weights, rs = s; else ycorr, rs
    None); rows: K as lists of (column, value), columns ascending; setup: tuple_setup(levels, q, w); u: q x k; varU, scale: k x k.
    dep: walk the Gauss-Seidel depth by depth (every row of a depth reads u and du as they were when the depth began) instead of
    in level order.  Returns (yt, u [q][k], varU [k k]) new, or varU None when a matrix was not positive definite."""
    levels = np.asarray(levels)
    k, N = levels.shape
    recs, Wd, Wrows = setup
    yt = [float(x) for x in yt]
    u = [[float(x) for x in r] for r in np.asarray(u, dtype=np.float64).reshape(q, k)]
    sig = t_spd_inv([float(x) for x in np.asarray(varU, dtype=np.float64).ravel()], k)
    iVarE = 1.0 / varE
    Yi, inv, tz, dhi = [None] * q, [None] * q, [None] * q, [None] * q
    zall = O.draws(seed, chain, it, KIND_U_NORMAL, rset << 40, 1, q * k, 0.0, 0.0, indexed=True).tolist()   # key (rset << 40) | (l k + b)
    for l in range(q):
        S = []
        for m in range(k):
            if not recs[m][l]:                       # (64 lanes of 0.0 sum to 0.0)
                S.append(0.0)
                continue
            lanes = [0.0] * 64
            for p, i in enumerate(recs[m][l]):
                t = rs[i] * yt[i] if rs is not None else yt[i]
                lanes[p % 64] = lanes[p % 64] + t
            S.append(_butterfly(lanes))
        W = Wd[l]
        Yi[l] = []
        for a in range(k):
            t = 0.0
            for b in range(k):
                t = t + W[a * k + b] * u[l][b]
            Yi[l].append((S[a] + t) * iVarE)
        kd = [v for c, v in rows[l] if c == l][0]
        LHS = [W[a] * iVarE + kd * sig[a] for a in range(k * k)]
        inv[l] = t_spd_inv(LHS, k)
        L = t_chol(inv[l], k)
        z = zall[l * k:l * k + k]
        tz[l] = []
        for a in range(k):
            t = 0.0
            for b in range(a + 1):
                t = t + L[a * k + b] * z[b]
            tz[l].append(t)
        d = [0.0] * k
        for c, v in rows[l]:
            if c > l:
                for a in range(k):
                    d[a] = d[a] + v * u[c][a]
        dhi[l] = d
    du = [[0.0] * k for _ in range(q)]

    def row(l, ur, dur):
        d, wlo = [0.0] * k, [0.0] * k
        for c, v in rows[l]:
            if c < l:
                for a in range(k):
                    d[a] = d[a] + v * ur[c][a]
        for c, Wb in Wrows[l]:
            if c < l:
                for a in range(k):
                    for b in range(k):
                        wlo[a] = wlo[a] + Wb[a * k + b] * dur[c][b]
        d = [d[a] + dhi[l][a] for a in range(k)]
        rhs = []
        for a in range(k):
            sd = 0.0
            for b in range(k):
                sd = sd + sig[a * k + b] * d[b]
            t = iVarE * wlo[a]
            r = Yi[l][a] - t
            rhs.append(r - sd)
        un = []
        for a in range(k):
            mean = 0.0
            for b in range(k):
                mean = mean + inv[l][a * k + b] * rhs[b]
            un.append(mean + tz[l][a])
        return un, [un[a] - ur[l][a] for a in range(k)]

    if dep is None:
        for l in range(q):
            u[l], du[l] = row(l, u, du)
    else:
        order, dptr = schedule_of(dep)
        for d in range(len(dptr) - 1):
            fu, fdu = [list(r) for r in u], [list(r) for r in du]
            for l in reversed(order[dptr[d]:dptr[d + 1]]):
                u[l], du[l] = row(l, fu, fdu)
    for i in range(N):
        t = 0.0
        for m in range(k):
            lv = int(levels[m, i])
            if lv >= 0:
                t = t + du[lv][m]
        if rs is not None:
            t = rs[i] * t
        yt[i] = yt[i] - t
    pairs = [(a, b) for a in range(k) for b in range(a, k)]
    thr = [[0.0] * 1024 for _ in pairs]
    for l in range(q):
        r = [0.0] * k
        for c, v in rows[l]:
            for b in range(k):
                r[b] = r[b] + v * u[c][b]
        for p, (a, b) in enumerate(pairs):
            thr[p][l % 1024] = thr[p][l % 1024] + u[l][a] * r[b]
    scale = [float(x) for x in np.asarray(scale, dtype=np.float64).ravel()]
    Psi = [0.0] * (k * k)
    for p, (a, b) in enumerate(pairs):
        waves = [_butterfly(thr[p][64 * w:64 * w + 64]) for w in range(16)]
        tot = waves[0]
        for w in range(1, 16):
            tot = tot + waves[w]
        Psi[a * k + b] = scale[a * k + b] + tot
        Psi[b * k + a] = scale[b * k + a] + tot
    return yt, u, inverse_wishart_blocked(O, seed, chain, it, rset, df + q, Psi, k)


def conditional_of_level(l, levels, q, K, u, varU, varE, ycorr, literal=False):
    """(mean, covariance) of level l's k-vector as the restatement draws it, every other level at its value in u (q x k); ycorr is
    the residual with EVERY effect taken out.  K dense q x q.  literal: the reference's lines."""
    levels = np.asarray(levels)
    k, N = levels.shape
    Zl = [np.zeros((N, k)) for _ in range(q)]                                   # data[i]: mme.jl:215-217
    for m in range(k):
        for i in range(N):
            if levels[m, i] >= 0:
                Zl[int(levels[m, i])][i, m] = 1.0
    u = np.asarray(u, dtype=np.float64)
    yc = ycorr + sum(Zl[c] @ u[c] for c in range(q))                           # functions.jl:102-104
    iVarU = np.linalg.inv(varU)
    uVec = u.copy()
    uVec[l] = 0.0                                                               # :80
    rhs = Zl[l].T @ yc / varE - np.kron(K[[l], :], iVarU) @ uVec.ravel()        # :81-82
    if not literal:
        for c in range(q):
            if c != l:
                rhs = rhs - (Zl[l].T @ Zl[c]) @ u[c] / varE
    invLhs = np.linalg.inv(Zl[l].T @ Zl[l] / varE + K[l, l] * iVarU)            # :83
    return invLhs @ rhs, invLhs


class TupleRefChain(RandomRefChain):
    """RandomRefChain with sampleZ!(::Tuple) for tuple sets (unweighted, as the reference has it).  Random sets of both kinds share one
    id sequence, in the order added."""

    def __init__(self, *a, literal=False, **kw):
        super().__init__(*a, **kw)
        self.literal = literal

    def add_random_tuple(self, levels, q, K=None, df=None, scale=None, v=None):      # mme.jl:207-239, 265-271
        levels = np.asarray(levels, dtype=np.int64)
        k = levels.shape[0]
        data = [np.zeros((self.N, k)) for _ in range(q)]
        for m in range(k):
            for i in range(self.N):
                if levels[m, i] >= 0:
                    data[int(levels[m, i])][i, m] = 1.0
        df = 3.0 + k if df is None else df
        v = np.asarray(v, dtype=np.float64).reshape(k, k)
        self.Z = getattr(self, "Z", [])
        self.Z.append(dict(tuple=True, k=k, data=data, zpz=[d.T @ d for d in data], iVarStr=np.eye(q) if K is None else np.asarray(K, dtype=np.float64),
                           df=df, scale=v * (df - k - 1.0) if scale is None else np.asarray(scale, dtype=np.float64).reshape(k, k)))
        self.u = getattr(self, "u", [])
        self.u.append(np.zeros((q, k)))                                               # (the reference holds it k x q)
        self.varU = getattr(self, "varU", [])
        self.varU.append(v.copy())

    def sampleZ(self, r, varE):
        Zs = self.Z[r]
        if not Zs.get("tuple"):
            return super().sampleZ(r, varE)
        k, data, K = Zs["k"], Zs["data"], Zs["iVarStr"]
        q = len(data)
        u = self.u[r]
        for c in range(q):                                                            # functions.jl:102-104
            self.ycorr += data[c] @ u[c]
        iVarU = np.linalg.inv(self.varU[r])                                           # :78
        for i in range(q):
            u[i] = 0.0                                                                # :80
            Yi = data[i].T @ self.ycorr                                               # :81
            rhsU = Yi / varE - np.kron(K[[i], :], iVarU) @ u.ravel()                  # :82
            if not self.literal:                                                      # THE ONE CHANGE: W_ic u_c / varE for c != i
                for c in self._linked(Zs, i):
                    rhsU = rhsU - (data[i].T @ data[c]) @ u[c] / varE
            invLhsU = np.linalg.inv(Zs["zpz"][i] / varE + K[i, i] * iVarU)            # :83
            meanU = invLhsU @ rhsU                                                    # :84
            z = np.array([self.draw_k(KIND_U_NORMAL, (r << 40) | (i * k + m), 1) for m in range(k)])
            u[i] = meanU + np.linalg.cholesky((invLhsU + invLhsU.T) / 2) @ z          # :85
        S = u.T @ K @ u                                                               # :505 (effVec is k x q there)
        self.varU[r] = self._inverse_wishart(r, Zs["df"] + q, (S + S.T) / 2 + Zs["scale"], k)
        for c in range(q):                                                            # :107-109
            self.ycorr -= data[c] @ u[c]

    def _linked(self, Zs, i):
        if "links" not in Zs:
            q = len(Zs["data"])
            nz = [set(np.nonzero(d.any(axis=1))[0].tolist()) for d in Zs["data"]]
            Zs["links"] = [[c for c in range(q) if c != l and nz[l] & nz[c]] for l in range(q)]
        return Zs["links"][i]

    def _inverse_wishart(self, r, nu, Psi, k):
        L = np.linalg.cholesky(np.linalg.inv(Psi))
        A = np.zeros((k, k))
        for i in range(k):
            for j in range(i + 1):
                kind, key = (KIND_U_CHI2, r) if i == 0 else (KIND_U_WISHART, (r << 40) | (i << 4) | j)
                A[i, j] = math.sqrt(self.draw_k(kind, key, 2, nu - i)) if i == j else self.draw_k(kind, key, 1)
        LA = L @ A
        return np.linalg.inv(LA @ LA.T)
