"""Numpy restatement of the BayesRCpi marker set (TEST INFRASTRUCTURE): annotation-informed BayesR, src/functions.jl:291-360 with
:518-520 and :536-544, set-up src/mme.jl:384-403.  The C oracle has no such set; this file is the specification the device is held to
("BayesRCpi sets").  Two forms:

  * RCRefChain -- the REFERENCE ORDER: one locus after another in Float64, the literal lines, with the project's draw layer and keys
    (`O.draws`: the first draw of the keyed stream).  Agrees with the device to rounding; it also records the smallest relative margin
    of every comparison it makes, so that a test can tell a rounding difference from a wrong rule.
  * lane_tables / lane_eval / block_chain / behind_sweep -- the BLOCKED rule, operation by operation as k_prep, eval_rcform and the
    kernels of ngp_bayesrc.h perform it (fma where they use one, every other operation rounded on its own): bit for bit the device.

Keys (kind, index): the locus' normal (3, set<<40 | locus); the annotation uniform (19, set<<40 | locus); the comparison uniform of
slot i = a K + v (8 for i < 8 else 18, set<<40 | locus<<3 | i&7); the variance of annotation a (4, set<<40 | a); the Dirichlet gamma
of slot i (9, set<<40 | i); the annotProb gamma (20, set<<40 | locus<<3 | a)."""
import math

import numpy as np

from ref_numpy import RefChain
from ref_random_tuple import fma

K_NORMAL, K_CHI2, K_UNI, K_DIR, K_UNI_HI, K_RC_UNI, K_RC_ANNOT = 3, 4, 8, 9, 18, 19, 20
INF = float("inf")


def draw(O, seed, chain, it, kind, index, what, p1=0.0, p2=0.0):
    return float(O.draws(seed, chain, it, kind, index, what, 1, p1, p2, indexed=True)[0])


def slot_uniform(O, seed, chain, it, si, l, i):
    return draw(O, seed, chain, it, K_UNI if i < 8 else K_UNI_HI, (si << 40) | (l << 3) | (i & 7), 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# the blocked rule
# ---------------------------------------------------------------------------------------------------------------------------------
def lane_tables(O, seed, chain, it, si, l, mpm, lhs0, iVarE, varBeta, vClass, logpi, prob, mask):
    """k_prep's slot tables of locus l: dict(q, a, t, u: one entry per slot; U; alast).  varBeta[a]; logpi[a][v]; prob[a] = annotProb[l, a];
    mask[a] = the locus has annotation a."""
    A, K = len(varBeta), len(vClass)
    t2 = mpm * iVarE + lhs0
    z = draw(O, seed, chain, it, K_NORMAL, (si << 40) | l, 1)
    q, a_, t, u = [], [], [], []
    alast = 0
    for a in range(A):
        has = bool(mask[a])
        if has:
            alast = a
        lp = O.det_log(prob[a]) if has else 0.0
        for v in range(K):
            i = a * K + v
            uv = slot_uniform(O, seed, chain, it, si, l, i)
            varc = varBeta[a] * vClass[v]
            if not has:
                q.append(0.0); a_.append(-INF); t.append(0.0); u.append(INF)
            elif varc == 0.0:
                q.append(0.0); a_.append(logpi[a][v] + lp); t.append(0.0); u.append(uv)
            else:
                lhs = t2 + 1.0 / varc
                ilhs = 1.0 / lhs
                hl = 0.5 * O.det_log(varc * lhs)
                q.append(ilhs); a_.append((logpi[a][v] - hl) + lp); t.append(math.sqrt(ilhs) * z); u.append(uv)
    return dict(q=q, a=a_, t=t, u=u, U=draw(O, seed, chain, it, K_RC_UNI, (si << 40) | l, 0), alast=alast, K=K, A=A)


def lane_eval(O, T, r, iVarE, rhs0, bo):
    """eval_rcform: (class from 0, annotation from 0, candidate dlt) of a lane with tables T at the current r."""
    K, A = T["K"], T["A"]
    ns = A * K
    rhs = r * iVarE + rhs0
    hs = 0.5 * (rhs * rhs)
    L = [T["a"][i] if T["q"][i] == 0.0 else fma(hs, T["q"][i], T["a"][i]) for i in range(ns)]
    m = L[0]
    for i in range(1, ns):
        m = L[i] if L[i] > m else m
    e = [O.det_exp(L[i] - m) if L[i] - m >= -708.0 else 0.0 for i in range(ns)]
    Ta = []
    for a in range(A):
        tc = e[a * K]
        for v in range(1, K):
            tc = tc + e[a * K + v]
        Ta.append(tc)
    S = Ta[0]
    for a in range(1, A):
        S = S + Ta[a]
    thr = T["U"] * S
    asel, cum = T["alast"], 0.0
    for a in range(A):
        cum = Ta[0] if a == 0 else cum + Ta[a]
        if cum >= thr:
            asel = a
            break
    c, cum = K - 1, 0.0
    for v in range(K):
        i = asel * K + v
        cum = e[i] if v == 0 else cum + e[i]
        if cum >= T["u"][i] * Ta[asel]:
            c = v
            break
    i = asel * K + c
    cand = (fma(rhs, T["q"][i], T["t"][i]) - bo) if T["q"][i] != 0.0 else -bo
    return c, asel, cand


def block_chain(O, tables, r0, G, iVarE, rhs0, bo):
    """The 64-wide rule on one block whose lanes are all of the set: every lane evaluated, the first non-zero candidate at or behind the
    cursor steps (r_j = fma(-G[k][j], dlt_k, r_j) for j > k), the lanes behind it are evaluated again; a lane that is passed over keeps
    the class and annotation of the evaluation in which it was passed.  Returns per lane (class, annotation, dlt)."""
    n = len(tables)
    r = list(r0)
    fin = [None] * n
    kstart = 0
    while kstart < n:
        ev = {j: lane_eval(O, tables[j], r[j], iVarE, rhs0[j], bo[j]) for j in range(kstart, n)}
        for j in range(kstart, n):
            fin[j] = ev[j]
        todo = [j for j in range(kstart, n) if ev[j][2] != 0.0]
        if not todo:
            break
        kk = todo[0]
        dk = ev[kk][2]
        for j in range(kk + 1, n):
            r[j] = fma(-float(G[kk][j]), dk, r[j])
        kstart = kk + 1
    return fin


def _butterfly(x):
    x = list(x)
    for off in (32, 16, 8, 4, 2, 1):
        x = [x[i] + x[i ^ off] for i in range(64)]
    return x[0]


def behind_sweep(O, seed, chain, it, si, beta, cls, ann, mask, df, scale, vClass, A, estPi):
    """k_rc_count + k_rc_draw + k_rc_annot from the classes / annotations (from 0) and effects the sweep left: (varBeta[A], pi[A][K] or
    None, annotProb[ncol][A]).  sumS in the segment pattern of k_rssq: 256-locus segments, lane l adds loci l, l+64, l+128, l+192, xor
    butterfly, segments in order."""
    n, K = len(beta), len(vClass)
    varBeta, pi = [], []
    for a in range(A):
        tot = None
        for s0 in range(0, n, 256):
            acc = [0.0] * 64
            for lane in range(64):
                for m in range(4):
                    l = s0 + lane + 64 * m
                    if l < min(n, s0 + 256) and ann[l] == a and vClass[cls[l]] != 0.0:
                        acc[lane] = acc[lane] + (beta[l] * beta[l]) / vClass[cls[l]]
            p = _butterfly(acc)
            tot = p if tot is None else tot + p
        nl = [int(np.sum((np.asarray(ann) == a) & (np.asarray(cls) == v))) for v in range(K)]
        nnz = sum(nl[v] for v in range(K) if vClass[v] != 0.0)
        varBeta.append((scale * df + tot) / draw(O, seed, chain, it, K_CHI2, (si << 40) | a, 2, df + nnz))
        if estPi:
            g = [draw(O, seed, chain, it, K_DIR, (si << 40) | (a * K + v), 4, nl[v] + 1.0) for v in range(K)]
            gs = 0.0
            for x in g:
                gs = gs + x
            pi.append([x / gs for x in g])
    prob = np.zeros((n, A))
    for l in range(n):
        pres = [a for a in range(A) if mask[l][a]]
        if len(pres) == 1:
            prob[l, pres[0]] = 1.0
            continue
        g, gs = {}, 0.0
        for a in pres:
            g[a] = draw(O, seed, chain, it, K_RC_ANNOT, (si << 40) | (l << 3) | a, 4, 2.0 if a == ann[l] else 1.0)
            gs = gs + g[a]
        for a in pres:
            prob[l, a] = g[a] / gs
    return varBeta, (pi if estPi else None), prob


# ---------------------------------------------------------------------------------------------------------------------------------
# the exact law of one locus (closed forms the draws are held to)
# ---------------------------------------------------------------------------------------------------------------------------------
def locus_law(rhs, mpm_ivare_lhs0, varBeta, vClass, pi, prob):
    """(P[annotation a], P[class v | annotation a]) of a locus with right-hand side rhs: weights w[a][v] = pi[a][v] (varc lhs)^-1/2
    exp(rhs^2 / (2 lhs)) annotProb[a]; the annotation has probability S_a / sum S; inside it the fresh-uniform search stops at class v
    with probability c_v prod_{m<v} (1 - c_m), c_v the cumulative share, the last class taking the remainder."""
    A, K = len(varBeta), len(vClass)
    logw = np.full((A, K), -np.inf)
    for a in range(A):
        if prob[a] <= 0.0:
            continue
        for v in range(K):
            varc = varBeta[a] * vClass[v]
            if varc == 0.0:
                logw[a, v] = math.log(pi[a][v]) + math.log(prob[a])
            else:
                lhs = mpm_ivare_lhs0 + 1.0 / varc
                logw[a, v] = math.log(pi[a][v]) - 0.5 * math.log(varc * lhs) + 0.5 * rhs * rhs / lhs + math.log(prob[a])
    w = np.exp(logw - logw.max())
    Sa = w.sum(axis=1)
    pa = Sa / Sa.sum()
    pc = np.zeros((A, K))
    for a in range(A):
        if Sa[a] == 0.0:
            continue
        cshare = np.cumsum(w[a]) / Sa[a]
        left = 1.0
        for v in range(K):
            stop = 1.0 if v == K - 1 else min(1.0, cshare[v])
            pc[a, v] = left * stop
            left *= 1.0 - stop
    return pa, pc


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference order
# ---------------------------------------------------------------------------------------------------------------------------------
class RCRefChain(RefChain):
    """RefChain with BayesRCpi sets (method 6).  min_margin: the smallest relative margin |lhs - rhs| / max(|lhs|, |rhs|) over every
    comparison of an annotation or class search made so far."""

    def __init__(self, *a, **k):
        super().__init__(*a, **k)
        self.min_margin = INF
        self.annotCat, self.annotProb = {}, {}

    def add_set_rc(self, col0, ncol, df, scale, v, vClass, pi, annot, estPi=False):      # mme.jl:384-403
        self.add_set(col0, ncol, 6, df, scale, [(j, j + 1) for j in range(ncol)], [v] * np.asarray(annot).shape[1], pi0=0.5, estPi=estPi)
        M = self.M[-1]
        an = np.asarray(annot, dtype=np.float64).reshape(ncol, -1)
        M["vClass"] = np.array(vClass, float); M["annot"] = an; M["A"] = an.shape[1]
        M["piHat"] = np.tile(np.array(pi, float), (an.shape[1], 1)); M["logPi"] = np.log(M["piHat"])          # :388-392
        M["annotProb"] = an / an.sum(axis=1, keepdims=True)                                                    # :396
        M["annotCat"] = np.ones(ncol, dtype=np.int64)     # (:403 starts at zeros; never read before the first sweep, 1 as the library)

    def _inclusion(self, si, locus, rrr, varE, vbeta):     # (BayesB / BayesC sets beside such a set: their comparison's margin too)
        M = self.M[si]
        v0 = np.float64(M["mpm"][locus]) * varE
        v1 = (np.float64(M["mpm"][locus]) ** 2) * vbeta + v0
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            p1 = 1.0 / (1.0 + np.exp((-0.5 * (np.log(v0) + rrr ** 2 / v0) + M["logPi"][0]) - (-0.5 * (np.log(v1) + rrr ** 2 / v1) + M["logPi"][1])))
        u = self.draw("B_UNIFORM", (si << 40) | locus, 0)
        if np.isfinite(p1):
            self.min_margin = min(self.min_margin, abs(u - p1) / max(abs(u), abs(p1), 1e-300))
        return u < p1

    def _cmp(self, a, b):
        self.min_margin = min(self.min_margin, abs(a - b) / max(abs(a), abs(b), 1e-300))
        return a >= b

    def sampleBayesRC(self, si, varE):                       # functions.jl:291-360
        M, beta, delta, vb = self.M[si], self.beta[si], self.delta[si], self.varBeta[si]
        K, A = len(M["vClass"]), M["A"]
        nLoci = np.zeros((A, K), dtype=np.int64)
        sumS, nNonZero = np.zeros(A), np.zeros(A, dtype=np.int64)
        iVarE = 1.0 / varE
        for locus in range(M["dims"][1]):
            self.ycorr += beta[locus] * M["data"][:, locus]
            rhs = np.dot(M["Mp"][locus], self.ycorr) * iVarE + M["rhs"][locus]
            base = M["mpm"][locus] * iVarE + M["lhs"][locus]
            logL = np.full((A, K), -np.inf); lhs = np.zeros((A, K))
            for a in range(A):
                if M["annot"][locus, a] == 0:
                    continue
                for v in range(K):
                    varc = vb[a] * M["vClass"][v]
                    if varc == 0.0:
                        logL[a, v] = M["logPi"][a, v]
                    else:
                        lhs[a, v] = base + 1.0 / varc
                        logL[a, v] = -0.5 * (math.log(varc * lhs[a, v]) - rhs ** 2 / lhs[a, v]) + M["logPi"][a, v]
                logL[a] += math.log(M["annotProb"][locus, a])
            w = np.exp(logL - logL.max())                    # (annotProb .* sum(exp(logL)) relative to the largest weight: rounding only)
            Ta = [float(np.cumsum(w[a])[-1]) for a in range(A)]
            S = float(np.cumsum(Ta)[-1])
            U = self.draw_k(K_RC_UNI, (si << 40) | locus, 0)
            asel = max(a for a in range(A) if M["annot"][locus, a] != 0)
            cum = 0.0
            for a in range(A):
                cum += Ta[a]
                if M["annot"][locus, a] != 0 and self._cmp(cum, U * S):
                    asel = a
                    break
            c, cum = K - 1, 0.0
            for v in range(K):
                cum += w[asel, v]
                i = asel * K + v
                if self._cmp(cum, self.draw_k(K_UNI if i < 8 else K_UNI_HI, (si << 40) | (locus << 3) | (i & 7), 0) * Ta[asel]):
                    c = v
                    break
            delta[locus] = c + 1
            M["annotCat"][locus] = asel + 1
            nLoci[asel, c] += 1
            if vb[asel] * M["vClass"][c] != 0.0:
                nNonZero[asel] += 1
                b = self.sampleBeta(si, locus, rhs / lhs[asel, c], lhs[asel, c])
                beta[locus] = b
                self.ycorr += -1.0 * b * M["data"][:, locus]
                sumS[asel] += b * b / M["vClass"][c]
            else:
                beta[locus] = 0.0
        for a in range(A):                                   # :518-520 per annotation
            vb[a] = (M["scale"] * M["df"] + sumS[a]) / self.draw_k(K_CHI2, (si << 40) | a, 2, M["df"] + nNonZero[a])
        if M["estPi"]:                                       # :536-538 per annotation
            for a in range(A):
                g = np.array([self.draw_k(K_DIR, (si << 40) | (a * K + v), 4, nLoci[a, v] + 1.0) for v in range(K)])
                M["piHat"][a] = g / g.sum()
            M["logPi"] = np.log(M["piHat"])
        for locus in range(M["dims"][1]):                    # :322, :541-544: outside the estPi branch
            pres = [a for a in range(A) if M["annot"][locus, a] != 0]
            if len(pres) == 1:
                continue
            g = np.array([self.draw_k(K_RC_ANNOT, (si << 40) | (locus << 3) | a, 4, 2.0 if a + 1 == M["annotCat"][locus] else 1.0) for a in pres])
            M["annotProb"][locus, pres] = g / g.sum()

    def draw_k(self, kind, index, what, p1=0.0, p2=0.0):
        return draw(self.O, self.seed, self.chain, self.iter, kind, index, what, p1, p2)

    def run(self, niter):
        for _ in range(niter):
            self.iter += 1
            varE = self.sampleVarE()
            self.varE = varE
            if self.intercept:
                self.sampleX(varE)
            for si, M in enumerate(self.M):
                {0: self.sampleBayesPR, 1: self.sampleBayesB, 2: self.sampleBayesC, 3: self.sampleBayesR, 6: self.sampleBayesRC}[M["method"]](si, varE)
