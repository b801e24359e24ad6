"""BayesLV marker sets (TEST INFRASTRUCTURE): two restatements, written from the Julia source and from DESIGN.md, not from the HIP code.

    /root/reference/src/functions.jl:421-440   sampleBayesLV!, the sweep: BayesPR's with one variance per locus
    /root/reference/src/functions.jl:442-470   the slice draw of every locus' variance
    /root/reference/src/functions.jl:475-485   c ~ MvNormal(iCpC C'logVar, iCpC varZeta), zeta = logVar - C c, varZeta
    /root/reference/src/mme.jl:418-439         set-up: logVar, design matrix, iCpC = inv(C'C + min|diag / 10000| I)

LVRefChain is the reference's order on top of ref_numpy.RefChain (libm log / exp, ** -1.5, numpy dots and var: agreement to
rounding).  lv_step_blocked is the device's documented order of ONE variance step ("BayesLV sets") in plain Python loops:
bit for bit what the device computes behind the sweep of such a set.  The step has no FMA, so every operation below is one IEEE
double operation; log and exp are the oracle's fixed sequences (det_log, det_exp).  Draws come from oracle.draws on the new kinds 14
(four consecutive uniforms of ONE stream per locus: key (set << 40) | locus), 15 (normal of coefficient k: (set << 40) | k) and 16
(starting value of zeta at iteration 0: (set << 40) | locus).
"""
import math

import numpy as np

from ref_numpy import RefChain

KIND_LV_UNIFORM, KIND_LV_NORMAL, KIND_LV_START = 14, 15, 16
INF, NAN = float("inf"), float("nan")


# ---- IEEE helpers: Python raises where the hardware returns inf / NaN ----
def fdiv(a, b):
    if b == 0.0 and a == a:
        if a == 0.0:
            return NAN
        return math.copysign(INF, a) * math.copysign(1.0, b)
    return a / b


def fsqrt(x):
    if x != x or x < 0.0:
        return NAN
    return math.sqrt(x)


def det_exp_any(O, x):
    """x <= 0: the oracle's det_exp; x > 0: its IEEE reciprocal 1 / det_exp(-x); a NaN comes back a NaN."""
    if x <= 0.0:
        return O.det_exp(x)
    return fdiv(1.0, O.det_exp(-x))


def butterfly(v):
    """acc = acc + shfl_xor(acc, off), off = 32 .. 1, over 64 lanes; lane 0's value."""
    v = list(v)
    off = 32
    while off >= 1:
        v = [v[j] + v[j ^ off] for j in range(64)]
        off >>= 1
    return v[0]


def sum_segments(p):
    tot = p[0]
    for x in p[1:]:
        tot = tot + x
    return tot


def segment_partials(n, term):
    """One partial per 256 loci: lane j adds term(l) of its loci j, j + 64, j + 128, j + 192 (that order, from 0.0), then the butterfly."""
    out = []
    for s0 in range(0, n, 256):
        lanes = [0.0] * 64
        for j in range(64):
            for m in range(4):
                l = s0 + j + 64 * m
                if l < min(n, s0 + 256):
                    lanes[j] = lanes[j] + term(l)
        out.append(butterfly(lanes))
    return out


def zeta_start(O, seed, chain, lset, n):
    return np.array([float(O.draws(seed, chain, 0, KIND_LV_START, (lset << 40) | l, 0, 1)[0]) for l in range(n)])


def icpc(C):
    """inv(C'C + min_i |(C'C)_ii / 10000| I)  (src/mme.jl:432-437)."""
    C = np.asarray(C, dtype=np.float64)
    A = C.T @ C
    A = A + np.eye(A.shape[0]) * np.abs(np.diag(A) / 10000).min()
    return np.linalg.inv(A)


def slice_bounds(O, vari, bi, z, varZeta, u1, u2, u3):
    """(lbound, rbound) of one locus in the device's order (src/functions.jl:448-462, left to right as Julia parses each line)."""
    lv0 = O.det_log(vari)
    var_mui = lv0 - z
    sv = math.sqrt(vari)
    v15 = vari * sv
    p15 = fdiv(1.0, v15)
    c1 = p15 * u1
    hb = -0.5 * bi
    hbb = hb * bi
    a2 = fdiv(hbb, vari)
    c2 = det_exp_any(O, a2) * u2
    hz = -0.5 * z
    hzz = hz * z
    a3 = fdiv(hzz, varZeta)
    c3 = det_exp_any(O, a3) * u3
    m2v = -2.0 * varZeta
    t3 = m2v * O.det_log(c3)
    temp = fsqrt(t3)
    lbound = det_exp_any(O, var_mui - temp)
    rbound = det_exp_any(O, var_mui + temp)
    r2 = det_exp_any(O, (-2.0 / 3.0) * O.det_log(c1))
    if r2 < rbound:
        rbound = r2
    l2 = fdiv(hbb, O.det_log(c2))
    if l2 > lbound:
        lbound = l2
    return lbound, rbound


def lv_step_blocked(O, seed, chain, it, lset, beta, varBeta, zeta, C, iCpC, varZeta, mode=0, frac=0.0, bounds=None):
    """One variance step in the device's order.  C: n x ncov; iCpC: ncov x ncov; mode 0 / 1 / 2 as est_mode.  Returns
    (varBeta, c, zeta, varZeta, trapped) new; inputs are not changed.  bounds: a list that receives (old variance, lbound, rbound)."""
    n, ncov = C.shape
    vb = [float(x) for x in varBeta]
    logv = [0.0] * n
    trapped = 0
    for l in range(n):
        u1, u2, u3, u4 = (float(x) for x in O.draws(seed, chain, it, KIND_LV_UNIFORM, (lset << 40) | l, 0, 4))
        lb, rb = slice_bounds(O, vb[l], float(beta[l]), float(zeta[l]), varZeta, u1, u2, u3)
        if bounds is not None:
            bounds.append((vb[l], lb, rb))
        if lb >= rb:
            trapped += 1
        else:
            d = rb - lb
            t = u4 * d
            vb[l] = lb + t
        logv[l] = O.det_log(vb[l])
    Cl = [[float(C[l, k]) for k in range(ncov)] for l in range(n)]
    rhsC = [sum_segments(segment_partials(n, lambda l, k=k: Cl[l][k] * logv[l])) for k in range(ncov)]
    zz = [float(O.draws(seed, chain, it, KIND_LV_NORMAL, (lset << 40) | k, 1, 1)[0]) for k in range(ncov)]
    A = [[float(iCpC[i][j]) for j in range(ncov)] for i in range(ncov)]
    L = [[0.0] * ncov for _ in range(ncov)]
    bad = False
    for i in range(ncov):
        for j in range(i + 1):
            s = A[i][j] * varZeta
            for k in range(j):
                s = s - L[i][k] * L[j][k]
            if i == j:
                bad = bad or not s > 0.0
                L[i][i] = fsqrt(s)
            else:
                L[i][j] = fdiv(s, L[j][j])
    c = []
    for i in range(ncov):
        mean = 0.0
        for j in range(ncov):
            mean = mean + A[i][j] * rhsC[j]
        acc = 0.0
        for j in range(i + 1):
            acc = acc + L[i][j] * zz[j]
        c.append(NAN if bad else mean + acc)
    znew = []
    for l in range(n):
        fit = 0.0
        for k in range(ncov):
            fit = fit + Cl[l][k] * c[k]
        znew.append(logv[l] - fit)
    if mode != 0:
        x = znew if mode == 1 else logv
        mean = sum_segments(segment_partials(n, lambda l: x[l])) / float(n)
        ss = sum_segments(segment_partials(n, lambda l: (x[l] - mean) * (x[l] - mean)))
        v = ss / float(n - 1)
        varZeta = frac * v if mode == 2 else v
    return np.array(vb), np.array(c), np.array(znew), varZeta, trapped


class LVRefChain(RefChain):
    """ref_numpy.RefChain with sampleBayesLV! (method 5).  blocked_step=True swaps the variance model for lv_step_blocked (the sweep
    stays the reference's): two chains that differ in nothing but the rounding of the variance step."""

    def __init__(self, *a, blocked_step=False, **kw):
        super().__init__(*a, **kw)
        self.blocked_step = blocked_step

    def add_set_lv(self, col0, ncol, v, C, varZeta, est=False, zeta0=None):      # mme.jl:418-439
        self.add_set(col0, ncol, 5, 4.0, 0.0, [(j, j + 1) for j in range(ncol)], [v] * ncol)
        M = self.M[-1]
        C = np.asarray(C, dtype=np.float64).reshape(ncol, -1)
        si = len(self.M) - 1
        M.update(piHat=np.array([0.5, 0.5]), covariates=C, covariatesT=C.T.copy(), iCpC=icpc(C), varZeta=[float(varZeta)], estVarZeta=est,
                 logVar=np.full(ncol, math.log(v)), c=np.zeros(C.shape[1]), trapped=0,
                 SNPVARRESID=zeta_start(self.O, self.seed, self.chain, si, ncol) if zeta0 is None else np.array(zeta0, float))

    def sampleBayesLV(self, si, varE):                                            # functions.jl:421-486
        M, beta, vb = self.M[si], self.beta[si], self.varBeta[si]
        var_var = M["varZeta"][0]
        iVarE = 1.0 / varE
        for r, theseLoci in enumerate(M["regionArray"]):
            for locus in theseLoci:
                self.ycorr += beta[locus] * M["data"][:, locus]                                   # :432
                rhs = np.dot(M["Mp"][locus], self.ycorr) * iVarE + M["rhs"][locus]                # :433
                lhs = M["mpm"][locus] * iVarE + M["lhs"][locus] + 1.0 / vb[locus]                 # :434
                meanBeta = rhs / lhs
                beta[locus] = self.sampleBeta(si, locus, meanBeta, lhs)                           # :436
                self.ycorr += -1.0 * beta[locus] * M["data"][:, locus]                            # :437
        if self.blocked_step:
            mode = 0 if M["estVarZeta"] is False else 1 if M["estVarZeta"] is True else 2
            v2, c, z, vz, tr = lv_step_blocked(self.O, self.seed, self.chain, self.iter, si, beta, vb, M["SNPVARRESID"], M["covariates"], M["iCpC"],
                                               var_var, mode, 0.0 if mode != 2 else float(M["estVarZeta"]))
            vb[:] = v2; M["logVar"][:] = np.log(v2); M["c"][:] = c; M["SNPVARRESID"][:] = z; M["varZeta"][0] = vz; M["trapped"] = tr
            return
        trapped = 0
        with np.errstate(divide="ignore", over="ignore", invalid="ignore"):
            for r, theseLoci in enumerate(M["regionArray"]):
                for locus in theseLoci:
                    u = self.O.draws(self.seed, self.chain, self.iter, KIND_LV_UNIFORM, (si << 40) | locus, 0, 4)   # the four rand() of :455-466
                    vari = np.float64(vb[locus])
                    bi = np.float64(beta[locus])
                    log_vari = M["logVar"][locus]
                    zt = M["SNPVARRESID"][locus]
                    var_mui = log_vari - zt                                                           # :453
                    c1 = vari ** -1.5 * u[0]                                                          # :455
                    c2 = np.exp(-0.5 * bi * bi / vari) * u[1]
                    c3 = np.exp(-0.5 * zt * zt / var_var) * u[2]
                    temp = np.sqrt(-2 * var_var * np.log(c3))
                    lbound = np.exp(var_mui - temp)
                    rbound = np.exp(var_mui + temp)
                    if np.exp((-2 / 3) * np.log(c1)) < rbound:                                        # :461
                        rbound = np.exp((-2 / 3) * np.log(c1))
                    if -0.5 * bi * bi / np.log(c2) > lbound:                                          # :462
                        lbound = -0.5 * bi * bi / np.log(c2)
                    if lbound >= rbound:
                        trapped += 1
                    else:
                        vari = lbound + u[3] * (rbound - lbound)                                      # :467
                        vb[locus] = vari
                        M["logVar"][locus] = np.log(vari)
        M["trapped"] = trapped
        rhsC = M["covariatesT"] @ M["logVar"]                                                         # :475
        meanC = M["iCpC"] @ rhsC
        S = M["iCpC"] * var_var
        z = np.array([float(self.O.draws(self.seed, self.chain, self.iter, KIND_LV_NORMAL, (si << 40) | k, 1, 1)[0]) for k in range(len(meanC))])
        M["c"][:] = meanC + np.linalg.cholesky((S + S.T) / 2) @ z                                     # :477 rand(MvNormal(mean, Symmetric(S)))
        M["SNPVARRESID"][:] = M["logVar"] - M["covariates"] @ M["c"]                                  # :478
        if isinstance(M["estVarZeta"], float):                                                        # :481-485
            M["varZeta"][0] = M["estVarZeta"] * np.var(M["logVar"], ddof=1)
        elif M["estVarZeta"] is True:
            M["varZeta"][0] = np.var(M["SNPVARRESID"], ddof=1)

    def run(self, niter):                                                          # samplers.jl:29-53
        for _ in range(niter):
            self.iter += 1
            varE = self.sampleVarE()
            self.varE = varE
            if self.intercept:
                self.sampleX(varE)
            for f in range(len(getattr(self, "Xfix", []))):
                self.sampleXset(f, varE)
            for si, M in enumerate(self.M):
                {0: self.sampleBayesPR, 1: self.sampleBayesB, 2: self.sampleBayesC, 3: self.sampleBayesR, 5: self.sampleBayesLV}[M["method"]](si, varE)
