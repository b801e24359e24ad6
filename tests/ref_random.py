"""(1|g) random-effect sets (TEST INFRASTRUCTURE): two restatements, written from the Julia source and from DESIGN.md, not from the HIP code.

    /root/reference/src/functions.jl:57-72    sampleU(::Symbol): Yi = Z'ycorr / varE, Gauss-Seidel over iVarStr, Z'Z taken as diagonal
    /root/reference/src/functions.jl:92-97    sampleZ!(::Symbol): ycorr += Z u, sampleU, ycorr -= Z u, sampleVarU
    /root/reference/src/functions.jl:498-501  sampleVarU = (scale df + u K u') / chi2(df + q)
    /root/reference/src/samplers.jl:43-46     random-effect sets after the fixed effects, before the marker sets
    /root/reference/src/mme.jl:165-272        zpz, df = 3 + 1, scale = v (df - 2) / df

RandomRefChain is the reference's order on top of ref_numpy.RefChain (numpy dots: agreement to rounding).  random_step_blocked is the
device's documented order of ONE random step ("Random-effect sets") in plain Python loops: bit for bit what
ngp_sample_random_set computes.  The random step has no FMA, so every operation below is one IEEE double operation.  Draws come
from oracle.draws on the new kinds 12 (normal of level l of set r: key (r << 40) | l) and 13 (chi-square of varU: key r).
"""
import math

import numpy as np

from ref_numpy import RefChain

KIND_U_NORMAL, KIND_U_CHI2 = 12, 13


def draw(O, seed, chain, it, kind, index, what, p1=0.0):
    return float(O.draws(seed, chain, it, kind, index, what, 1, p1, 0.0, indexed=True)[0])


def csr_of(K, q):
    """K (None = identity, or a dense q x q array) as rows of (column, value), columns ascending."""
    if K is None:
        return [[(l, 1.0)] for l in range(q)]
    K = np.asarray(K, dtype=np.float64)
    return [[(int(c), float(K[l, c])) for c in np.nonzero(K[l])[0]] for l in range(q)]


def level_records(level, q):
    recs = [[] for _ in range(q)]
    for i, l in enumerate(level):
        recs[int(l)].append(i)
    return recs


def zpz_of(level, q, w=None):
    """zpz_l: the record count, or the sum of w over the level's records in ascending record order (weighted residuals)."""
    out = []
    for r in level_records(level, q):
        if w is None:
            out.append(float(len(r)))
        else:
            a = 0.0
            for i in r:
                a = a + float(w[i])
            out.append(a)
    return out


def _butterfly(v):
    """acc = acc + shfl_xor(acc, off), off = 32 .. 1, over 64 lanes; every lane ends with the same value, lane 0's is returned."""
    v = list(v)
    off = 32
    while off >= 1:
        v = [v[j] + v[j ^ off] for j in range(64)]
        off >>= 1
    return v[0]


def random_step_blocked(O, seed, chain, it, rset, yt, rs, level, q, K, zpz, u, varU, varE, df, scale):
    """One random step in the device's order.  yt: the device's residual (y~ = s ycorr under weights, rs = s; else ycorr, rs None).
    Returns (yt, u, varU) new; inputs are not changed."""
    yt = [float(x) for x in yt]
    u = [float(x) for x in u]
    rows = csr_of(K, q)
    recs = level_records(level, q)
    offdiag = any(c != l for l in range(q) for c, _ in rows[l])
    iVarE = 1.0 / varE
    iVarU = 1.0 / varU
    Yi, inv, tz, dhi, du = [0.0] * q, [0.0] * q, [0.0] * q, [0.0] * q, [0.0] * q
    unew = list(u)
    for l in range(q):
        lanes = [0.0] * 64
        for k, i in enumerate(recs[l]):
            t = rs[i] * yt[i] if rs is not None else yt[i]
            lanes[k % 64] = lanes[k % 64] + t
        acc = _butterfly(lanes)
        tu = zpz[l] * u[l]
        tot = acc + tu
        Yi[l] = tot * iVarE
        t1 = zpz[l] * iVarE
        kd = [v for c, v in rows[l] if c == l][0]
        t2 = kd * iVarU
        lhs = t1 + t2
        inv[l] = 1.0 / lhs
        sd = math.sqrt(inv[l])
        tz[l] = sd * draw(O, seed, chain, it, KIND_U_NORMAL, (rset << 40) | l, 1)
        if not offdiag:
            mean = inv[l] * Yi[l]
            unew[l] = mean + tz[l]
            du[l] = unew[l] - u[l]
        else:
            d = 0.0
            for c, v in rows[l]:
                if c > l:
                    d = d + v * u[c]
            dhi[l] = d
    if offdiag:
        for l in range(q):
            dlo = 0.0
            for c, v in rows[l]:
                if c < l:
                    dlo = dlo + v * unew[c]
            d = dlo + dhi[l]
            t = d * iVarU
            rhs = Yi[l] - t
            mean = inv[l] * rhs
            un = mean + tz[l]
            du[l] = un - unew[l]
            unew[l] = un
    for i in range(len(yt)):
        t = du[level[i]]
        if rs is not None:
            t = rs[i] * t
        yt[i] = yt[i] - t
    thr = [0.0] * 1024
    for l in range(q):
        r = 0.0
        for c, v in rows[l]:
            r = r + v * unew[c]
        thr[l % 1024] = thr[l % 1024] + unew[l] * r
    waves = [_butterfly(thr[64 * w:64 * w + 64]) for w in range(16)]
    quad = waves[0]
    for w in range(1, 16):
        quad = quad + waves[w]
    chi = draw(O, seed, chain, it, KIND_U_CHI2, rset, 2, df + q)
    t = scale * df
    t = t + quad
    return yt, unew, t / chi


class RandomRefChain(RefChain):
    """ref_numpy.RefChain with sampleZ! of every (1|g) set after the fixed-effect sets (src/samplers.jl:43-46)."""

    def add_random(self, level, q, K=None, df=4.0, scale=None, v=100.0):     # mme.jl:165-272
        level = np.asarray(level, dtype=np.int64)
        Z = np.zeros((self.N, q))
        Z[np.arange(self.N), level] = 1.0
        self.Z = getattr(self, "Z", [])
        self.Z.append(dict(data=Z, Zp=Z.T.copy(), zpz=np.array([float(np.dot(c, c)) for c in Z.T]),
                           iVarStr=np.eye(q) if K is None else np.asarray(K, dtype=np.float64), df=df,
                           scale=v * (df - 2.0) / df if scale is None else scale))
        self.u = getattr(self, "u", [])
        self.u.append(np.zeros(q))
        self.varU = getattr(self, "varU", [])
        self.varU.append(float(v))

    def sampleZ(self, r, varE):                                               # functions.jl:92-97
        Zs = self.Z[r]
        self.ycorr += Zs["data"] @ self.u[r]                                  # :93
        uVec = self.u[r].copy()                                               # :57-72
        iVarE, iVarU = 1.0 / varE, 1.0 / self.varU[r]
        Yi = Zs["Zp"] @ self.ycorr * iVarE
        for i in range(len(uVec)):
            uVec[i] = 0.0
            rhsU = Yi[i] - iVarU * np.dot(Zs["iVarStr"][:, i], uVec)
            lhsU = Zs["zpz"][i] * iVarE + Zs["iVarStr"][i, i] * iVarU
            invLhsU = 1.0 / lhsU
            uVec[i] = invLhsU * rhsU + math.sqrt(invLhsU) * self.draw_k(KIND_U_NORMAL, (r << 40) | i, 1)
        self.u[r] = uVec
        self.ycorr -= Zs["data"] @ self.u[r]                                  # :95
        q = len(uVec)
        self.varU[r] = (Zs["scale"] * Zs["df"] + float(uVec @ Zs["iVarStr"] @ uVec)) / self.draw_k(KIND_U_CHI2, r, 2, Zs["df"] + q)  # :498-501

    def draw_k(self, kind, index, what, p1=0.0):
        return draw(self.O, self.seed, self.chain, self.iter, kind, index, what, p1)

    def sampleXset(self, f, varE):
        super().sampleXset(f, varE)
        if f == len(self.Xfix) - 1:                                           # the random sets follow the last fixed-effect set
            self._random(varE)

    def _random(self, varE):
        for r in range(len(getattr(self, "Z", []))):
            self.sampleZ(r, varE)

    def run(self, niter):
        if getattr(self, "Xfix", []):
            return super().run(niter)
        # no fixed-effect set beyond the intercept: sample the random sets right after the intercept (samplers.jl:39-46)
        orig = self.sampleX

        def sampleX_then_random(varE):
            if self.intercept:
                orig(varE)
            self._random(varE)
        intercept = self.intercept
        self.sampleX, self.intercept = sampleX_then_random, True
        try:
            return super().run(niter)
        finally:
            self.sampleX, self.intercept = orig, intercept
