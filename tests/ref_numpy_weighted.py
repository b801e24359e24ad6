"""Weighted residuals (E.str == "D") in the reference's own order (TEST INFRASTRUCTURE): ref_numpy.RefChain with what D changes.

Written from the Julia source, not from the device code:

    /root/reference/src/mme.jl:71-75           E.iVarStr = inv.(d): the weights w
    /root/reference/src/functions.jl:526-528   sampleVarE(E, ycorr, n) = (df scale + sum(w ycorr^2)) / chi2(df + n)   (samplers.jl:32-35)
    /root/reference/src/mme.jl:299-303         Mp[j] = (x_j .* w)', mpm[j] = sum(x_j w x_j)
    /root/reference/src/mme.jl:133-136         fixed sets: Xp = (X .* w)', xpx = X'(w .* X) (+ the ridge of :149-152); the intercept is the
                                               fixed set of a ones column: Xp = w', xpx = sum(w)

ycorr stays unscaled and its updates unweighted (ycorr -= x_j dbeta), as in the reference.  One deliberate departure: the inclusion
statistic of BayesB / BayesC (functions.jl:168, :209) is written there as data'ycorr; under D this restatement uses Mp[j] ycorr =
x_j'W ycorr, the statistic whose variance the v0 / v1 of the same lines describe (mpm is x'Wx under D).  The library samples the
row-scaled problem, where that is the only statistic there is ("Weighted residuals").
"""
import math

import numpy as np

from ref_numpy import RefChain


class WeightedRefChain(RefChain):
    def __init__(self, O, X, y, w, seed, chain, intercept=True):
        super().__init__(O, X, y, seed, chain, intercept=intercept)
        self.w = np.asarray(w, dtype=np.float64)                                                  # E.iVarStr

    def add_set(self, col0, ncol, method, df, scale, regions, varBeta0, pi0=0.0, estPi=False, lhs=None, rhs=None):
        super().add_set(col0, ncol, method, df, scale, regions, varBeta0, pi0=pi0, estPi=estPi, lhs=lhs, rhs=rhs)
        M = self.M[-1]
        M["Mp"] = [M["data"][:, j] * self.w for j in range(ncol)]                                 # mme.jl:302
        M["mpm"] = [float(np.sum(M["data"][:, j] * self.w * M["data"][:, j])) for j in range(ncol)]  # mme.jl:299-301

    def sampleVarE(self):                                                                         # functions.jl:526-528
        return (self.E_df * self.E_scale + np.sum(self.w * self.ycorr ** 2)) / self.draw("VARE_CHI2", 0, 2, self.E_df + self.N)

    def sampleX(self, varE):                                                                      # functions.jl:39-47, Xp = w', xpx = sum(w)
        iVarE = 1.0 / varE
        self.ycorr += self.ones * self.b[0]
        rhs = np.dot(self.w, self.ycorr) * iVarE + 0.0
        lhs = float(np.sum(self.w)) * iVarE + 0.0
        self.b[0] = rhs / lhs + math.sqrt(1.0 / lhs) * self.draw("FIXED_NORMAL", 0, 1)
        self.ycorr -= self.ones * self.b[0]

    def add_fixed(self, X, lhs=None, rhs=None):                                                   # mme.jl:133-136, 149-152
        super().add_fixed(X, lhs=lhs, rhs=rhs)
        F = self.Xfix[-1]
        X = F["data"]
        xpx = X.T @ (self.w[:, None] * X)
        if F["nCol"] > 1:
            xpx = xpx + np.eye(F["nCol"]) * (np.abs(np.diag(xpx)) / 10000).min()
        F["Xp"] = (X * self.w[:, None]).T.copy()
        F["xpx"] = xpx

    def _inclusion(self, si, locus, rrr, varE, vbeta):                                            # functions.jl:168 / :209 under D
        rrr = np.dot(self.M[si]["Mp"][locus], self.ycorr)
        return super()._inclusion(si, locus, rrr, varE, vbeta)
