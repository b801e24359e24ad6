"""APY GBLUP (TEST INFRASTRUCTURE): plain fp64 numpy written from the formulas of the APY form (include/nextgp_hip.h, "GBLUP at scale"),
not from the HIP code.  Levels are numbered core first.

    Kc0 = inv(Gcc);  P = Gnc Kc0;  m_i = g_ii - P_i. (Gnc)_i.;  d = 1 / m;  Kcc = Kc0 + P' diag(d) P;  K_APY = [Kcc, -P'D; -DP, D]

Every function returns, beside each quantity, a forward-error bound by ONE rule: the quantity's own expression evaluated on absolute
values (its operands, as computed, replaced by their absolute values, every subtraction by a sum, an inverse by the absolute values of
its entries; no bound of an operand is carried into the next quantity) times gamma(n) = n eps / (1 - n eps), n the number of terms
of the longest sum feeding it.  A comparison to rounding uses TOL = 4 x the bound: the factor covers the two or three chained sums
between an input and an output.  Nothing here is tuned to what the device gives.
"""
import numpy as np

from ref_gblup import make_g
from ref_random import KIND_U_CHI2, KIND_U_NORMAL, draw, level_records

EPS = 2.0 ** -53
TOL = 4.0


def gamma(n):
    return n * EPS / (1.0 - n * EPS)


def pieces(M, nc, method=1):
    """The APY form of make_g(M) with the first nc animals as the core: {"P", "m", "d", "Kc0", "Kcc"} and the bounds {"bP", "bm", "bKcc"}.
    Absolute G: |Xc| |Xc|' / denom + ridge (make_g's second result).  The longest sum runs over the SNPs, the core or the other animals."""
    N, nsnp = M.shape
    G, aG = make_g(M, method)
    aG = aG + 0.001 * np.eye(N)
    Gcc, Gnc, g = G[:nc, :nc], G[nc:, :nc], np.diag(G)[nc:]
    Kc0 = np.linalg.inv(Gcc)
    Kc0 = (Kc0 + Kc0.T) / 2.0
    P = Gnc @ Kc0
    m = g - np.sum(P * Gnc, axis=1)
    d = 1.0 / m
    Kcc = Kc0 + P.T @ (d[:, None] * P)
    gm = gamma(max(nsnp, nc, N - nc) + 2)
    aK, aGnc = np.abs(Kc0), aG[nc:, :nc]
    aP = aGnc @ aK
    am = np.diag(aG)[nc:] + np.sum(aP * aGnc, axis=1)
    aKcc = aK + aP.T @ (np.abs(d)[:, None] * aP)
    return dict(P=P, m=m, d=d, Kc0=Kc0, Kcc=Kcc, bP=gm * aP, bm=gm * am, bKcc=gm * aKcc)


def assemble(pc):
    """K_APY as a dense, exactly symmetric N x N matrix."""
    P, d, Kcc = pc["P"], pc["d"], pc["Kcc"]
    off = -(d[:, None] * P)
    return np.block([[Kcc, off.T], [off, np.diag(d)]])


def step(O, seed, chain, it, rset, yt, rs, level, pc, zpz, u, varU, varE, df, scale):
    """One step of sampleU over K_APY in level order from the pieces pc (exact inputs), with the keyed draws every random set uses.  yt is
    the device's residual (y~ = s ycorr under weights, rs = s; else ycorr, rs None); level None: the identity incidence.  Returns a dict
    of u, s (the seed of the NEXT sweep), uKu, yt, varU and of their bounds bu, bs, buKu, byt, bvarU (a...: the absolute counterpart of each
    quantity's own expression).  The sums of a level have at most q + 2 terms, whichever way they are split between seed, chain and
    tail: gamma(q + 2) serves all of them (and a dense set over assemble(pc))."""
    P, d, Kc0, Kcc = pc["P"], pc["d"], pc["Kc0"], pc["Kcc"]
    nn, nc = P.shape
    q = nc + nn
    yt, u, zpz = np.array(yt, dtype=np.float64), np.array(u, dtype=np.float64), np.asarray(zpz, dtype=np.float64)
    level = np.arange(len(yt)) if level is None else np.asarray(level, dtype=np.int64)
    iVarE, iVarU, g = 1.0 / varE, 1.0 / varU, gamma(q + 2)
    term = yt * rs if rs is not None else yt
    recs = level_records(level, q)
    Yi = (np.array([term[r].sum() for r in recs]) + zpz * u) * iVarE
    aYi = (np.array([np.abs(term[r]).sum() for r in recs]) + np.abs(zpz * u)) * iVarE
    kd = np.concatenate([np.diag(Kcc), d])
    inv = 1.0 / (zpz * iVarE + kd * iVarU)
    z = O.draws(seed, chain, it, KIND_U_NORMAL, (rset << 40), 1, q, 0.0, 0.0, indexed=True)
    tz = np.sqrt(inv) * z
    aP, aKcc, aK0 = np.abs(P), np.abs(Kcc), np.abs(Kc0)
    s0 = -(P.T @ (d * u[nc:]))
    as0 = aP.T @ np.abs(d * u[nc:])
    un, au = u.copy(), np.zeros(q)
    for l in range(nc):                                                 # the core, in level order: new values left of l, old ones right
        row, arow = Kcc[l].copy(), aKcc[l].copy()
        row[l] = arow[l] = 0.0
        un[l] = inv[l] * (Yi[l] - (s0[l] + row @ un[:nc]) * iVarU) + tz[l]
        au[l] = inv[l] * (aYi[l] + (as0[l] + arow @ np.abs(un[:nc])) * iVarU) + np.abs(tz[l])
    v, av = P @ un[:nc], aP @ np.abs(un[:nc])
    un[nc:] = inv[nc:] * (Yi[nc:] + iVarU * d * v) + tz[nc:]
    au[nc:] = inv[nc:] * (aYi[nc:] + iVarU * d * av) + np.abs(tz[nc:])
    s, as_ = -(P.T @ (d * un[nc:])), aP.T @ np.abs(d * un[nc:])
    e, ae = un[nc:] - v, np.abs(un[nc:]) + av
    uKu = un[:nc] @ Kc0 @ un[:nc] + np.sum(d * e * e)
    auKu = np.abs(un[:nc]) @ aK0 @ np.abs(un[:nc]) + np.sum(d * ae * ae)
    t, at = (un - u)[level], (np.abs(un) + np.abs(u))[level]
    if rs is not None:
        t, at = rs * t, rs * at
    chi = draw(O, seed, chain, it, KIND_U_CHI2, rset, 2, df + q)
    return dict(u=un, s=s, uKu=float(uKu), yt=yt - t, varU=float((scale * df + uKu) / chi), bu=g * au, bs=g * as_, buKu=float(g * auKu),
                byt=g * (np.abs(yt) + at), bvarU=float(g * (scale * df + auKu) / chi))
