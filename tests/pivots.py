"""The laws of the sampler's draws, and nothing else (TEST INFRASTRUCTURE).

Given a model's inputs and two consecutive chain states -- before and after ONE iteration -- `pivots()` returns, for every draw the
iteration made, a number that is N(0,1) or U(0,1) under a correct sampler, given everything drawn before it.  Nothing here knows
how a draw is produced: no generator, no key, no kind number, nothing from oracle/, tests/ref_*.py or the library.  numpy float64
and scipy.stats only.  A chain whose draws reuse a number, lack a term of a conditional or take a wrong degree of freedom shows up
as pivots that are not iid; bit-for-bit twins written from one draw spec cannot see that.

The walk follows the reference's iteration (/root/reference/src/samplers.jl:29-53): varE, the intercept and the fixed sets, the
random-effect sets, the marker sets with their variance and pi draws.  It rebuilds ycorr as it goes, at every draw with the new
values of what was already drawn and the old values of the rest, and at the end asserts that its ycorr is the after-state's to
1e-8 relative: otherwise the walk is wrong and the pivots mean nothing.

Conditionals, from /root/reference/src/functions.jl (quirks included):

  varE            :523-528   (df scale + sum w ycorr^2) / chi2(df + N)
  fixed effects   :22-53     one column: rhs = x'W ycorr / varE, lhs = x'W x / varE.  Several columns: Gauss-Seidel over
                             xpx = X'WX + min(|diag|)/10000 I (mme.jl:149-152) -- the ridge is the reference's, kept
  random sets     :57-72, 92-97, 498-501   Gauss-Seidel over the levels, K = Z.iVarStr (identity, diagonal, pedigree A^-1, inv(G)),
                             Z'Z diagonal (Z is one-hot), varU = (df scale + u'Ku) / chi2(df + q)
  tuple random    DESIGN.md "Correlated random-effect sets": the device draws the EXACT conditional of a level's k effects,
                             precision W_ll / varE + K_ll inv(varU), every other level (linked by K or by a shared record) at its
                             current value -- a documented departure from :75-89, which the pivot follows; varU inverse-Wishart
  BayesPR         :118-137   lhs = mpm / varE + 1 / varBeta[region]; region variance (df scale + sum beta^2) / chi2(df + size)
  Tuple BayesPR   :140-154, 513-516   MvNormal(inv(LHS) RHS, inv(LHS)), LHS = X_l'X_l / varE + inv(varBeta[region]); inverse-Wishart
  BayesB          :157-195   inclusion by probDelta1 (:169-174); an excluded locus sets varBeta = 0 (:186), so on re-entry
                             1 / varBeta = Inf, lhs = Inf and beta = 0 exactly: no normal pivot there (asserted), the locus
                             variance (df scale + beta^2) / chi2(df + 1) follows.  A monomorphic column has mpm = 0,
                             probDelta1 = NaN, the comparison is false: asserted excluded, no pivot
  BayesC          :197-235   as B with one variance; rhs WITHOUT M.rhs (:220); variance chi2(df + nIn); pi Beta(nIn + 1, P - nIn + 1)
  BayesR          :238-289   class by findfirst(x -> x >= rand(), cumsum(probs)) with a FRESH uniform per comparison (:261): the law is
                             the sequential P(v) = c_v prod_{u<v} (1 - c_u), c = cumsum(probs), not probs; variance from
                             sumS = sum beta^2 / vClass, chi2(df + nNonZero); pi Dirichlet(nLoci + 1) (:536-538)
  weights         mme.jl:71-75, 133-136, 299-303: w enters x'W ycorr, x'W x and sum w ycorr^2; B / C form the inclusion statistic as
                  x'W ycorr (DESIGN.md "Weighted residuals")

Left out: BayesLV's slice draw of a locus' log-variance (:455-466) has no one-step pivot (a slice sampler's transition law is
not a closed-form CDF of the new value), and its regression normals (:477) are not covered either.

`wrong` names deliberately wrong laws (the power checks of tests/test_pivots_host.py): a test that cannot fail is worth nothing.
"""
import numpy as np
from scipy import stats

WRONG = ("drop_ivarbeta", "nu_plus_one", "probs_class", "dirichlet_a", "iw_nu", "iw_stale", "k_identity", "fixed_no_gs", "incl_no_prior",
         "beta_a", "vare_unweighted")
NORMAL = ("z_fixed", "z_random", "z_marker", "iw_off")
UNIFORM = ("chi2_varE", "chi2_region", "chi2_locus", "chi2_varU", "iw_diag", "pit_incl", "pit_class", "pi_beta", "pi_dirichlet")


class Out:
    """family -> values in draw order; for the normal families also the site (a draw's fixed place in the model) of each value."""

    def __init__(self):
        self.v = {}
        self.site = {}

    def add(self, fam, value, site=-1):
        self.v.setdefault(fam, []).append(float(value))
        self.site.setdefault(fam, []).append(int(site))


def _chi2_pivot(out, fam, num, v_new, nu, wrong):
    out.add(fam, stats.chi2.cdf(num / v_new, nu + (1.0 if "nu_plus_one" in wrong else 0.0)))


def _pit(out, fam, F_lo, F_hi, rng):
    out.add(fam, F_lo + rng.random() * (F_hi - F_lo))


def _mv_pivot(out, fam, x_new, mean, cov, site0):
    """k components of chol(cov)^-1 (x_new - mean)."""
    L = np.linalg.cholesky((cov + cov.T) / 2.0)
    for a, z in enumerate(np.linalg.solve(L, x_new - mean)):
        out.add(fam, z, site0 + a)


def _iw_pivot(out, V_new, Psi, nu, wrong, site0):
    """Bartlett: W = inv(V_new) ~ Wishart(nu, inv(Psi)); A = chol(inv(Psi))^-1 chol(W) is lower with A_ii^2 ~ chi2(nu - i) and
    A_ij ~ N(0,1), i > j.  This does not depend on how the sampler builds the draw."""
    k = Psi.shape[0]
    L = np.linalg.cholesky(np.linalg.inv(Psi))
    Cw = np.linalg.cholesky(np.linalg.inv((V_new + V_new.T) / 2.0))
    A = np.linalg.solve(L, Cw)
    for i in range(k):
        for j in range(i):
            out.add("iw_off", A[i, j], site0 + i * k + j)
        out.add("iw_diag", stats.chi2.cdf(A[i, i] ** 2, nu - (0 if "iw_nu" in wrong else i) + (1.0 if "nu_plus_one" in wrong else 0.0)))


def sequential_class_law(probs):
    """P(class = v) of findfirst(x -> x >= rand(), cumsum(probs)) with a fresh uniform per comparison (functions.jl:259-261); the
    last class also takes what falls through."""
    c = np.minimum(np.cumsum(probs), 1.0)
    law = c * np.concatenate([[1.0], np.cumprod(1.0 - c[:-1])])
    law[-1] = max(1.0 - law[:-1].sum(), 0.0)
    return law


def pivots(model, s0, s1, rng, wrong=()):
    """model: dict(X [N, P] float64, w [N] or None, E_df, E_scale, intercept, fixed [list of N x c], random [list of dict(levels k x N
    with -1 = none, q, K dense q x q or None, df, scale (scalar, or k x k for k > 1))], sets [list of dict(method 'PR'|'B'|'C'|'R'|'T',
    col0, ncol, df, scale, regions, estPi, vClass, cols [nloc, k])]).
    s0, s1: dict(ycorr, varE, b, fixed [list], u [list of q x k], varU [list of k x k], beta [P], delta [P], varBeta [list per set],
    pi [list per set: (1 - pi, pi) or the class probabilities]).  rng: numpy generator of the randomized PITs.  Returns Out."""
    assert all(x in WRONG for x in wrong)
    out = Out()
    X = model["X"]
    N = X.shape[0]
    w = np.ones(N) if model.get("w") is None else np.asarray(model["w"], dtype=np.float64)
    yc = np.array(s0["ycorr"], dtype=np.float64)

    # ---- varE (functions.jl:523-528) ----
    varE = float(s1["varE"])
    ss = float(np.sum((1.0 if "vare_unweighted" in wrong else w) * yc * yc))
    _chi2_pivot(out, "chi2_varE", model["E_df"] * model["E_scale"] + ss, varE, model["E_df"] + N, wrong)

    # ---- intercept and fixed sets (functions.jl:22-53) ----
    site = 0
    if model.get("intercept", True):
        yc += s0["b"]
        lhs = w.sum() / varE
        out.add("z_fixed", (s1["b"] - (np.dot(w, yc) / varE) / lhs) * np.sqrt(lhs), site)
        yc -= s1["b"]
    site += 1
    for f, F in enumerate(model.get("fixed", [])):
        F = np.asarray(F, dtype=np.float64).reshape(N, -1)
        c = F.shape[1]
        b0, b1 = np.asarray(s0["fixed"][f], dtype=np.float64), np.asarray(s1["fixed"][f], dtype=np.float64)
        xpx = F.T @ (w[:, None] * F)
        if c > 1:
            xpx = xpx + np.eye(c) * (np.abs(np.diag(xpx)) / 10000.0).min()      # mme.jl:149-152
        yc += F @ b0
        Yi = F.T @ (w * yc) / varE
        bVec = b0.copy()
        for i in range(c):
            bVec[i] = 0.0
            rhs = Yi[i] - (0.0 if "fixed_no_gs" in wrong else np.dot(xpx[i], bVec) / varE)
            lhs = xpx[i, i] / varE
            out.add("z_fixed", (b1[i] - rhs / lhs) * np.sqrt(lhs), site + i)
            bVec[i] = b1[i]
        yc -= F @ b1
        site += c

    # ---- random-effect sets (functions.jl:57-97; tuple sets: the exact conditional of DESIGN.md) ----
    site = 0
    for r, R in enumerate(model.get("random", [])):
        lev = np.atleast_2d(np.asarray(R["levels"]))
        k, q = lev.shape[0], R["q"]
        K = np.eye(q) if (R.get("K") is None or "k_identity" in wrong) else np.asarray(R["K"], dtype=np.float64)
        u0 = np.asarray(s0["u"][r], dtype=np.float64).reshape(q, k)
        u1 = np.asarray(s1["u"][r], dtype=np.float64).reshape(q, k)
        Si = np.linalg.inv(np.asarray(s0["varU"][r], dtype=np.float64).reshape(k, k))
        recs = [[np.nonzero(lev[a] == l)[0] for l in range(q)] for a in range(k)]
        u = u0.copy()
        for l in range(q):
            for a in range(k):
                yc[recs[a][l]] += u[l, a]                      # take this level's own effects out of the residual
            Wll = np.zeros((k, k))
            rhs = np.zeros(k)
            for a in range(k):
                ia = recs[a][l]
                rhs[a] = np.dot(w[ia], yc[ia]) / varE
                for b in range(k):
                    Wll[a, b] = w[ia][lev[b][ia] == l].sum()
            Kl = K[l].copy()
            Kl[l] = 0.0
            rhs -= Si @ (Kl @ u)                               # the couplings K_lc inv(varU) u_c, c != l, at their current values
            cov = np.linalg.inv(Wll / varE + K[l, l] * Si)
            _mv_pivot(out, "z_random", u1[l], cov @ rhs, cov, site + l * k)
            u[l] = u1[l]
            for a in range(k):
                yc[recs[a][l]] -= u[l, a]
        site += q * k
        S = u1.T @ np.asarray(K) @ u1
        V1 = np.asarray(s1["varU"][r], dtype=np.float64).reshape(k, k)
        if k == 1:
            _chi2_pivot(out, "chi2_varU", R["df"] * R["scale"] + S[0, 0], V1[0, 0], R["df"] + q, wrong)
        else:
            if "iw_stale" in wrong:
                S = u0.T @ np.asarray(K) @ u0
            _iw_pivot(out, V1, np.asarray(R["scale"], dtype=np.float64).reshape(k, k) + S, R["df"] + q, wrong, 16 * r)

    # ---- marker sets ----
    beta0, beta1 = np.asarray(s0["beta"], dtype=np.float64), np.asarray(s1["beta"], dtype=np.float64)
    delta1 = np.asarray(s1["delta"])
    keep = 0.0 if "drop_ivarbeta" in wrong else 1.0
    for si, M in enumerate(model["sets"]):
        meth, col0, df, scale = M["method"], M["col0"], M["df"], M["scale"]
        vb0, vb1 = np.asarray(s0["varBeta"][si], dtype=np.float64), np.asarray(s1["varBeta"][si], dtype=np.float64)
        pi0 = None if s0["pi"][si] is None else np.asarray(s0["pi"][si], dtype=np.float64)

        def locus(col):
            x = X[:, col]
            xw = x * w
            yc[:] += beta0[col] * x
            return x, float(np.dot(xw, yc)), float(np.dot(xw, x))

        def normal(col, x, rhs, lhs):
            out.add("z_marker", (beta1[col] - rhs / lhs) * np.sqrt(lhs), col)
            yc[:] -= beta1[col] * x

        if meth == "PR":                                                         # :118-137
            for r, (a, b) in enumerate(M["regions"]):
                for col in range(col0 + a, col0 + b):
                    x, xy, mpm = locus(col)
                    normal(col, x, xy / varE, mpm / varE + keep / vb0[r])
                ss = float(np.sum(beta1[col0 + a:col0 + b] ** 2))
                _chi2_pivot(out, "chi2_region", scale * df + ss, vb1[r], df + (b - a), wrong)
        elif meth == "T":                                                        # :140-154, 513-516
            cols = np.asarray(M["cols"])
            k = cols.shape[1]
            vb0, vb1 = vb0.reshape(-1, k, k), vb1.reshape(-1, k, k)
            for r, (a, b) in enumerate(M["regions"]):
                invB = np.linalg.inv(vb0[r])
                for l in range(a, b):
                    Xl = X[:, cols[l]]
                    yc += Xl @ beta0[cols[l]]
                    cov = np.linalg.inv(Xl.T @ (w[:, None] * Xl) / varE + keep * invB)
                    _mv_pivot(out, "z_marker", beta1[cols[l]], cov @ (Xl.T @ (w * yc) / varE), cov, int(cols[l, 0]))
                    yc -= Xl @ beta1[cols[l]]
                Bm = (beta0 if "iw_stale" in wrong else beta1)[cols[a:b]]
                _iw_pivot(out, vb1[r], np.asarray(scale, dtype=np.float64).reshape(k, k) + Bm.T @ Bm, df + (b - a), wrong, 16 * (1000 * (si + 1) + r))
        elif meth in ("B", "C"):                                                 # :157-235
            nIn = 0
            lp = np.zeros(2) if "incl_no_prior" in wrong else np.log(pi0)
            for j in range(M["ncol"]):
                col = col0 + j
                vb = vb0[j] if meth == "B" else vb0[0]
                x, rrr, mpm = locus(col)
                if mpm == 0.0:                                                   # probDelta1 = NaN: excluded, no pivot
                    assert delta1[col] == 0 and beta1[col] == 0.0
                    continue
                v0 = mpm * varE
                v1 = mpm * mpm * vb + v0
                d = (-0.5 * (np.log(v0) + rrr * rrr / v0) + lp[0]) - (-0.5 * (np.log(v1) + rrr * rrr / v1) + lp[1])
                p1 = 1.0 / (1.0 + np.exp(min(d, 700.0)))
                inc = int(delta1[col]) == 1
                _pit(out, "pit_incl", 1.0 - p1 if inc else 0.0, 1.0 if inc else 1.0 - p1, rng)
                if not inc:
                    assert beta1[col] == 0.0 and (meth == "C" or vb1[j] == 0.0)
                    continue
                nIn += 1
                if vb == 0.0:                                                    # BayesB re-entry: lhs = Inf, beta = 0 exactly
                    assert meth == "B" and beta1[col] == 0.0
                else:
                    normal(col, x, rrr / varE, mpm / varE + keep / vb)
                if meth == "B":
                    _chi2_pivot(out, "chi2_locus", scale * df + beta1[col] ** 2, vb1[j], df + 1.0, wrong)
            if meth == "C":
                ss = float(np.sum(beta1[col0:col0 + M["ncol"]] ** 2))
                _chi2_pivot(out, "chi2_region", scale * df + ss, vb1[0], df + nIn, wrong)
            if M.get("estPi"):
                a, b = nIn + 1.0, M["ncol"] - nIn + 1.0
                if "beta_a" in wrong:
                    a, b = a - 1.0, b - 1.0
                if a > 0.0 and b > 0.0:
                    out.add("pi_beta", stats.beta.cdf(s1["pi"][si][1], a, b))
        elif meth == "R":                                                        # :238-289
            vC = np.asarray(M["vClass"], dtype=np.float64)
            Kc = len(vC)
            varc = vb0[0] * vC
            nz = varc != 0.0
            nLoci = np.zeros(Kc)
            sumS, nNonZero = 0.0, 0
            logPi = np.log(pi0)
            for j in range(M["ncol"]):
                col = col0 + j
                x, xy, mpm = locus(col)
                rhs = xy / varE
                lhs = np.where(nz, mpm / varE + keep / np.where(nz, varc, 1.0), 1.0)
                logL = np.where(nz, -0.5 * (np.log(np.where(nz, varc, 1.0) * lhs) - rhs * rhs / lhs), 0.0) + logPi
                probs = np.exp(logL - logL.max())
                probs /= probs.sum()
                law = probs if "probs_class" in wrong else sequential_class_law(probs)
                F = np.concatenate([[0.0], np.cumsum(law)])
                F[-1] = 1.0
                v = int(delta1[col]) - 1
                _pit(out, "pit_class", F[v], F[v + 1], rng)
                nLoci[v] += 1
                if nz[v]:
                    nNonZero += 1
                    normal(col, x, rhs, lhs[v])
                    sumS += beta1[col] ** 2 / vC[v]
                else:
                    assert beta1[col] == 0.0
            _chi2_pivot(out, "chi2_region", scale * df + sumS, vb1[0], df + nNonZero, wrong)
            if M.get("estPi"):
                a = nLoci + (0.0 if "dirichlet_a" in wrong else 1.0)
                p = np.asarray(s1["pi"][si], dtype=np.float64)
                for v in range(Kc - 1):
                    rest = a[v + 1:].sum()
                    if a[v] > 0.0 and rest > 0.0:
                        out.add("pi_dirichlet", stats.beta.cdf(p[v] / (1.0 - p[:v].sum()), a[v], rest))
        else:
            raise ValueError(meth)

    ref = np.asarray(s1["ycorr"], dtype=np.float64)
    err = np.abs(yc - ref).max() / max(np.abs(ref).max(), 1e-300)
    assert err <= 1e-8, f"the walk's ycorr is not the after-state's (relative {err:.3g}): the pivots mean nothing"
    return out


def pool(outs):
    """Out of every iteration -> family -> (values [n], site [n], iteration [n])."""
    res = {}
    for t, o in enumerate(outs):
        for fam, v in o.v.items():
            a = res.setdefault(fam, ([], [], []))
            a[0].extend(v); a[1].extend(o.site[fam]); a[2].extend([t] * len(v))
    return {f: (np.array(a[0]), np.array(a[1]), np.array(a[2])) for f, a in res.items()}


def ks_p(fam, values):
    return float(stats.kstest(values, "norm" if fam in NORMAL else "uniform").pvalue)


def lag1_draw_order(values):
    """(r, n): correlation of consecutive pivots in draw order."""
    return float(np.corrcoef(values[:-1], values[1:])[0, 1]), len(values) - 1


def lag1_per_site(values, site, it):
    """(r, n): correlation of a site's pivot with the same site's pivot one iteration later, pooled over the sites."""
    key = site.astype(np.int64) * (int(it.max()) + 2) + it
    order = np.argsort(key, kind="stable")
    k, v = key[order], values[order]
    pair = np.nonzero(k[1:] == k[:-1] + 1)[0]
    if len(pair) < 3:
        return 0.0, 0
    return float(np.corrcoef(v[pair], v[pair + 1])[0, 1]), len(pair)
