"""Numpy restatement of DESIGN.md section 2, "Normal distribution function" and "Cowles' threshold step": det_pnorm, det_lpdiff, the
proposal, the likelihood terms with their reduction tree, the decision and the adaptation of the proposal SD.  As in ref_liability.py
every function is the sequence of IEEE double operations the device performs (one operation per numpy call, no fused multiply-add;
det_log and det_exp are the oracle's), so a test may ask for equality bit for bit."""
import numpy as np

from ref_liability import INF, Uniforms, f64, tnormal

KIND_THRESHOLD_MH = 24
WG = 1024            # rows of one workgroup of the likelihood kernel
TARGET = f64(0.44)   # acceptance rate the adaptation aims at
LS_MIN, LS_MAX = f64(-20.0), f64(0.0)   # bounds of log sigma under adaptation
SQRT1_2 = f64(0.70710678118654752440)

T = [9.60497373987051638749E0, 9.00260197203842689217E1, 2.23200534594684319226E3, 7.00332514112805075473E3, 5.55923013010394962768E4]
U = [1.0, 3.35617141647503099647E1, 5.21357949780152679795E2, 4.59432382970980127987E3, 2.26290000613890934246E4, 4.92673942608635921086E4]
P = [2.46196981473530512524E-10, 5.64189564831068821977E-1, 7.46321056442269912687E0, 4.86371970985681366614E1, 1.96520832956077098242E2,
     5.26445194995477358631E2, 9.34528527171957607540E2, 1.02755188689515710272E3, 5.57535335369399327526E2]
Q = [1.0, 1.32281951154744992508E1, 8.67072140885989742329E1, 3.54937778887819891062E2, 9.75708501743205489753E2, 1.82390916687909736289E3,
     2.24633760818710981792E3, 1.65666309194161350182E3, 5.57535340817727675546E2]
R = [5.64189583547755073984E-1, 1.27536670759978104416E0, 5.01905042251180477414E0, 6.16021097993053585195E0, 7.40974269950448939160E0,
     2.97886665372100240670E0]
S = [1.0, 2.26052863220117276590E0, 9.39603524938001434673E0, 1.20489539808096656605E1, 1.70814450747565897222E1, 9.60896809063285878198E0,
     3.36907645100081516050E0]


def _horner(c, x):
    r = f64(c[0])
    for ci in c[1:]:
        r = r * x
        r = r + f64(ci)
    return r


def pnorm(O, x):
    """det_pnorm: Phi(x) by the rational error functions of Cephes (after Cody 1969)."""
    x = f64(x)
    if x != x:
        return x
    with np.errstate(all="ignore"):
        z = x * SQRT1_2
        az = np.abs(z)
        if az < 1.0:
            zz = z * z
            num = _horner(T, zz)
            den = _horner(U, zz)
            e = (z * num) / den
            return f64(0.5) + f64(0.5) * e
        q = -(az * az)
        if q < -708.0:
            return f64(1.0) if z > 0.0 else f64(0.0)
        ex = f64(O.det_exp(q))
        if az < 8.0:
            num, den = _horner(P, az), _horner(Q, az)
        else:
            num, den = _horner(R, az), _horner(S, az)
        y = f64(0.5) * ((ex * num) / den)
        return f64(1.0) - y if z > 0.0 else y


def lpdiff(O, a, b):
    """det_lpdiff: log(Phi(b) - Phi(a)), -inf unless a < b and the mass is a positive double."""
    a, b = f64(a), f64(b)
    if not (a < b):
        return -INF
    p = pnorm(O, -a) - pnorm(O, -b) if a >= 0.0 else pnorm(O, b) - pnorm(O, a)
    if not (p > 0.0):
        return -INF
    return f64(O.det_log(p))


def pnorm_v(O, x):
    """pnorm on a vector: the same operations per element (every branch evaluated on the elements that take it)."""
    x = np.asarray(x, dtype=np.float64)
    out = np.empty_like(x)
    with np.errstate(all="ignore"):
        nan = x != x
        out[nan] = x[nan]
        z = x * SQRT1_2
        az = np.abs(z)
        small = ~nan & (az < 1.0)
        zs = z[small]
        zz = zs * zs
        e = (zs * _horner(T, zz)) / _horner(U, zz)
        out[small] = f64(0.5) + f64(0.5) * e
        q = -(az * az)
        under = ~nan & ~small & (q < -708.0)
        out[under] = np.where(z[under] > 0.0, 1.0, 0.0)
        rest = ~nan & ~small & ~under
        a = az[rest]
        ex = np.array([O.det_exp(float(v)) for v in q[rest]], dtype=np.float64)
        mid = a < 8.0
        num = np.where(mid, _horner(P, a), _horner(R, a))
        den = np.where(mid, _horner(Q, a), _horner(S, a))
        y = f64(0.5) * ((ex * num) / den)
        out[rest] = np.where(z[rest] > 0.0, f64(1.0) - y, y)
    return out


def lpdiff_v(O, a, b):
    """lpdiff on vectors: Phi(hi) - Phi(lo) with (lo, hi) = (a, b), or (-b, -a) where a >= 0 (a negation changes no bit)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    out = np.full(a.shape, -INF)
    with np.errstate(all="ignore"):
        ok = a < b
        pos = a >= 0.0
        lo, hi = np.where(pos, -b, a)[ok], np.where(pos, -a, b)[ok]
        p = pnorm_v(O, hi) - pnorm_v(O, lo)
        lg = np.full(p.shape, -INF)
        good = p > 0.0
        lg[good] = [O.det_log(float(v)) for v in p[good]]
        out[ok] = lg
    return out


# ---- Cowles' step ----
def sigma_start(m):
    """Proposal SD of a fresh adapted chain: 1 / sqrt(m), m the augmented rows."""
    return f64(1.0) / np.sqrt(f64(m))


def propose(O, thr, C, sigma, seed, chain, it, draw=None):
    """(g, ok): the proposal g[0..C] from thr[0..C] (thr[0] = -inf, thr[1] = 0, thr[C] = +inf) and whether it is strictly ordered.
    draw(c, a, b) replaces the truncated normal of threshold c (tests force a draw onto its bound with it)."""
    thr = np.asarray(thr, dtype=np.float64)
    sigma = f64(sigma)
    g = thr.copy()
    ok = True
    with np.errstate(all="ignore"):
        for c in range(2, C):
            a = (g[c - 1] - thr[c]) / sigma
            b = (thr[c + 1] - thr[c]) / sigma
            if draw is None:
                z, _ = tnormal(O, Uniforms(O, seed, chain, it, KIND_THRESHOLD_MH, c), a, b)
            else:
                z = f64(draw(c, a, b))
            g[c] = thr[c] + sigma * z
            ok = ok and bool(g[c - 1] < g[c]) and bool(g[c] < thr[c + 1])
    return g, ok


def row_terms(O, thr, g, cls, liab, r_A, varE=1.0, s_A=None):
    """The likelihood term of every augmented row: fit and sd as the augmentation step forms them."""
    cls = np.asarray(cls, dtype=np.int64)
    thr, g = np.asarray(thr, dtype=np.float64), np.asarray(g, dtype=np.float64)
    sde = np.sqrt(f64(varE))
    out = np.zeros(len(cls))
    with np.errstate(all="ignore"):
        t0, t1, g0, g1 = thr[cls - 1], thr[cls], g[cls - 1], g[cls]
        mv = ~((g0 == t0) & (g1 == t1))
        fit = (np.asarray(liab, dtype=np.float64) - np.asarray(r_A, dtype=np.float64))[mv]
        sd = np.full(len(fit), sde) if s_A is None else sde / np.asarray(s_A, dtype=np.float64)[mv]
        new = lpdiff_v(O, (g0[mv] - fit) / sd, (g1[mv] - fit) / sd)
        old = lpdiff_v(O, (t0[mv] - fit) / sd, (t1[mv] - fit) / sd)
        out[mv] = new - old
    return out


def partials(terms):
    """partial[w] of every workgroup: 1024 rows, per wave of 64 the butterfly 32 .. 1, then the 16 wave sums in index order."""
    terms = np.asarray(terms, dtype=np.float64)
    nwg = (len(terms) + WG - 1) // WG
    v = np.zeros(nwg * WG)
    v[:len(terms)] = terms
    out = np.empty(nwg)
    with np.errstate(all="ignore"):
        for w in range(nwg):
            x = v[w * WG:(w + 1) * WG].reshape(16, 64)
            off = 32
            while off >= 1:
                x = x[:, :off] + x[:, off:2 * off]
                off //= 2
            s = f64(x[0, 0])
            for k in range(1, 16):
                s = s + f64(x[k, 0])
            out[w] = s
    return out


def correction(O, thr, g, C, sigma):
    sigma = f64(sigma)
    corr = f64(0.0)
    with np.errstate(all="ignore"):
        for c in range(2, C):
            fwd = lpdiff(O, (f64(g[c - 1]) - f64(thr[c])) / sigma, (f64(thr[c + 1]) - f64(thr[c])) / sigma)
            rev = lpdiff(O, (f64(thr[c - 1]) - f64(g[c])) / sigma, (f64(g[c + 1]) - f64(g[c])) / sigma)
            corr = corr + (fwd - rev)
    return corr


def decide(O, thr, g, ok, part, C, sigma, tries, accepted, adapt, seed, chain, it, u=None):
    """(thr', sigma', tries', accepted', accept): the decision and, with adapt, the Robbins-Monro step of log sigma with the gain
    1 / sqrt(tries').  u replaces the uniform of stream (seed, chain, it, 24, 1)."""
    thr = np.array(thr, dtype=np.float64)
    accept = False
    with np.errstate(all="ignore"):
        if ok:
            s = f64(part[0])
            for w in range(1, len(part)):
                s = s + f64(part[w])
            L = s + correction(O, thr, g, C, sigma)
            if u is None:
                u = O.draws(seed, chain, it, KIND_THRESHOLD_MH, 1, 0, 1)[0]
            accept = bool(f64(O.det_log(f64(u))) < L)
        if accept:
            thr[2:C] = np.asarray(g)[2:C]
        tries += 1
        accepted += int(accept)
        sigma = f64(sigma)
        if adapt:
            ls = f64(O.det_log(sigma))
            gain = f64(1.0) / np.sqrt(f64(tries))
            d = (f64(1.0) if accept else f64(0.0)) - TARGET
            ls = ls + gain * d
            ls = LS_MIN if ls < LS_MIN else ls
            ls = LS_MAX if ls > LS_MAX else ls
            sigma = f64(O.det_exp(ls))
    return thr, sigma, tries, accepted, accept


def step(O, thr, cls, liab, r_A, C, sigma, tries, accepted, adapt, seed, chain, it, varE=1.0, s_A=None, draw=None, u=None):
    """One whole step on thr[0..C]; returns what decide returns."""
    g, ok = propose(O, thr, C, sigma, seed, chain, it, draw)
    part = partials(row_terms(O, thr, g, cls, liab, r_A, varE, s_A)) if ok else None
    return decide(O, thr, g, ok, part, C, sigma, tries, accepted, adapt, seed, chain, it, u)


def full_thr(t, C):
    """thr[0..C] from the C - 1 thresholds t_1 .. t_{C-1} the library reports."""
    out = np.empty(C + 1)
    out[0], out[C] = -np.inf, np.inf
    out[1:C] = t
    return out


# ---- class probabilities of held-out records ----
def class_probs(O, thr, C, fit, varE=1.0, s=None):
    """p[k][c - 1] = exp(det_lpdiff((t_{c-1} - fit_k) / sd_k, (t_c - fit_k) / sd_k)) (det_exp; a mass of 0 gives 0)."""
    sde = np.sqrt(f64(varE))
    fit = np.asarray(fit, dtype=np.float64)
    out = np.zeros((len(fit), C))
    with np.errstate(all="ignore"):
        sd = np.full(len(fit), sde) if s is None else sde / np.asarray(s, dtype=np.float64)
        for c in range(1, C + 1):
            lp = lpdiff_v(O, (f64(thr[c - 1]) - fit) / sd, (f64(thr[c]) - fit) / sd)
            has = lp > -INF
            out[has, c - 1] = [O.det_exp(float(v)) for v in lp[has]]
    return out


# ---- cross-validation metrics, computed directly ----
def cv_metrics(prob, obs, C):
    """Brier score (sum over classes, mean over records), log-loss, accuracy of the arg-max class and, for C = 2, the AUC of p_2 by the
    rank-sum with ties at half weight; records with a NaN probability are left out."""
    prob, obs = np.asarray(prob, dtype=np.float64), np.asarray(obs)
    ok = ~np.isnan(prob).any(axis=1)
    p, o = prob[ok], obs[ok].astype(np.int64)
    onehot = np.zeros_like(p)
    onehot[np.arange(len(o)), o - 1] = 1.0
    out = dict(brier=float(((p - onehot) ** 2).sum(axis=1).mean()),
               logloss=float(-np.log(np.maximum(p[np.arange(len(o)), o - 1], np.finfo(np.float64).tiny)).mean()),
               class_accuracy=float((p.argmax(axis=1) + 1 == o).mean()))
    if C == 2:
        pos, neg = p[o == 2, 1], p[o == 1, 1]
        gt = (pos[:, None] > neg[None, :]).sum() + 0.5 * (pos[:, None] == neg[None, :]).sum()
        out["auc"] = float(gt / (len(pos) * len(neg))) if len(pos) and len(neg) else float("nan")
    return out


# ---- mixing: Geyer's estimator, and the law of the intercept-only model under Cowles' step with numpy's generator ----
def tau_geyer(x):
    """Integrated autocorrelation time n / ESS by Geyer's initial positive sequence estimator (the estimator of bench.py --full)."""
    x = np.asarray(x, dtype=np.float64) - np.mean(x)
    n = len(x)
    if n < 8 or not np.any(x):
        return 1.0
    f = np.fft.rfft(x, 2 * n)
    acf = np.fft.irfft(f * np.conj(f))[:n] / (x @ x)
    tau, k = -1.0, 0
    while k + 1 < n:
        pair = acf[k] + acf[k + 1]
        if pair <= 0:
            break
        tau += 2.0 * pair
        k += 2
    return float(max(tau, 1e-12))


def simulate_classes_cowles(cls, C, n_burn, n_kept, seed):
    """ref_liability.simulate_classes with Cowles' step in the place of the uniform draws (the device's order: thresholds, liabilities,
    intercept; sigma adapted through burn-in by the device's rule).  It measures the autocorrelation time the law test's bound uses,
    never the device's draws.  Returns the kept draws of (b, t_2 .. t_{C-1}) as an array [n_kept][C - 1]."""
    from scipy import stats
    rng = np.random.default_rng(seed)
    cls = np.asarray(cls)
    N = len(cls)
    thr = np.zeros(C + 1); thr[0], thr[C] = -np.inf, np.inf
    fr = np.cumsum([(cls == c).mean() for c in range(1, C)])
    q = stats.norm.ppf(fr)
    thr[1:C] = q - q[0]
    liab = np.array([thr[1] - 0.5 if c == 1 else thr[C - 1] + 0.5 if c == C else 0.5 * (thr[c - 1] + thr[c]) for c in cls])
    b, r = 0.0, liab.copy()
    sigma, tries = 1.0 / np.sqrt(N), 0
    out = np.empty((n_kept, C - 1))
    lpd = lambda a, bb: np.log(stats.norm.cdf(bb) - stats.norm.cdf(a))   # noqa: E731
    for it in range(n_burn + n_kept):
        fit = liab - r
        g = thr.copy()
        for c in range(2, C):
            g[c] = thr[c] + sigma * stats.truncnorm.rvs((g[c - 1] - thr[c]) / sigma, (thr[c + 1] - thr[c]) / sigma, random_state=rng)
        L = float(np.sum(lpd(g[cls - 1] - fit, g[cls] - fit) - lpd(thr[cls - 1] - fit, thr[cls] - fit)))
        for c in range(2, C):
            L += lpd((g[c - 1] - thr[c]) / sigma, (thr[c + 1] - thr[c]) / sigma) - lpd((thr[c - 1] - g[c]) / sigma, (g[c + 1] - g[c]) / sigma)
        take = np.log(rng.random()) < L
        if take:
            thr = g
        tries += 1
        if it < n_burn:
            sigma = float(np.exp(min(0.0, max(-20.0, np.log(sigma) + (float(take) - 0.44) / np.sqrt(tries)))))
        z = stats.truncnorm.rvs(thr[cls - 1] - fit, thr[cls] - fit, random_state=rng)
        liab = fit + z; r = z
        bn = (r.sum() + N * b) / N + rng.standard_normal() / np.sqrt(N)
        r = r - (bn - b); b = bn
        if it >= n_burn:
            out[it - n_burn, 0] = b
            out[it - n_burn, 1:] = thr[2:C]
    return out
