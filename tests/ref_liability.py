"""Numpy restatement of DESIGN.md section 2, "Liability traits": the truncated standard normal of the draw layer (Robert 1995), the start
values, the threshold step and the augmentation step.  Every function is the sequence of IEEE double operations the device performs (one
operation per numpy call, no fused multiply-add; det_log, det_exp and ppnd16 are the oracle's), so a test may ask for equality bit for bit.
simulate_* are the laws of the intercept-only models with numpy's own generator: they measure the autocorrelation time the law tests'
bounds use, never the device's draws."""
import numpy as np

KIND_LIABILITY = 22
KIND_THRESHOLD = 23
ROUNDS = 256
TWO_SQRT_E = np.float64(3.2974425414002564)
SQRT_2PI = np.float64(2.5066282746310002)
INF = np.float64(np.inf)
f64 = np.float64


class Uniforms:
    """The successive uniforms of one keyed stream (oracle.draws, what = 0), fetched as they are asked for."""

    def __init__(self, O, seed, chain, it, kind, index):
        self.O, self.key, self.buf, self.k = O, (seed, chain, it, kind, index), np.empty(0), 0

    def __call__(self):
        if self.k >= len(self.buf):
            n = 16 if len(self.buf) == 0 else 2 * ROUNDS
            if self.k >= n:
                raise RuntimeError("a draw took more uniforms than its loops allow")
            self.buf = self.O.draws(*self.key, 0, n)
        u = f64(self.buf[self.k])
        self.k += 1
        return u


class FromGenerator:
    """The same interface over numpy's generator (for the law and KS checks on the host); ppnd16 etc. still come from O."""

    def __init__(self, rng):
        self.rng = rng

    def __call__(self):
        return f64((np.floor(self.rng.random() * 2.0 ** 52) + 0.5) * 2.0 ** -52)


def _normal_above(O, u, a):
    for _ in range(ROUNDS):
        x = f64(O.ppnd16(u()))
        if x > a:
            return x
    return None


def _tail(O, u, a, b):
    aa = a * a
    s = np.sqrt(aa + f64(4.0))
    alpha = (a + s) / f64(2.0)
    for _ in range(ROUNDS):
        u1 = u(); u2 = u()
        lg = f64(O.det_log(u1))
        x = a - lg / alpha
        d = x - alpha
        q = -(d * d) / f64(2.0)
        rho = f64(O.det_exp(q))
        if x <= b and u2 <= rho:
            return x
    return None


def _above(O, u, a):
    return _normal_above(O, u, a) if a < 0.0 else _tail(O, u, a, INF)


def _uniform(O, u, a, b, m2):
    w = b - a
    for _ in range(ROUNDS):
        u1 = u(); u2 = u()
        x = a + w * u1
        q = (m2 - x * x) / f64(2.0)
        rho = f64(O.det_exp(min(q, f64(0.0)) if q == q else q))  # (det_exp takes an argument above 0 as 0)
        if u2 <= rho:
            return x
    return None


def switch_point(O, a):
    """a + 2 sqrt(e) / (a + sqrt(a^2 + 4)) exp((a^2 - a sqrt(a^2 + 4)) / 4), in the device's operation order."""
    aa = a * a
    s = np.sqrt(aa + f64(4.0))
    t = a * s
    d = aa - t
    q = d / f64(4.0)
    ex = f64(O.det_exp(min(q, f64(0.0))))
    den = a + s
    c = TWO_SQRT_E / den
    w = c * ex
    return a + w, aa


def _between_pos(O, u, a, b):
    lim, aa = switch_point(O, a)
    return _uniform(O, u, a, b, aa) if b <= lim else _tail(O, u, a, b)


def tnormal(O, u, a, b):
    """(z, fell): z from N(0, 1) restricted to (a, b) out of the uniforms u(); fell: the loop ran out and z is the fall-back value."""
    a, b = f64(a), f64(b)
    z = None
    with np.errstate(all="ignore"):
        if a < b:
            if b == INF:
                z = _above(O, u, a)
            elif a == -INF:
                z = _above(O, u, -b)
                z = None if z is None else -z
            elif a >= 0.0:
                z = _between_pos(O, u, a, b)
            elif b <= 0.0:
                z = _between_pos(O, u, -b, -a)
                z = None if z is None else -z
            elif b - a <= SQRT_2PI:
                z = _uniform(O, u, a, b, f64(0.0))
            else:
                for _ in range(ROUNDS):
                    x = f64(O.ppnd16(u()))
                    if x > a and x < b:
                        z = x
                        break
        if z is not None:
            return z, False
        fa, fb = bool(np.isfinite(a)), bool(np.isfinite(b))
        if fa and fb:
            return a + (b - a) / f64(2.0), True
        return (a if fa else (b if fb else f64(0.0))), True


def tnormal_stream(O, seed, chain, it, kind, index, a, b):
    return tnormal(O, Uniforms(O, seed, chain, it, kind, index), a, b)


# ---- start values ----
def start_classes(O, cls, C):
    """(thr[C + 1] with thr[0] = -inf, thr[1] = 0, thr[C] = +inf, liab) of the augmented rows' classes cls (1..C)."""
    cls = np.asarray(cls, dtype=np.int64)
    m = len(cls)
    thr = np.zeros(C + 1)
    thr[0], thr[C] = -np.inf, np.inf
    cum, q = 0, []
    for c in range(1, C):
        cum += int((cls == c).sum())
        q.append(f64(O.ppnd16(f64(cum) / f64(m))))
    for c in range(1, C):
        thr[c] = q[c - 1] - q[0]
    liab = np.empty(m)
    for k, c in enumerate(cls):
        liab[k] = thr[1] - f64(0.5) if c == 1 else thr[C - 1] + f64(0.5) if c == C else (thr[c - 1] + thr[c]) / f64(2.0)
    return thr, liab


def start_bounds(lo, hi):
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    with np.errstate(all="ignore"):
        mid = (lo + hi) / f64(2.0)
    return np.where(np.isfinite(lo) & np.isfinite(hi), mid, np.where(np.isfinite(lo), lo, hi))


# ---- one iteration ----
def thresholds(O, thr, cls, liab, C, seed, chain, it):
    """The threshold step (C >= 3): thr' from thr and the liabilities before the augmentation."""
    thr = np.array(thr, dtype=np.float64)
    cls = np.asarray(cls)
    for c in range(2, C):
        lower = max(thr[c - 1], f64(liab[cls == c].max()))
        upper = min(thr[c + 1], f64(liab[cls == c + 1].min()))
        u = f64(O.draws(seed, chain, it, KIND_THRESHOLD, c, 0, 1)[0])
        wd = upper - lower
        thr[c] = lower + u * wd
    return thr


def step(O, rows, liab, r_A, varE, lo, hi, seed, chain, it, s_A=None):
    """One augmentation step: r_A the residual of the augmented rows as ngp_get_state gives it, (lo, hi) their intervals (per row), s_A
    their row scales sqrt(w) under residual weights.  Returns (liab', e: the words the device writes into its residual, e': the residual
    ngp_get_state then reports, the number of draws that fell through).  varE == 0: nothing changes (None for the two residuals)."""
    if varE == 0.0:
        return np.array(liab), None, None, 0
    m = len(rows)
    sde = np.sqrt(f64(varE))
    out, e, ep, fell = np.empty(m), np.empty(m), np.empty(m), 0
    with np.errstate(all="ignore"):
        for k in range(m):
            fit = f64(liab[k]) - f64(r_A[k])
            sd = sde if s_A is None else sde / f64(s_A[k])
            a = (f64(lo[k]) - fit) / sd
            b = (f64(hi[k]) - fit) / sd
            z, f = tnormal_stream(O, seed, chain, it, KIND_LIABILITY, int(rows[k]), a, b)
            fell += int(f)
            e[k] = sde * z
            ep[k] = e[k] if s_A is None else e[k] / f64(s_A[k])
            out[k] = fit + ep[k]
    return out, e, ep, fell


# ---- the laws on the host, numpy's generator (tau for the bounds of the law tests) ----
def simulate_classes(cls, C, n_burn, n_kept, seed):
    """Intercept-only threshold model, varE = 1, in the device's order (thresholds, liabilities, intercept).  Returns the kept draws of
    (b, t_2 .. t_{C-1}) as an array [n_kept][C - 1]."""
    rng = np.random.default_rng(seed)
    cls = np.asarray(cls)
    N = len(cls)
    thr = np.zeros(C + 1); thr[0], thr[C] = -np.inf, np.inf
    fr = np.cumsum([(cls == c).mean() for c in range(1, C)])
    from scipy import stats
    q = stats.norm.ppf(fr)
    thr[1:C] = q - q[0]
    liab = np.array([thr[1] - 0.5 if c == 1 else thr[C - 1] + 0.5 if c == C else 0.5 * (thr[c - 1] + thr[c]) for c in cls])
    b = 0.0
    r = liab.copy()
    out = np.empty((n_kept, C - 1))
    for it in range(n_burn + n_kept):
        for c in range(2, C):
            lower = max(thr[c - 1], liab[cls == c].max()); upper = min(thr[c + 1], liab[cls == c + 1].min())
            thr[c] = lower + rng.random() * (upper - lower)
        fit = liab - r
        z = stats.truncnorm.rvs(thr[cls - 1] - fit, thr[cls] - fit, random_state=rng)
        liab = fit + z; r = z
        bn = (r.sum() + N * b) / N + rng.standard_normal() / np.sqrt(N)
        r = r - (bn - b); b = bn
        if it >= n_burn:
            out[it - n_burn, 0] = b
            out[it - n_burn, 1:] = thr[2:C]
    return out


def simulate_censored(y, rows, lo, hi, n_burn, n_kept, e_df, e_scale, seed):
    """Intercept-only Tobit model in the device's order (liabilities, varE, intercept): the kept draws of (b, varE) [n_kept][2]."""
    from scipy import stats
    rng = np.random.default_rng(seed)
    N = len(y)
    liab = start_bounds(lo, hi)
    r = np.array(y, dtype=np.float64); r[rows] = liab
    b, varE = 0.0, 0.0
    out = np.empty((n_kept, 2))
    for it in range(n_burn + n_kept):
        if varE > 0.0:
            fit = liab - r[rows]
            sd = np.sqrt(varE)
            z = stats.truncnorm.rvs((lo - fit) / sd, (hi - fit) / sd, random_state=rng)
            liab = fit + sd * z; r[rows] = sd * z
        varE = (e_df * e_scale + float(r @ r)) / rng.chisquare(e_df + N)
        bn = (r.sum() + N * b) / N + np.sqrt(varE / N) * rng.standard_normal()
        r = r - (bn - b); b = bn
        if it >= n_burn:
            out[it - n_burn] = b, varE
    return out


def autocorrelation_time(x):
    """Integrated autocorrelation time 1 + 2 sum rho_k, the sum cut at the first non-positive rho_k (Geyer's initial positive sequence,
    simplified)."""
    x = np.asarray(x, dtype=np.float64) - np.mean(x)
    n = len(x)
    v = float(x @ x) / n
    tau = 1.0
    for k in range(1, n // 4):
        rho = float(x[:-k] @ x[k:]) / (n * v)
        if rho <= 0.0:
            break
        tau += 2.0 * rho
    return tau


# ---- the data of the law tests (tests/test_gpu_liability.py) and their exact posteriors by quadrature ----
def law_binary():
    cls = 1 + (np.random.default_rng(41).normal(size=60) + 0.4 > 0.0).astype(np.int32)
    return dict(cls=cls, C=2, burn=500, kept=4000, seed=7)


def law_ordinal():
    l = np.random.default_rng(42).normal(size=60) + 0.3
    cls = (1 + (l > 0.0) + (l > 1.0)).astype(np.int32)
    return dict(cls=cls, C=3, burn=500, kept=4000, seed=8)


def law_censored():
    y = 3.0 + np.random.default_rng(43).normal(size=60)
    rows = np.flatnonzero(y > 3.5).astype(np.int64)
    return dict(y=y, rows=rows, lo=np.full(len(rows), 3.5), hi=np.full(len(rows), np.inf), e_df=4.0, e_scale=0.5, burn=500, kept=4000, seed=9)


def _moments(w, *grids):
    """Means and SDs of the coordinates under the weights w on the product grid."""
    w = w / w.sum()
    out = []
    for k, g in enumerate(grids):
        shape = [1] * len(grids); shape[k] = len(g)
        gk = g.reshape(shape)
        m = float((w * gk).sum())
        out.append((m, float(np.sqrt((w * (gk - m) ** 2).sum()))))
    return out


def posterior_binary(cls):
    """(mean, SD) of b under the flat prior: density Phi(b)^n1 (1 - Phi(b))^n0 (class 2 is l > 0)."""
    from scipy import stats
    n1, n0 = int((cls == 2).sum()), int((cls == 1).sum())
    b = np.linspace(-4.0, 4.0, 16001)
    lw = n1 * stats.norm.logcdf(b) + n0 * stats.norm.logcdf(-b)
    return _moments(np.exp(lw - lw.max()), b)[0]


def posterior_ordinal(cls):
    """[(mean, SD) of b, (mean, SD) of t_2] under flat priors on b and on t_2 > 0."""
    from scipy import stats
    n = [int((cls == c).sum()) for c in (1, 2, 3)]
    b = np.linspace(-3.0, 3.0, 1201).reshape(-1, 1)
    t = np.linspace(1e-4, 5.0, 2001).reshape(1, -1)
    with np.errstate(divide="ignore"):
        lw = n[0] * stats.norm.logcdf(-b) + n[1] * np.log(stats.norm.cdf(t - b) - stats.norm.cdf(-b)) + n[2] * stats.norm.logcdf(b - t)
    return _moments(np.exp(lw - lw.max()), b.ravel(), t.ravel())


def posterior_censored(y, rows, lo, e_df, e_scale):
    """[(mean, SD) of b, (mean, SD) of varE]: flat prior on b, scaled inverse chi-square (e_df, e_scale) on varE, records `rows` known only
    to exceed lo."""
    from scipy import stats
    obs = np.delete(np.asarray(y), rows)
    b = np.linspace(1.5, 5.0, 701).reshape(-1, 1)
    v = np.linspace(0.15, 6.0, 1171).reshape(1, -1)
    ss = ((obs.reshape(-1, 1, 1) - b) ** 2).sum(axis=0)
    lw = -(e_df / 2.0 + 1.0) * np.log(v) - e_df * e_scale / (2.0 * v) - 0.5 * len(obs) * np.log(v) - ss / (2.0 * v)
    for c in lo:
        lw = lw + stats.norm.logcdf((b - c) / np.sqrt(v))
    return _moments(np.exp(lw - lw.max()), b.ravel(), v.ravel())
