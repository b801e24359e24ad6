"""Numpy restatement of DESIGN.md section 2, "Held-out records": the start value, the augmentation step and the sums over kept draws.
Every function is the sequence of IEEE double operations the device performs (one operation per numpy call, no fused multiply-add), so a
test may ask for equality bit for bit.  simulate_intercept_only is the law of the intercept-only model under augmentation with numpy's own
generator: it checks the closed-form bound of the law test, not the device's draws."""
import numpy as np

KIND_AUGMENT = 21


def ybar_obs(y, H):
    """Sum of the observed phenotypes in index order, left to right, divided by their count; y[H] is never read."""
    held = np.zeros(len(y), dtype=bool)
    held[np.asarray(H, dtype=np.int64)] = True
    acc = 0.0
    for i in range(len(y)):
        if not held[i]:
            acc = acc + float(y[i])
    return acc / float(len(y) - int(held.sum()))


def start(y, H):
    """(y as the chain starts from it -- the mean of the observed phenotypes on the held-out rows --, yaug[m])."""
    H = np.asarray(H, dtype=np.int64)
    yb = ybar_obs(y, H)
    y0 = np.array(y, dtype=np.float64)
    y0[H] = yb
    return y0, np.full(len(H), yb)


def step(yaug, r_H, varE, z, s_H=None):
    """One augmentation step: r_H the residual of the held-out rows as ngp_get_state gives it, z their normals (stream kind 21, keyed by
    the row), s_H their row scales sqrt(w) under residual weights.  Returns (yaug', the words the device writes into its residual, the
    residual ngp_get_state then reports).  varE == 0: nothing changes (None for the two residuals)."""
    if varE == 0.0:
        return np.array(yaug), None, None
    e = np.sqrt(np.float64(varE)) * np.asarray(z, dtype=np.float64)
    ep = e if s_H is None else e / np.asarray(s_H, dtype=np.float64)
    fit = np.asarray(yaug, dtype=np.float64) - np.asarray(r_H, dtype=np.float64)
    return fit + ep, e, ep


def accumulate(sum_fit, sum_fit2, n_fit, H, yaug, r_H):
    """A kept draw: fit = yaug - r into the three sums (N entries each, zero off H), in place."""
    H = np.asarray(H, dtype=np.int64)
    fit = np.asarray(yaug, dtype=np.float64) - np.asarray(r_H, dtype=np.float64)
    sum_fit[H] = sum_fit[H] + fit
    sum_fit2[H] = sum_fit2[H] + fit * fit
    n_fit[H] = n_fit[H] + 1.0
    return fit


def law_bound(mean_varE, f, n_obs, n_kept, sigmas=6.0):
    """The posterior of the intercept is N(ybar_obs, varE / n_obs); augmentation adds lag-1 autocorrelation of about f to its chain, so the
    mean of n_kept draws has variance about v (1 + f) / ((1 - f) n_obs n_kept)."""
    return sigmas * np.sqrt(mean_varE * (1.0 + f) / ((1.0 - f) * n_obs * n_kept))


def simulate_intercept_only(y, H, n_burn, n_kept, e_df, e_scale, seed):
    """The chain of y = b + e with the rows H held out, in the order of the device's iteration (augmentation, varE, intercept), drawn with
    numpy's generator.  Returns (mean of b, mean of the fitted values of H, mean of varE) over the kept draws."""
    rng = np.random.default_rng(seed)
    H = np.asarray(H, dtype=np.int64)
    N = len(y)
    y0, yaug = start(y, H)
    ycorr = y0.copy()
    b, varE = 0.0, 0.0
    sb = sv = 0.0
    sfit = np.zeros(len(H))
    for it in range(1, n_burn + n_kept + 1):
        yaug, e, _ = step(yaug, ycorr[H], varE, rng.standard_normal(len(H)))
        if e is not None:
            ycorr[H] = e
        varE = (e_df * e_scale + float(ycorr @ ycorr)) / rng.chisquare(e_df + N)
        bn = (float(ycorr.sum()) + N * b) / N + np.sqrt(varE / N) * rng.standard_normal()
        ycorr -= bn - b
        b = bn
        if it > n_burn:
            sb += b; sv += varE
            sfit += yaug - ycorr[H]
    return sb / n_kept, sfit / n_kept, sv / n_kept
