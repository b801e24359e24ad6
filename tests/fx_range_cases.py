"""Inputs and comparisons shared by tests/test_fx_range_host.py (oracle, CPU) and tests/test_gpu_fx_range.py (device): chains whose
response is scaled by a power of two, and chains whose head residual is small against the priors.

Power-of-two scaling.  Every draw, the Gibbs arithmetic and the scale rule floor(ilogb(m) / 2) are exactly equivariant under
y -> 2^k y when the prior scales and the start variances go with 2^2k: multiplying by a power of two is exact, so every rounding of
the scaled chain is the unit chain's rounding.  `setup_scaled` makes the k-th chain of a model, `assert_scaled` compares two
histories with array_equal."""
import math

import numpy as np

from conftest import add_sets

SCHEDULE = (6, 2, 2)
NITER = 6


# ---- the scale rule restated (csrc/ngp_common.h fx_exponent, csrc/ngp_kernels.h k_head; the clamp to +-900 is out of reach here) ----
def E_of(m):
    return (math.frexp(m)[1] - 1) // 2 + 5 if m > 0 else 5


def limit_old(mpm_max, yy):
    """a term t is refused when |t| 2^(52 - E) >= 2^53: the limit is 2^(E + 1); before the floor E came from ycorr'ycorr alone"""
    return 2.0 ** (E_of(mpm_max * yy) + 1)


def limit_new(mpm_max, yy, W, varE):
    fl = 2.0 ** -8 * W * varE
    return 2.0 ** (E_of(mpm_max * (yy if yy > fl else fl)) + 1)


# ---- power-of-two scaling ----
def fixed_columns(N, seed=3):
    """a two-column fixed-effect set (a covariate and a 0/1 factor), the same for every k: the design does not scale"""
    rng = np.random.default_rng(seed)
    return np.asfortranarray(np.column_stack([rng.normal(size=N), (rng.uniform(size=N) < 0.4).astype(np.float64)]))


def setup_scaled(m, spec, v, y, k, prior=(4.0, 1.0), Xfix=None, extra=None):
    """the k-th chain of a model on the oracle or the device: y 2^k, prior scales and start variances 2^2k (add_sets takes both
    from v; v (df - 2) / df is v's rounding times a power of two)"""
    add_sets(m, spec, math.ldexp(v, 2 * k))
    if extra is not None:
        extra(m, k)
    if Xfix is not None:
        m.add_fixed_set(Xfix)
    m.set_y(np.ldexp(y, k))
    m.set_residual_prior(prior[0], math.ldexp(prior[1], 2 * k))
    m.set_schedule(*SCHEDULE)


def snapshot(m, rsets=(), has_fixed=False):
    st = m.get_state()
    if has_fixed:
        st["fixed"] = m.get_fixed()["b"]
    for si in rsets:
        st["cls%d" % si] = m.get_class_state(si)["piHat"]
    return st


def sums(m, rsets=(), has_fixed=False):
    ps = m.get_posterior_sums()
    if has_fixed:
        ps["sum_fixed"] = m.get_fixed()["sum_b"]
    for si in rsets:
        ps["sum_cls%d" % si] = m.get_class_state(si)["sum_pi"]
    return ps


def walk(m, rsets=(), has_fixed=False, niter=NITER, step=None):
    """the state after every iteration and the posterior sums at the end"""
    hist = []
    for _ in range(niter):
        step() if step else m.run(1)
        hist.append(snapshot(m, rsets, has_fixed))
    return hist, sums(m, rsets, has_fixed)


ONE = ("ycorr", "beta", "b", "fixed", "sum_beta", "sum_b", "sum_fixed")      # scale with 2^k
TWO = ("varE", "varBeta", "sum_beta2", "sum_varBeta", "sum_varE")            # scale with 2^2k
SAME = ("delta", "piHat", "iter", "sum_delta", "sum_pi", "nKept")            # do not scale (and cls*, sum_cls*)


def assert_scaled_dict(u, s, k, where):
    assert set(u) == set(s), where
    for key in u:
        p = k if key in ONE else 2 * k if key in TWO else 0
        assert key in ONE or key in TWO or key in SAME or key.startswith("cls") or key.startswith("sum_cls"), key
        a, b = np.asarray(u[key]), np.asarray(s[key])
        if a.dtype.kind == "f":
            assert np.isfinite(b).all(), (where, key)
            a = np.ldexp(a, p)
        assert np.array_equal(a, b), (where, key, k)


def assert_scaled(unit, scaled, k):
    """unit, scaled: (history, sums) of walk(); the scaled chain is the unit chain times 2^k, bit for bit"""
    assert len(unit[0]) == len(scaled[0])
    for it, (u, s) in enumerate(zip(unit[0], scaled[0])):
        assert_scaled_dict(u, s, k, "iteration %d" % (it + 1))
    assert_scaled_dict(unit[1], scaled[1], k, "posterior sums")


# ---- small head residuals ----
SMALL_SET = dict(df=4.0, scale=0.025, vb0=0.05)     # the one BayesPR set of every small-head input
SMALL_HEADS = {  # name -> (response: factor of default_rng(9).normal, residual prior, fixed varE, intercept)
    "tiny_y": (1e-9, (4.0, 100.0), 0.0, True),
    "zero_y_wide_prior": (0.0, (4.0, 1600.0), 0.0, True),
    "zero_y_fixed_varE": (0.0, (4.0, 100.0), 4.0, True),
    # ngp_sweep_set handed a zero ycorr, zero beta and varE = 1.5: the fine seam draws neither varE nor an intercept, so on a set that
    # covers the panel its n-th call is the n-th iteration of the chain with y = 0, varE held at 1.5 and no intercept
    "fine_seam_zero": (0.0, (4.0, 100.0), 1.5, False),
}


# Shapes of the small-head inputs: name -> (N, P, byte tiles, panel multiplier).  With a zero head the first iteration's terms are a
# few sqrt(max x'x varE) whatever the priors (the effects are drawn about sqrt(varE / x'x) wide), and the limit before the floor
# was 64: on the N = 300 panel of centred genotypes (x'x <= 150) no zero-head input leaves it twofold.  The fp32 engines therefore
# take the zero-head inputs over the panel times 4 (a covariate in other units: x'x 16-fold, terms and both limits 4-fold), byte
# tiles -- codes 0, 1, 2 cannot be rescaled -- over N = 1500.  The fine seam's varE = 1.5 stays below 128 on byte tiles of N <= 1500
# (83 measured on the oracle): that one combination is left out.  The zero-head shapes have P = 450, eight blocks: with four blocks
# and lag 6 no GEMV of the first iteration would see an update, and no term of it would grow at all.
SMALL_SHAPES = {
    "n300": (300, 200, False, 1.0), "n300_x4": (300, 450, False, 4.0),
    "n1500": (1500, 200, False, 1.0), "n1500_x4": (1500, 450, False, 4.0),
    "n300_bytes": (300, 200, True, 1.0), "n1500_bytes": (1500, 450, True, 1.0),
}
ZERO_HEADS = ("zero_y_wide_prior", "zero_y_fixed_varE", "fine_seam_zero")
SMALL_CASES = ([("tiny_y", s) for s in ("n300", "n1500", "n300_bytes")] + [(n, s) for s in ("n300_x4", "n1500_x4") for n in ZERO_HEADS] +
               [("zero_y_wide_prior", "n1500_bytes"), ("zero_y_fixed_varE", "n1500_bytes")])


# the inputs the oracle's own range check refuses under the rule before the floor, on the layouts of tests/test_fx_range_host.py (the
# others leave the old range only in the coarser measure max |x_j'ycorr|: their shard partials, the terms themselves, stay below 64)
OLD_RULE_REFUSES = {c for c in SMALL_CASES if c[0] == "tiny_y" or (c[1] in ("n300_x4", "n1500_x4") and c != ("fine_seam_zero", "n1500_x4"))}


def small_panel(O, shape):
    """(the panel as set_panel takes it, the same in Float64 and centred as the chain sees it)"""
    from conftest import make_problem
    N, P, u8, mult = SMALL_SHAPES[shape]
    X, _, _, _ = make_problem(O, N, P)
    if u8:
        _, mu = O.generate_panel(N, P)
        G = np.rint(X.astype(np.float64) + mu[None, :]).astype(np.uint8)      # the genotype codes behind the centred panel
        return G, G.astype(np.float64) - G.mean(axis=0)
    X = np.asfortranarray(X * np.float32(mult))
    return X, X.astype(np.float64)


def small_y(name, N, k=0):
    return np.ldexp(SMALL_HEADS[name][0] * np.random.default_rng(9).normal(size=N), k)


def setup_small(m, name, N, P, k=0):
    """the chain of a small-head input on the oracle or the device (k: the same input scaled by 2^k)"""
    f, prior, fix, intercept = SMALL_HEADS[name]
    m.add_marker_set(0, P, 0, SMALL_SET["df"], math.ldexp(SMALL_SET["scale"], 2 * k), [(0, P)], [math.ldexp(SMALL_SET["vb0"], 2 * k)])
    m.set_residual_prior(prior[0], math.ldexp(prior[1], 2 * k))
    if fix > 0.0:
        m.fix_residual_variance(math.ldexp(fix, 2 * k))
    if not intercept:
        m.set_intercept(False)
    m.set_y(small_y(name, N, k))
    m.set_schedule(*SCHEDULE)
