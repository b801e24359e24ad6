"""Law tests on the CPU: every conditional draw of a running chain against its closed-form law (tests/pivots.py), which shares
nothing with the draw layer -- the check that bit-for-bit twins written from one draw spec cannot give.

Chains: the C oracle in both orders (the blocked order's bits are the device's), and for what the oracle lacks (weighted residuals,
random-effect sets) the tests/ref_*.py restatements.  Per model and pivot family: KS against N(0,1) / U(0,1), p > 1e-4; lag-1
correlation of the normal pivots in draw order and per site across iterations, |r| < 4.5 / sqrt(n).  Seed and inputs are fixed in
tests/pivot_models.py.  Power: for every family a deliberately wrong law on the same recorded states must give p < 1e-8."""
import numpy as np
import pytest

import pivot_models as PM
import pivots as PV

BLOCKED = dict(R=8, S=12, D=4, near=3)        # a blocked layout of 96 rows: 12 shards of 8
_chains = {}                                  # a chain is recorded once and read by its law test and its power tests


def oracle_chain(O, name, order):
    key = (name, order)
    if key not in _chains:
        spec = PM.build(O, name)
        o = O.Oracle(order=order, seed=PM.SEED, chain=0)
        o.set_panel_f32(spec["X"], **(BLOCKED if order else {}))
        PM.apply_handle(o, spec)
        _chains[key] = (spec, PM.record(lambda: o.run(1), lambda: PM.state_handle(o, spec), spec))
    return _chains[key]


def ref_chain(O, name):
    if name not in _chains:
        import ref_numpy_weighted as RW
        import ref_random_tuple as RT
        spec = PM.build(O, name)
        X64 = spec["X"].astype(np.float64)
        c = RW.WeightedRefChain(O, X64, spec["y"], spec["w"], PM.SEED, 0) if spec["w"] is not None else RT.TupleRefChain(O, X64, spec["y"], PM.SEED, 0)
        PM.apply_ref(c, spec)
        _chains[name] = (spec, PM.record(lambda: c.run(1), lambda: PM.state_ref(c, spec), spec))
    return _chains[name]


@pytest.mark.parametrize("order", [0, 1], ids=["reference_order", "blocked_order"])
@pytest.mark.parametrize("name", [m for m in PM.MARKER if m != "PRw"] + PM.HOST_ONLY)
def test_oracle_draws_follow_their_laws(O, name, order):
    spec, states = oracle_chain(O, name, order)
    PM.check(PM.walk(spec, states), f"{name}/ora{order}")


@pytest.mark.parametrize("name", ["PRw"] + PM.RANDOM)
def test_restatement_draws_follow_their_laws(O, name):
    """Weighted residuals and the random-effect sets (identity, pedigree A^-1, dense inv(G), the (ID, Dam) tuple with unknown dams, one
    BayesPR set beside each): the chains of tests/ref_numpy_weighted.py and tests/ref_random_tuple.py, which the device is held to."""
    spec, states = ref_chain(O, name)
    PM.check(PM.walk(spec, states), f"{name}/ref")


# (family, the chain it is shown on, the wrong law)
POWER = [("z_marker", "PR", "drop_ivarbeta"),            # the 1 / varBeta term dropped from lhs
         ("z_fixed", "PR", "fixed_no_gs"),               # the other columns' current values left out of a fixed column's rhs
         ("z_random", "rand_ped", "k_identity"),         # K taken as identity for the pedigree set
         ("chi2_locus", "B", "nu_plus_one"),             # nu off by one
         ("chi2_region", "PRs", "nu_plus_one"),          # nu off by one, regions of 4 loci
         ("chi2_varE", "PRw", "vare_unweighted"),        # sum ycorr^2 in place of sum w ycorr^2
         ("chi2_varU", "rand_ped", "k_identity"),        # u'u in place of u'Ku
         ("pit_incl", "C", "incl_no_prior"),             # the prior odds left out of probDelta1
         ("pit_class", "R12", "probs_class"),            # probs in place of the sequential class law
         ("pi_dirichlet", "R12", "dirichlet_a"),         # Dirichlet a = nLoci
         ("pi_beta", "Cpi", "beta_a"),                   # Beta(nIn, P - nIn): the prior counts left out (1500 iterations, 8 columns)
         ("iw_diag", "T3", "iw_nu"),                     # the IW diagonal with nu for every i
         ("iw_off", "T3", "iw_stale")]                   # Psi from the effects of the iteration before


@pytest.mark.parametrize("fam,name,wrong", POWER, ids=[f"{f}-{w}" for f, _, w in POWER])
def test_a_wrong_law_is_seen(O, fam, name, wrong):
    """The same recorded states, one law deliberately wrong: the family's KS p-value falls below 1e-8 (and is fine under the right law:
    the tests above)."""
    spec, states = ref_chain(O, name) if name in PM.RANDOM + ["PRw"] else oracle_chain(O, name, 0)
    v = PM.walk(spec, states, wrong=(wrong,))[fam][0]
    p = PV.ks_p(fam, v)
    print(f"LAW power {fam} under {wrong} on {name}: n={len(v)} KS p={p:.3g}")
    assert p < 1e-8


@pytest.mark.parametrize("order", [0, 1], ids=["reference_order", "blocked_order"])
def test_class_search_of_twelve_classes(O, order):
    """A BayesR set over all-zero columns: rhs = 0 and every class's likelihood term is 1, so the class law is the sequential law of the
    fixed pi whatever the state.  With comparison 9's uniform keyed onto a neighbouring comparison 1 (the key packing before kind 18)
    the counts at odd loci and the independence at even loci both gave p = 0."""
    spec, states = oracle_chain(O, "search", order)
    cls = np.array([s["delta"][64:] for s in states[1:]])
    fig = PM.class_search_figures(cls, f"search/ora{order}")
    assert all(p > PM.KS_MIN for p in fig.values()), fig
    PM.check(PM.walk(spec, states), f"search/ora{order}")
