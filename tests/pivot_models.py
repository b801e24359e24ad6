"""The models of the law tests (TEST INFRASTRUCTURE): one description per model, applied alike to the C oracle, to a tests/ref_*.py
chain and to the device handle; the chain's state after every iteration in the shape tests/pivots.py reads; and the assertions over
the pooled pivots.  Inputs and seeds are fixed here, before any result is looked at."""
import numpy as np

import pivots as PV
from conftest import make_problem

N = 96
SEED = 1001
KS_MIN = 1e-4            # conditions, not measurements: KS p-value of a family, and the same tail for a lag-1 correlation
LAG_Z = 4.5

R12_V = [0.0, 1e-5, 3e-5, 1e-4, 3e-4, 1e-3, 3e-3, 0.01, 0.03, 0.1, 0.3, 1.0]
R12_PI = [0.4, 0.1, 0.08, 0.08, 0.07, 0.06, 0.05, 0.05, 0.04, 0.03, 0.02, 0.02]
SEARCH_PI = [0.125] + [0.005] * 7 + [0.06, 0.26, 0.26, 0.26]          # the class-search case: twelve classes, a zero class first

MARKER = ["PR", "B", "C", "R4", "R12", "R16", "T2", "T3", "PRw", "PRs"]       # PRs: BayesPR with 48 regions of 4 loci (nu = df + 4)
HOST_ONLY = ["Cpi"]               # a long BayesC chain over 8 columns: where the counts are small the prior +1 of Beta(nIn + 1, P - nIn + 1) shows
RANDOM = ["rand_I", "rand_ped", "rand_G", "rand_T2"]
ITERS = dict(PR=150, PRw=150, B=300, C=300, R4=200, R12=200, R16=200, T2=150, T3=150, rand_I=300, rand_ped=200, rand_G=150, rand_T2=200,
             search=400, PRs=150, Cpi=1500)


def tuple_columns(col0, nloc, k):
    """Panel column of component m of locus l (include/nextgp_hip.h, ngp_add_marker_set_tuple): 64 // k loci per 64-column block."""
    l = np.arange(nloc)[:, None]
    Lb = 64 // k
    return col0 + 64 * (l // Lb) + k * (l % Lb) + np.arange(k)[None, :]


def tabular_A(s, d):
    """Numerator relationship matrix by the tabular method; s / d 0-based parents listed earlier, -1 unknown."""
    n = len(s)
    A = np.zeros((n, n))
    for i in range(n):
        A[i, i] = 1.0 + (0.5 * A[s[i], d[i]] if s[i] >= 0 and d[i] >= 0 else 0.0)
        for j in range(i):
            A[i, j] = A[j, i] = 0.5 * ((A[j, s[i]] if s[i] >= 0 else 0.0) + (A[j, d[i]] if d[i] >= 0 else 0.0))
    return A


def pedigree(n, founders, rng):
    s, d = np.full(n, -1), np.full(n, -1)
    for i in range(founders, n):
        lo = max(0, i - 20)
        s[i], d[i] = rng.choice(np.arange(lo, i), 2, replace=False)
    K = np.linalg.inv(tabular_A(s, d))
    K[np.abs(K) < 1e-9] = 0.0                     # A^-1 is sparse (an animal, its parents, mates and offspring): rounding noise is not structure
    return s, d, (K + K.T) / 2.0


def _marker(kind, col0, ncol, v):
    df = 4.0
    sc = v * (df - 2.0) / df
    one = [(j, j + 1) for j in range(ncol)]
    if kind == "PR":
        h = (ncol * 52) // 100
        return dict(method="PR", col0=col0, ncol=ncol, df=df, scale=sc, regions=[(0, h), (h, ncol)], vb0=[v, v])
    if kind == "PRs":
        regs = [(a, a + 4) for a in range(0, ncol, 4)]
        return dict(method="PR", col0=col0, ncol=ncol, df=df, scale=sc, regions=regs, vb0=[v] * len(regs))
    if kind == "B":
        return dict(method="B", col0=col0, ncol=ncol, df=df, scale=sc, regions=one, vb0=[v] * ncol, pi0=0.3, estPi=True)
    if kind == "Cpi":
        return dict(method="C", col0=col0, ncol=ncol, df=df, scale=sc, regions=[(0, ncol)], vb0=[v], pi0=0.1, estPi=True)
    if kind == "C":
        return dict(method="C", col0=col0, ncol=ncol, df=df, scale=sc, regions=[(0, ncol)], vb0=[v], pi0=0.3, estPi=True)
    if kind == "R4":
        return dict(method="R", col0=col0, ncol=ncol, df=df, scale=sc, regions=one, vb0=[v], vClass=[0.0, 0.01, 0.1, 1.0], pi=[0.5, 0.3, 0.15, 0.05], estPi=True)
    if kind == "R12":
        return dict(method="R", col0=col0, ncol=ncol, df=df, scale=sc, regions=one, vb0=[v], vClass=R12_V, pi=R12_PI, estPi=True)
    if kind == "R16":
        return dict(method="R", col0=col0, ncol=ncol, df=df, scale=sc, regions=one, vb0=[v], vClass=[2.0 ** (i - 15) for i in range(16)], pi=[1.0 / 16] * 16,
                    estPi=False)
    if kind == "search":
        return dict(method="R", col0=col0, ncol=ncol, df=df, scale=sc, regions=one, vb0=[v], vClass=R12_V, pi=SEARCH_PI, estPi=False)
    raise ValueError(kind)


def _tuple(k, nloc, v):
    df = 3.0 + k                                                               # mme.jl:493, 501
    vm = v * (0.6 * np.eye(k) + 0.4 * np.ones((k, k)))
    h = (nloc * 2) // 5
    # k = 2: two regions; k = 3: eight regions of eight loci -- small nu = df + 8 and many draws, so that a wrong nu - i shows
    regions = [(0, h), (h, nloc)] if k == 2 else [(a, a + 8) for a in range(0, nloc, 8)]
    return dict(method="T", col0=0, ncol=int(tuple_columns(0, nloc, k).max()) + 1, k=k, nloc=nloc, cols=tuple_columns(0, nloc, k), df=df,
                scale=vm * (df - k - 1.0), regions=regions, vb0=vm)


def build(O, name):
    """The model `name`: dict(X float32 panel, y, w, E, fixed, random, sets, iters)."""
    rng = np.random.default_rng(7)
    spec = dict(name=name, w=None, fixed=[], random=[], iters=ITERS[name[:-2] if name.endswith("_w") else name])
    if name in ("T2", "T3"):
        k = int(name[1])
        nloc = 96 if k == 2 else 64
        Xs, y, bt, v = make_problem(O, N, nloc * k, ncausal=12)
        t = _tuple(k, nloc, v)
        X = np.zeros((N, 192 if k == 2 else 256), dtype=np.float32, order="F")
        for m in range(k):
            X[:, t["cols"][:, m]] = Xs[:, m * nloc:(m + 1) * nloc]
        spec.update(X=X, y=y, sets=[t])
    elif name == "search":
        Xs, y, bt, v = make_problem(O, N, 64)
        X = np.zeros((N, 320), dtype=np.float32, order="F")
        X[:, :64] = Xs                                                          # one ordinary set keeps mpm_max positive
        spec.update(X=X, y=y, sets=[dict(method="PR", col0=0, ncol=64, df=4.0, scale=v * 0.5, regions=[(0, 64)], vb0=[v]), _marker("search", 64, 256, v)])
    elif name in MARKER or name in HOST_ONLY:
        P = 8 if name == "Cpi" else (192 if name in ("PR", "PRw", "PRs", "B", "C") else 256)
        X, y, bt, v = make_problem(O, N, P, ncausal=5 if name == "Cpi" else 20)
        if name in ("B", "C"):
            X[:, 5] = 0.0                        # a monomorphic column: mpm = 0, probDelta1 = NaN, never included (functions.jl:169-174)
        spec.update(X=X, y=y, sets=[_marker("PR" if name == "PRw" else name, 0, P, v)])
        if name in ("PR", "PRw"):
            F = rng.normal(size=(N, 3))
            F[:, 1] += 0.6 * F[:, 0]                                             # correlated columns: the Gauss-Seidel couplings matter
            spec["fixed"] = [F]
            spec["y"] = y + F @ np.array([1.0, -0.5, 0.8])
        if name == "PRw":
            spec["w"] = rng.uniform(0.3, 3.0, N)
    else:
        weighted = name.endswith("_w")
        base = name[:-2] if weighted else name
        X, y, bt, v = make_problem(O, N, 192, ncausal=20)
        sets = [dict(method="PR", col0=0, ncol=192, df=4.0, scale=v * 0.5, regions=[(0, 192)], vb0=[v])]
        vy = float(y.var())
        if base == "rand_I":
            q = 24
            R = dict(levels=rng.integers(0, q, N)[None, :], q=q, K=None, df=4.0, v0=0.3 * vy)
        elif base == "rand_ped":
            q = 96
            s, d, K = pedigree(q, 12, rng)
            R = dict(levels=rng.integers(0, q, N)[None, :], q=q, K=K, df=4.0, v0=0.3 * vy)
        elif base == "rand_G":
            q = N
            Xd = X.astype(np.float64)
            G = Xd @ Xd.T / np.sum(Xd * Xd) * N + 0.05 * np.eye(N)
            K = np.linalg.inv(G)
            R = dict(levels=np.arange(N)[None, :], q=q, K=(K + K.T) / 2.0, df=4.0, v0=0.3 * vy, dense=True)
        elif base == "rand_T2":
            q = 96
            s, d, K = pedigree(q, 12, rng)
            animal = rng.integers(0, q, N)
            animal[:8] = np.arange(8)                                            # founders: their dam is unknown
            V0 = 0.3 * vy * np.array([[1.0, 0.3], [0.3, 0.6]])
            R = dict(levels=np.stack([animal, d[animal]]), q=q, K=K, df=5.0, v0=V0, scale=V0 * (5.0 - 2.0 - 1.0))
            assert (R["levels"][1] < 0).any() and (R["levels"][1] >= 0).any()
        else:
            raise ValueError(name)
        if "scale" not in R:
            R["scale"] = R["v0"] * (R["df"] - 2.0) / R["df"]
        lev = R["levels"]
        ut = rng.normal(size=(R["q"], lev.shape[0])) * np.sqrt(0.3 * vy)
        y = y + sum(np.where(lev[a] >= 0, ut[np.maximum(lev[a], 0), a], 0.0) for a in range(lev.shape[0]))
        spec.update(X=X, y=y, sets=sets, random=[R])
        if weighted:
            spec["w"] = rng.uniform(0.3, 3.0, N)
    spec["E"] = (4.0, 0.25 * float(np.var(spec["y"])))
    return spec


def law_model(spec, device=False):
    """What tests/pivots.py is given.  The panel is the float64 of what the chain holds: the float32 panel, or, for a weighted device
    chain, the float32 tiles s x taken back to unscaled terms (DESIGN.md "Weighted residuals")."""
    X = spec["X"].astype(np.float64)
    if device and spec["w"] is not None:
        s = np.sqrt(spec["w"])[:, None]
        X = (s * X).astype(np.float32).astype(np.float64) / s
    return dict(X=X, w=spec["w"], E_df=spec["E"][0], E_scale=spec["E"][1], intercept=True, fixed=spec["fixed"], random=spec["random"], sets=spec["sets"])


# ---- one description, three kinds of chain ----
def apply_handle(m, spec, device=False):
    """The C oracle or the device handle (the panel is set by the caller).  Returns nothing; set ids are positions."""
    for F in spec["fixed"]:
        m.add_fixed_set(F)
    for R in spec["random"]:
        k = R["levels"].shape[0]
        if k > 1:
            m.add_random_set_tuple(R["levels"], R["q"], K=R["K"], df=R["df"], scale=R["scale"], varU0=R["v0"])
        elif R.get("dense"):
            m.add_random_set_dense(None, R["q"], K=R["K"], df=R["df"], scale=R["scale"], varU0=R["v0"])
        else:
            m.add_random_set(R["levels"][0], R["q"], K=R["K"], df=R["df"], scale=R["scale"], varU0=R["v0"])
    for M in spec["sets"]:
        if M["method"] == "R":
            m.add_marker_set_r(M["col0"], M["ncol"], M["df"], M["scale"], M["vb0"][0], M["vClass"], M["pi"], estPi=M["estPi"])
        elif M["method"] == "T":
            m.add_marker_set_tuple(M["col0"], M["nloc"], M["k"], M["df"], M["scale"], M["regions"], M["vb0"])
        else:
            m.add_marker_set(M["col0"], M["ncol"], {"PR": 0, "B": 1, "C": 2}[M["method"]], M["df"], M["scale"], M["regions"], M["vb0"], pi0=M.get("pi0", 0.0),
                             estPi=M.get("estPi", False))
    m.set_y(spec["y"])
    m.set_residual_prior(*spec["E"])


def apply_ref(c, spec):
    """A tests/ref_*.py chain (RefChain and its subclasses)."""
    c.E_df, c.E_scale = spec["E"]
    for F in spec["fixed"]:
        c.add_fixed(F)
    for R in spec["random"]:
        if R["levels"].shape[0] > 1:
            c.add_random_tuple(R["levels"], R["q"], K=R["K"], df=R["df"], scale=R["scale"], v=R["v0"])
        else:
            c.add_random(R["levels"][0], R["q"], K=R["K"], df=R["df"], scale=R["scale"], v=R["v0"])
    for M in spec["sets"]:
        if M["method"] == "R":
            c.add_set_r(M["col0"], M["ncol"], M["df"], M["scale"], M["vb0"][0], M["vClass"], M["pi"], estPi=M["estPi"])
        elif M["method"] == "T":
            c.add_set_tuple(M["cols"], M["df"], M["scale"], M["regions"], M["vb0"])
        else:
            c.add_set(M["col0"], M["ncol"], {"PR": 0, "B": 1, "C": 2}[M["method"]], M["df"], M["scale"], M["regions"], M["vb0"], pi0=M.get("pi0", 0.0),
                      estPi=M.get("estPi", False))


def _nvb(M):
    return {"PR": len(M["regions"]), "B": M["ncol"], "C": 1, "R": 1}[M["method"]] if M["method"] != "T" else len(M["regions"]) * M["k"] ** 2


def start_state(spec):
    """The chain before its first iteration (mme.jl:57, 443-444, 516): ycorr = y, every effect zero, the starting variances."""
    P = spec["X"].shape[1]
    vb = [np.tile(np.asarray(M["vb0"], dtype=np.float64).ravel(), len(M["regions"])) if M["method"] == "T" else np.array(M["vb0"], dtype=np.float64)
          for M in spec["sets"]]
    pi = [np.array(M["pi"], dtype=np.float64) if M["method"] == "R" else (np.array([1.0 - M["pi0"], M["pi0"]]) if "pi0" in M else None) for M in spec["sets"]]
    return dict(ycorr=np.array(spec["y"], dtype=np.float64), varE=float("nan"), b=0.0, fixed=[np.zeros(F.shape[1]) for F in spec["fixed"]],
                u=[np.zeros((R["q"], R["levels"].shape[0])) for R in spec["random"]],
                varU=[np.asarray(R["v0"], dtype=np.float64).reshape(R["levels"].shape[0], -1) for R in spec["random"]],
                beta=np.zeros(P), delta=np.ones(P, dtype=np.int64), varBeta=vb, pi=pi)


def state_handle(m, spec):
    st = m.get_state()
    out = dict(ycorr=st["ycorr"][:N].copy(), varE=st["varE"], b=st["b"], beta=st["beta"].copy(), delta=st["delta"].copy(), fixed=[], u=[], varU=[], varBeta=[],
               pi=[])
    if spec["fixed"]:
        b, o = m.get_fixed()["b"], 0
        for F in spec["fixed"]:
            out["fixed"].append(b[o:o + F.shape[1]].copy()); o += F.shape[1]
    for r in range(len(spec["random"])):
        g = m.get_random_tuple(r)
        out["u"].append(g["u"].copy()); out["varU"].append(g["varU"].copy())
    o = 0
    for si, M in enumerate(spec["sets"]):
        out["varBeta"].append(st["varBeta"][o:o + _nvb(M)].copy()); o += _nvb(M)
        out["pi"].append(m.get_class_state(si)["piHat"] if M["method"] == "R" else (st["piHat"][2 * si:2 * si + 2].copy() if M["method"] in ("B", "C") else None))
    return out


def state_ref(c, spec):
    st = c.state()
    P = spec["X"].shape[1]
    beta, delta = np.zeros(P), np.zeros(P, dtype=np.int64)
    o, vbs, pis = 0, [], []
    for si, M in enumerate(spec["sets"]):          # state() concatenates the sets' effects from each set's first column on
        n = M["ncol"]
        beta[M["col0"]:M["col0"] + n] = st["beta"][o:o + n]; delta[M["col0"]:M["col0"] + n] = st["delta"][o:o + n]; o += n
        vb = c.varBeta[si]
        vbs.append(np.concatenate([m.ravel() for m in vb]) if M["method"] == "T" else np.array(vb, dtype=np.float64))
        pis.append(c.M[si]["piHat"].copy() if M["method"] in ("B", "C", "R") else None)
    return dict(ycorr=st["ycorr"], varE=st["varE"], b=st["b"], beta=beta, delta=delta, fixed=[F["b"].copy() for F in getattr(c, "Xfix", [])],
                u=[np.array(u, dtype=np.float64).reshape(R["q"], -1) for u, R in zip(getattr(c, "u", []), spec["random"])],
                varU=[np.array(v, dtype=np.float64).reshape(R["levels"].shape[0], -1) for v, R in zip(getattr(c, "varU", []), spec["random"])], varBeta=vbs, pi=pis)


def record(step, state, spec):
    """States of the chain: before the first iteration and after each (step() runs one iteration)."""
    states = [start_state(spec)]
    for _ in range(spec["iters"]):
        step()
        states.append(state())
    return states


def walk(spec, states, device=False, wrong=()):
    """The pooled pivots of a recorded chain."""
    model = law_model(spec, device=device)
    rng = np.random.default_rng(2)              # the randomized PITs' own generator
    return PV.pool([PV.pivots(model, states[t], states[t + 1], rng, wrong=wrong) for t in range(len(states) - 1)])


def table(pooled):
    """family -> dict(n, ks, r_draw, n_draw, r_site, n_site)."""
    out = {}
    for fam, (v, site, it) in sorted(pooled.items()):
        row = dict(n=len(v), ks=PV.ks_p(fam, v))
        if fam in PV.NORMAL:
            row["r_draw"], row["n_draw"] = PV.lag1_draw_order(v)
            row["r_site"], row["n_site"] = PV.lag1_per_site(v, site, it)
        out[fam] = row
    return out


def check(pooled, label):
    """KS of every family against N(0,1) / U(0,1), p > 1e-4; lag-1 correlation of the normal pivots in draw order and per site across
    iterations, |r| < 4.5 / sqrt(n).  Every figure is printed before anything is asserted."""
    tab = table(pooled)
    for fam, row in tab.items():
        extra = f"  lag1 draw r={row['r_draw']:+.4f} (n={row['n_draw']})  site r={row['r_site']:+.4f} (n={row['n_site']})" if "r_draw" in row else ""
        print(f"LAW {label:>16s} {fam:<13s} n={row['n']:<7d} KS p={row['ks']:.3g}{extra}")
    for fam, row in tab.items():
        assert row["ks"] > KS_MIN, (label, fam, row)
        if "r_draw" in row:
            assert abs(row["r_draw"]) < LAG_Z / np.sqrt(row["n_draw"]), (label, fam, row)
            if row["n_site"] > 0:
                assert abs(row["r_site"]) < LAG_Z / np.sqrt(row["n_site"]), (label, fam, row)
    return tab


# ---- the BayesR class search, exactly ----
def class_search_figures(cls, label):
    """cls [iterations, 256]: classes (1-based) of the all-zero columns, whose class law is the sequential law of the fixed pi whatever the
    state.  Chi-square of the class counts per locus parity, and independence of [class_l == 9] and [class_{l+1} == 1] per parity of l."""
    from scipy import stats
    law = PV.sequential_class_law(np.array(SEARCH_PI))
    fig = {}
    for par in (0, 1):
        cnt = np.bincount(cls[:, par::2].ravel() - 1, minlength=len(law))
        fig[f"counts_{'even' if par == 0 else 'odd'}"] = float(stats.chisquare(cnt, law * cnt.sum()).pvalue)
        l = np.arange(par, cls.shape[1] - 1, 2)
        a, b = (cls[:, l] == 9).ravel(), (cls[:, l + 1] == 1).ravel()
        tab = np.array([[np.sum(a & b), np.sum(a & ~b)], [np.sum(~a & b), np.sum(~a & ~b)]])
        fig[f"indep_{'even' if par == 0 else 'odd'}"] = float(stats.chi2_contingency(tab, correction=False).pvalue)
    for k, p in fig.items():
        print(f"LAW {label:>16s} class search {k}: p={p:.3g}")
    return fig
