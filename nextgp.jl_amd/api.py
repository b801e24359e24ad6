"""Host-side mirror of the NextGP.jl user interface for the accelerated path.

Same names, argument meaning and output files as the reference, so a model script ports line by line:

    reference (Julia)                                   this module (Python stand-in for the Julia shim)
    ------------------------------------------------    ------------------------------------------------
    runLMEM(f, data, nChain, nBurn, nThin; VCV, ...)    runLMEM(f, data, nChain, nBurn, nThin, VCV=..., ...)   src/MCMC.jl:31-41
    BayesPR(r, v) / BayesB(pi, v; estimatePi)           BayesPR(r, v) / BayesB(pi, v, estimatePi=...)          src/runTime.jl:30-61
    Random("I", v)          (residual prior, key :e)    Random("I", v)                (key "e")                 src/runTime.jl:135-146
    Random(dvec, v)         (weighted residuals, "D")   Random(d, v), d_ii per record (key "e")                 src/mme.jl:71-75
    SNP(M, "geno.txt"[, "map.txt"]) in the formula      the same text inside the formula string                src/runTime.jl:13-28
    BayesLV(v, f, covariates, varZeta; estimateVarZeta) BayesLV(v, "0 ~ x1 + x2", {"x1": ..}, varZeta, ...)    src/runTime.jl:116-133
    summaryMCMC("betaM"; outFolder)                     summaryMCMC("betaM", outFolder=...)                    src/misc.jl:241-244

    makePed(pedigree, ids) / makeA(s, d)                makePed(path_or_rows, ids) / makeA(s, d)               src/misc.jl:73-115

Interpreted here: the response, the intercept `1`, covariate / factor columns (optionally grouped by `blockThese`), `(1|g)` random
effects, `PED(col)` pedigree effects (with `userPedData`), correlated (Tuple) pedigree effects -- a VCV key ("ID", "Dam") with a k x k
covariance -- and `SNP(...)` terms.  Interactions and BayesRCplus are outside the accelerated path and raise NotImplementedError naming the reference code that handles them.
All arithmetic happens in libnextgp_hip.so; this file only parses, reshapes and writes files.
"""
import os
import re
from dataclasses import dataclass
from typing import Optional

import numpy as np

from ._lib import pedigree_a22, pedigree_ainv, LV_MAXCOV, METHOD_BAYESB, METHOD_BAYESC, METHOD_BAYESPR, Sampler, tuple_columns, tuple_panel, tuple_span

__all__ = ["makePed", "makeA", "makeG", "gblup_terms", "BayesPR", "BayesB", "BayesC", "BayesR", "BayesRCπ", "BayesRCpi", "BayesRCplus", "BayesLV", "lv_design_matrix", "Random", "SNP", "runLMEM", "summaryMCMC", "read_genotypes", "read_panel_file", "is_panel_file", "prep2RegionData", "parse_formula", "design_columns", "samples_to_out_files", "random_levels", "random_prior", "random_file_names", "read_prediction_file", "write_prediction_file", "write_variance_out_files", "write_gwas_files",
           "is_bed_file", "read_plink", "write_plink", "decode_bed"]


# ----------------------------------------------------------------------------------------------
# prior / term types (src/runTime.jl)
# ----------------------------------------------------------------------------------------------
@dataclass
class BayesPRType:  # src/runTime.jl:30-45
    r: int
    v: object       # a variance, or -- for correlated marker sets, VCV key (:M1, :M2) -- their k x k covariance matrix (src/mme.jl:493-516)
    name: str = "BayesPR"


@dataclass
class BayesBType:  # src/runTime.jl:48-61
    pi: float
    v: float
    name: str = "BayesB"
    estimatePi: bool = False


@dataclass
class BayesCType:  # src/runTime.jl:64-77
    pi: float
    v: float
    name: str = "BayesC"
    estimatePi: bool = False


@dataclass
class BayesRType:  # src/runTime.jl:78-93
    pi: object      # class probabilities (one per class)
    class_: object  # variance-class multipliers (the reference's field is `class`, a Python keyword)
    v: float
    name: str = "BayesR"
    estimatePi: bool = False


@dataclass
class BayesRCType:  # BayesRCπ(pi, class, v, annot): annotation-informed BayesR (src/mme.jl:384-403, src/functions.jl:291-360)
    pi: object      # class probabilities, the start of every annotation's row
    class_: object  # variance-class multipliers
    v: float        # the start of every annotation's variance
    annot: object   # nSNPs x nAnnot matrix of 0 / 1; every SNP in at least one annotation
    name: str = "BayesRCπ"
    estimatePi: bool = False


@dataclass
class BayesLogVarType:  # src/runTime.jl:116-133
    v: float
    f: str               # the variance formula, e.g. "0 ~ x1 + x2" (the reference: a StatsModels @formula)
    covariates: object   # mapping of numeric columns, one row per SNP (the reference: a DataFrame)
    varZeta: float
    name: str = "BayesLV"
    estimateVarZeta: object = False   # False: varZeta fixed; True: var(zeta); a float f: f * var(logVar) (src/functions.jl:481-485)


@dataclass
class RandomEffectType:  # src/runTime.jl:135-146
    str: object
    v: float
    type: int = 1


@dataclass
class GenomicTerm:  # src/runTime.jl:13-28
    name: str
    path: object
    map: str = ""


def BayesPR(r, v, name="BayesPR"):
    return BayesPRType(int(r), float(v) if np.ndim(v) == 0 else np.asarray(v, dtype=np.float64), name)


def BayesB(pi, v, name="BayesB", estimatePi=False):
    return BayesBType(float(pi), float(v), name, bool(estimatePi))


def BayesC(pi, v, name="BayesC", estimatePi=False):
    return BayesCType(float(pi), float(v), name, bool(estimatePi))


def BayesR(pi, class_, v, name="BayesR", estimatePi=False):
    """BayesR(pi, class, v; estimatePi) of src/runTime.jl:87-93: `class_` = variance-class multipliers, `pi` their probabilities."""
    return BayesRType([float(x) for x in pi], [float(x) for x in class_], float(v), name, bool(estimatePi))


def BayesRCπ(pi, class_, v, annot, name="BayesRCπ", estimatePi=False):
    """BayesRCπ(pi, class, v, annot; estimatePi): BayesR whose class probabilities and variance belong to an annotation; every SNP draws
    the annotation it acts through among those it has (`annot`: nSNPs x nAnnot, entries 0 / 1, no all-zero row; at most 8 annotations
    and nAnnot * classes <= 16).  BayesRCpi is the same constructor under an ASCII name."""
    an = np.asarray(annot)
    if an.ndim != 2 or an.size == 0:
        raise ValueError("BayesRCπ: annot is a matrix, one row per SNP and one column per annotation")
    if not np.isin(an, (0, 1)).all():
        raise ValueError("BayesRCπ: annot holds entries other than 0 / 1")
    if (an.sum(axis=1) == 0).any():
        raise ValueError(f"BayesRCπ: SNP {int(np.argmax(an.sum(axis=1) == 0)) + 1} has no annotation; the reference divides 0 / 0 there "
                         "(src/mme.jl:396) -- put such SNPs in a set of their own")
    if an.shape[1] > 8 or an.shape[1] * len(pi) > 16 or len(pi) < 2 or len(pi) != len(class_):
        raise ValueError("BayesRCπ: 2 or more classes with one probability each, at most 8 annotations, annotations x classes <= 16")
    return BayesRCType([float(x) for x in pi], [float(x) for x in class_], float(v), an.astype(np.int32), name, bool(estimatePi))


BayesRCpi = BayesRCπ


def BayesRCplus(*args, **kwargs):
    raise NotImplementedError("BayesRCplus takes one step per annotation on the same column inside a locus and keeps only their sum "
                              "(src/functions.jl:362-419): a different block chain from BayesRCπ's, which is on the device; it stays on the "
                              "reference's Julia path")


def BayesLV(v, f, covariates, varZeta, name="BayesLV", estimateVarZeta=False):
    """Log-linear model of the SNP variances (src/runTime.jl:116-133): log(var_j) = C_j c + zeta_j, zeta_j ~ N(0, varZeta).  `f` is the
    variance formula as a string ("0 ~ x1 + x2": the left side is ignored), `covariates` a mapping of numeric columns with one row per
    SNP of the set."""
    if not isinstance(f, str) or "~" not in f:
        raise ValueError('BayesLV: f is the variance formula as text, e.g. "0 ~ x1 + x2"')
    if not (isinstance(estimateVarZeta, bool) or isinstance(estimateVarZeta, float)):
        raise ValueError("BayesLV: estimateVarZeta is False, True or a Float64 fraction (src/runTime.jl:122)")
    return BayesLogVarType(float(v), f, covariates, float(varZeta), name, estimateVarZeta)


def lv_design_matrix(f, covariates):
    """(C, names): the design matrix modelmatrix(f, covariates) builds for a BayesLV prior (src/mme.jl:427) -- an intercept column
    first unless the formula has `0 +` / `- 1`, then the named numeric columns in formula order."""
    rhs = re.sub(r"\s+", "", f.split("~", 1)[1])
    toks = re.findall(r"([+-]?)([A-Za-z_0-9.]+|.)", rhs)
    intercept, names = True, []
    for sign, t in toks:
        if not re.fullmatch(r"[A-Za-z_0-9.]+", t):
            raise NotImplementedError(f"BayesLV: term {t!r} in the variance formula: interactions, functions and categorical terms are left to "
                                      "StatsModels' modelmatrix on the Julia path (src/mme.jl:427)")
        if t == "1":
            intercept = sign != "-"
        elif t == "0":
            intercept = intercept and sign == "-"
        elif sign == "-":
            raise NotImplementedError(f"BayesLV: removing the term {t!r} from the variance formula is left to StatsModels (src/mme.jl:427)")
        elif t not in names:
            names.append(t)
    cols = []
    for nm in names:
        if nm not in covariates:
            raise KeyError(f"BayesLV: the covariates have no column {nm!r}")
        col = np.asarray(covariates[nm])
        if col.dtype.kind not in "fiub":
            raise NotImplementedError(f"BayesLV: column {nm!r} is not numeric; categorical terms of the variance formula are coded by StatsModels' "
                                      "modelmatrix in the reference (src/mme.jl:427) and are not on the accelerated path")
        cols.append(col.astype(np.float64))
    n = len(cols[0]) if cols else len(next(iter(covariates.values())))
    if intercept:
        cols.insert(0, np.ones(n)); names = ["(Intercept)"] + names
    if not cols:
        raise ValueError("BayesLV: the variance formula has no term")
    if len(cols) > LV_MAXCOV:
        raise ValueError(f"BayesLV: at most {LV_MAXCOV} columns in the design matrix of the variance formula")
    if len({len(c) for c in cols}) != 1:
        raise ValueError("BayesLV: the covariate columns differ in length")
    return np.asfortranarray(np.column_stack(cols)), names


def Random(str, v, type=1):
    """v: the variance, or the k x k covariance matrix of a correlated (Tuple) random effect (src/runTime.jl:135-146)."""
    return RandomEffectType(str, float(v) if np.ndim(v) == 0 else np.array(v, dtype=np.float64), type)


def SNP(name, path, map=""):
    return GenomicTerm(name, path, map)


# ----------------------------------------------------------------------------------------------
# formula (the subset of the StatsModels DSL the marker path uses, src/prepMatVec.jl:112-169)
# ----------------------------------------------------------------------------------------------
class ParsedFormula(tuple):
    """(lhs, intercept, [GenomicTerm, ...]) with the plain covariate / factor terms as `.covariates` -- the parse result carries
    everything itself (no state is left on the function: two models parsed in turn, or from threads, cannot pick up each other's
    covariates)."""

    def __new__(cls, lhs, intercept, snps, covariates, random=(), order=(), ped=()):
        t = super().__new__(cls, (lhs, intercept, snps))
        t.covariates = list(covariates)
        t.random = list(random)  # grouping columns of the (1|g) terms, in formula order
        t.order = list(order)    # ("1|", g), ("ped", col) and ("snp", name) in formula order: where a GBLUP or PED term stands among the (1|g) terms
        t.ped = list(ped)        # columns of the PED(col) terms, in formula order
        return t


def parse_formula(formula, random_effects=False, pedigree=False):
    """'y ~ 1 + x + SNP(M, "geno.txt", "map.txt")' -> ParsedFormula (lhs, intercept, [GenomicTerm, ...]; .covariates = ['x']).
    random_effects=True also takes (1|g) terms (.random = ['g'], in formula order), as runLMEM does; without it they are refused, as
    they were before the device sampled them.  pedigree=True also takes PED(col) terms (.ped = ['col'], in formula order; runLMEM
    builds their A^-1 from userPedData); without it they are refused, as they were before makePed existed."""
    if "~" not in formula:
        raise ValueError("formula needs a '~'")
    lhs, rhs = [t.strip() for t in formula.split("~", 1)]
    terms, depth, cur = [], 0, ""
    for ch in rhs:
        if ch == "(":
            depth += 1
        elif ch == ")":
            depth -= 1
        if ch == "+" and depth == 0:
            terms.append(cur.strip())
            cur = ""
        else:
            cur += ch
    if cur.strip():
        terms.append(cur.strip())
    intercept, snps, covs, rnd, order, ped = False, [], [], [], [], []
    for t in terms:
        m = re.fullmatch(r"\(?\s*1\s*\|\s*([A-Za-z_][A-Za-z_0-9]*)\s*\)?", t)
        if m and t.count("(") == t.count(")"):
            if not random_effects:
                raise NotImplementedError(f"term '{t}': (1|g) random effects are refused by parse_formula(formula) and would stay on the "
                                          "reference's Julia path (src/functions.jl:57-110); runLMEM and parse_formula(formula, "
                                          "random_effects=True) take them to the device")
            rnd.append(m.group(1))  # (1|g): a random effect of the levels of column g (src/prepMatVec.jl:136-153)
            order.append(("1|", m.group(1)))
            continue
        if t == "1":
            intercept = True
        elif t == "0":
            intercept = False
        elif t.startswith("SNP(") and t.endswith(")"):
            args = [a.strip() for a in re.split(r",(?=(?:[^\"]*\"[^\"]*\")*[^\"]*$)", t[4:-1])]
            if len(args) < 2:
                raise ValueError(f"SNP term needs a name and a path: {t}")
            unq = [a.strip("\"'") for a in args]
            snps.append(GenomicTerm(unq[0], unq[1], unq[2] if len(unq) > 2 else ""))
            order.append(("snp", unq[0]))
        elif pedigree and (mp := re.fullmatch(r"PED\(\s*([A-Za-z_][A-Za-z_0-9]*)\s*\)", t)):
            ped.append(mp.group(1))  # PED(col): a random effect of every animal of the pedigree, K = A^-1 (src/prepMatVec.jl:136-153)
            order.append(("ped", mp.group(1)))
        elif t.startswith("PED("):
            raise NotImplementedError(f"term '{t}': building A^-1 from a pedigree needs PedigreeBase (src/mme.jl:26-37, src/prepMatVec.jl:136-153), "
                                      "so PED terms stay on the reference's Julia path; its coarse seam hands the Ainv it built to the device")
        elif "|" in t:
            raise NotImplementedError(f"term '{t}': only (1|g) random intercepts are on the accelerated path; random slopes and correlated "
                                      "(Tuple) random effects stay on the reference's Julia path (src/functions.jl:75-89, 100-110)")
        elif re.fullmatch(r"[A-Za-z_][A-Za-z_0-9]*", t):
            covs.append(t)  # a column of the data: covariate or factor (src/prepMatVec.jl:150-165)
        else:
            raise NotImplementedError(f"term '{t}': interactions / function terms stay on the reference's Julia path (StatsModels, "
                                      "src/prepMatVec.jl:150-165); use the fine seam (ngp_sweep_set) to combine them with the GPU sweep")
    return ParsedFormula(lhs, intercept, snps, covs, rnd, order, ped)


def random_levels(col):
    """(1|g) incidence as level codes: (level[N] int32 in 0..q-1, level names).  The levels are the sorted unique values of the
    column -- the column order StatsModels' modelcols gives Z (src/prepMatVec.jl:143-150) -- and u, its sums and the header of the
    u file all follow that order (the reference's header is unique(data.g), first appearance: DESIGN.md, "Random-effect sets")."""
    col = np.asarray(col)
    names, codes = np.unique(col, return_inverse=True)
    return codes.astype(np.int32), [str(v) for v in names.tolist()]


def random_prior(VCV, g, q):
    """(K, df, scale, v) of the (1|g) set from VCV["1|g"] or VCV["(1|g)"] (src/mme.jl:25-46, 265-272): Random("I", v) -> K = None
    (identity), Random(Sigma, v) with a q x q covariance Sigma -> K = inv(Sigma) in fp64; no entry -> Random("I", 100)."""
    prior = VCV.get(f"1|{g}", VCV.get(f"(1|{g})"))
    if prior is None:
        prior = Random("I", 100.0)                               # src/mme.jl:40-44
    if not isinstance(prior, RandomEffectType):
        raise ValueError(f"prior of (1|{g}): Random(str, v)")
    st = prior.str
    if st is None or (isinstance(st, str) and st in ("I", "")):
        K = None
    elif isinstance(st, str):
        raise NotImplementedError(f"(1|{g}) with structure {st!r}: \"A\" / \"G\" need the pedigree / genomic matrix the reference builds "
                                  "(PedigreeBase, src/mme.jl:26-37); pass the covariance matrix itself, or use the Julia coarse seam")
    else:
        S = np.asarray(st, dtype=np.float64)
        if S.shape != (q, q):
            raise ValueError(f"(1|{g}): the covariance matrix must be {q} x {q} (one row per level)")
        K = np.linalg.inv(S)                                     # src/mme.jl:36: inv(priorVCV[zSet].str)
        K = (K + K.T) / 2.0                                      # (exactly symmetric, as the library requires)
    df = 3.0 + 1.0                                               # src/mme.jl:261
    v = float(prior.v)
    return K, df, v * (df - 2.0) / df, v                         # src/mme.jl:265-272


def makeA(s, d):
    """The dense numerator relationship matrix by the tabular method (src/misc.jl:73-90): s / d are the 1-based positions of sire and dam
    in the list, 0 = unknown, parents in front of their offspring.  A_ii = 1 + A[s_i, d_i] / 2; A_ij = (A[i, s_j] + A[i, d_j]) / 2 for
    j > i.  The dense check of makePed's sparse A^-1 (O(n^2): small pedigrees only)."""
    s = np.asarray(s, dtype=np.int64); d = np.asarray(d, dtype=np.int64)
    n = len(s)
    if len(d) != n or np.any(s < 0) or np.any(d < 0) or np.any(s > np.arange(n)) or np.any(d > np.arange(n)):
        raise ValueError("makeA: sire / dam as 1-based positions of animals listed earlier, 0 = unknown")
    A = np.zeros((n + 1, n + 1))                                  # (row / column n stands for the unknown parent: all zero)
    si = np.where(s == 0, n, s - 1); di = np.where(d == 0, n, d - 1)
    for i in range(n):
        A[i, i] = 1.0 + A[si[i], di[i]] / 2.0
        for j in range(i + 1, n):
            A[i, j] = (A[i, si[j]] + A[i, di[j]]) / 2.0
            A[j, i] = A[i, j]
    return A[:n, :n].copy()


def _read_ped_rows(path_or_rows):
    if isinstance(path_or_rows, (str, os.PathLike)):
        rows = []
        with open(path_or_rows) as f:
            for ln, line in enumerate(f, 1):
                line = line.strip()
                if not line or line.startswith("#"):
                    continue
                t = line.split()
                if len(t) < 3:
                    raise ValueError(f"pedigree file {path_or_rows}, line {ln}: ID Sire Dam expected")
                rows.append((t[0], t[1], t[2]))
        return rows
    return [(str(a), str(b), str(c)) for a, b, c in path_or_rows]


def makePed(path_or_rows, userIDs=None):
    """(pedigree table, Ainv) from the reference's pedigree text -- `ID Sire Dam` per line, whitespace separated, `0` unknown, `#`
    comment lines -- or from rows of such triples (src/misc.jl:98-115; PedigreeBase's part is done here and in ngp_pedigree_ainv).
    The animals are put parents first by a stable topological order: an animal keeps its file position unless a parent comes later
    (then the parent is moved in front of it).  Refused: duplicate IDs, a parent that is not listed, a cycle, and phenotyped IDs
    (userIDs) outside the pedigree.  The table: dict(origID [n names in pedigree order], ID 1..n, Sire, Dam (1-based positions, 0
    unknown), F inbreeding coefficients, pos {name: 0-based position}); Ainv: CSR arrays (k_ptr, k_col, k_val), columns ascending."""
    rows = _read_ped_rows(path_or_rows)
    if not rows:
        raise ValueError("pedigree: no animal")
    idx = {}
    for k, (a, _, _) in enumerate(rows):
        if a == "0":
            raise ValueError("pedigree: an animal is called 0 (0 means unknown)")
        if a in idx:
            raise ValueError(f"pedigree: ID {a} is listed twice")
        idx[a] = k
    par = []
    for a, sr, dm in rows:
        for p in (sr, dm):
            if p != "0" and p not in idx:
                raise ValueError(f"pedigree: parent {p} of {a} is not listed as an animal")
        par.append([idx[p] for p in (sr, dm) if p != "0"])
    order, state = [], [0] * len(rows)                            # 0 new, 1 on the stack (its parents are being placed), 2 placed
    for k0 in range(len(rows)):
        if state[k0]:
            continue
        stack = [(k0, 0)]
        state[k0] = 1
        while stack:
            k, nxt = stack.pop()
            if nxt < len(par[k]):
                stack.append((k, nxt + 1))
                p = par[k][nxt]
                if state[p] == 1:
                    raise ValueError(f"pedigree: {rows[p][0]} is its own ancestor (a cycle)")
                if state[p] == 0:
                    state[p] = 1
                    stack.append((p, 0))
            else:
                state[k] = 2
                order.append(k)
    newpos = {k: i for i, k in enumerate(order)}
    orig = [rows[k][0] for k in order]
    sire = np.array([0 if rows[k][1] == "0" else newpos[idx[rows[k][1]]] + 1 for k in order], dtype=np.int32)
    dam = np.array([0 if rows[k][2] == "0" else newpos[idx[rows[k][2]]] + 1 for k in order], dtype=np.int32)
    pos = {a: i for i, a in enumerate(orig)}
    if userIDs is not None and not all(str(a) in pos for a in userIDs):
        raise ValueError("ErrorException: phenotyed individuals are not a subset of pedigree")   # src/misc.jl:106, its words
    F, Ainv = pedigree_ainv(sire, dam)
    return dict(origID=orig, ID=np.arange(1, len(orig) + 1), Sire=sire, Dam=dam, F=F, pos=pos), Ainv


def single_step_order(n, geno_pos):
    """perm[new] = old position: the levels of a single-step set -- the animals without a genotype first, in pedigree order, then the
    genotyped ones in the order given (the row order of the genotypes), so that the dense block sits on the LAST levels."""
    g = np.asarray(geno_pos, dtype=np.int64)
    is_g = np.zeros(int(n), dtype=bool)
    is_g[g] = True
    return np.concatenate([np.flatnonzero(~is_g), g]).astype(np.int64)


def permute_csr(K, perm):
    """P K P' of a CSR triple (k_ptr, k_col, k_val) for perm[new] = old: new row r is old row perm[r] with its columns renumbered and
    sorted ascending again.  The values move, none is recomputed: a symmetric K stays exactly symmetric."""
    kp, kc, kv = (np.asarray(a) for a in K)
    perm = np.asarray(perm, dtype=np.int64)
    inv = np.empty(len(perm), dtype=np.int64)
    inv[perm] = np.arange(len(perm))
    cnt = (kp[1:] - kp[:-1])[perm]
    np_ = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    nc = np.empty(len(kc), dtype=np.int32); nv = np.empty(len(kv), dtype=np.float64)
    for r, o in enumerate(perm):
        c = inv[kc[kp[o]:kp[o + 1]]]
        srt = np.argsort(c, kind="stable")
        nc[np_[r]:np_[r + 1]] = c[srt]
        nv[np_[r]:np_[r + 1]] = kv[kp[o]:kp[o + 1]][srt]
    return np_, nc, nv


def single_step_terms(singleStep, VCV, parsed, summaryStat=None):
    """{col: {"geno", "ids", "w"}} of the PED(col) terms whose prior is Random("H", v, type=1|2): single-step GBLUP, one breeding value
    per animal of the pedigree over H^-1 = A^-1 + [0 0; 0 inv((1 - w) G + w A22) - inv(A22)].  Host checks only, before any device work."""
    singleStep = dict(singleStep or {})
    summaryStat = summaryStat or {}
    is_h = lambda p: isinstance(p, RandomEffectType) and isinstance(p.str, str) and p.str == "H"
    for key, prior in VCV.items():
        if isinstance(key, tuple) and is_h(prior):
            raise NotImplementedError(f"VCV key {key}: \"H\" inside a correlated (Tuple) random effect; a single-step set has one component")
        if not isinstance(key, tuple) and is_h(prior) and key not in parsed.ped:
            raise ValueError(f"Random(\"H\", v) under {key!r}: single-step GBLUP is the prior of a PED(col) term")
    out = {}
    for col in parsed.ped:
        prior = VCV.get(col)
        if not is_h(prior):
            if col in singleStep:
                raise ValueError(f"singleStep[{col!r}] is given, but the prior of PED({col}) is not Random(\"H\", v)")
            continue
        if col not in singleStep:
            raise ValueError(f"PED({col}) with Random(\"H\", v) needs singleStep={{{col!r}: {{\"geno\": ..., \"ids\": [...], \"w\": 0.05}}}}")
        if prior.type not in (1, 2):
            raise ValueError("enter a valid method")                  # src/misc.jl:156
        if col in summaryStat:
            raise NotImplementedError(f"summaryStat for the single-step term PED({col}): summary statistics enter marker sets and fixed effects only")
        spec = singleStep[col]
        if not isinstance(spec, dict) or "geno" not in spec or "ids" not in spec or set(spec) - {"geno", "ids", "w"}:
            raise ValueError(f"singleStep[{col!r}]: {{\"geno\": path | array, \"ids\": [...], \"w\": 0.05}}")
        w = float(spec.get("w", 0.05))
        if not (0.0 <= w < 1.0):
            raise ValueError(f"singleStep[{col!r}]: the blending weight w must be in [0, 1)")
        out[col] = dict(geno=spec["geno"], ids=[str(a) for a in spec["ids"]], w=w)
    for col in singleStep:
        if col not in parsed.ped:
            raise ValueError(f"singleStep[{col!r}]: the model has no PED({col}) term")
    return out


def _single_step_prepare(spec, table, Ainv):
    """The host side of one single-step term: the genotypes, the pedigree positions of the genotyped animals, the renumbering, A^-1
    permuted to it, A22 by Colleau's method (ngp_pedigree_a22)."""
    ids = spec["ids"]
    if len(set(ids)) != len(ids):
        dup = sorted({a for a in ids if ids.count(a) > 1})[0]
        raise ValueError(f"singleStep: genotyped ID {dup} is listed twice")
    for a in ids:
        if a not in table["pos"]:
            raise ValueError(f"singleStep: genotyped ID {a} is not in the pedigree")
    M = read_genotypes(spec["geno"] if isinstance(spec["geno"], (str, os.PathLike)) else np.asarray(spec["geno"]))
    if M.ndim != 2 or M.shape[0] != len(ids):
        raise ValueError(f"singleStep: the genotypes have {M.shape[0] if M.ndim == 2 else '?'} rows for {len(ids)} ids")
    gpos = np.array([table["pos"][a] for a in ids], dtype=np.int64)
    n = len(table["origID"])
    perm = single_step_order(n, gpos)
    inv = np.empty(n, dtype=np.int64)
    inv[perm] = np.arange(n)
    A22 = pedigree_a22(table["Sire"], table["Dam"], table["F"], gpos)
    return dict(M=M, w=spec["w"], gpos=gpos, perm=perm, inv=inv, S=permute_csr(Ainv, perm), A22=A22, ng=len(ids),
                levels=[table["origID"][o] for o in perm])


def gblup_terms(snps, VCV, summaryStat=None):
    """Names of the SNP terms that are GBLUP: a Random("G", v; type = 1|2) prior under the term's name (src/prepMatVec.jl:122-126).
    What the reference would handle elsewhere and this path does not is refused here, before any device is touched."""
    summaryStat = summaryStat or {}
    out = []
    for t in snps:
        prior = VCV.get(t.name)
        in_tuple = [key for key in VCV if isinstance(key, tuple) and t.name in key]
        if not isinstance(prior, RandomEffectType):
            continue
        if not (isinstance(prior.str, str) and prior.str == "G"):
            raise NotImplementedError(f"prior of {t.name}: a Random prior under a SNP term's name means GBLUP and needs the structure \"G\" "
                                      "(src/prepMatVec.jl:122-126)")
        if prior.type not in (1, 2):
            raise ValueError("enter a valid method")                  # src/misc.jl:156
        if in_tuple:
            raise NotImplementedError(f"VCV key {in_tuple[0]} holds the GBLUP term {t.name}: correlated (Tuple) random effects stay on the "
                                      "reference's Julia path (sampleZ!(::Tuple), src/functions.jl:75-89, 100-110)")
        if t.map:
            raise NotImplementedError(f"map file on the GBLUP term {t.name}: the reference stores it with the Z set and never reads it "
                                      "(src/prepMatVec.jl:126); regions belong to marker priors (src/misc.jl:163-215)")
        if t.name in summaryStat:
            raise NotImplementedError(f"summaryStat for the GBLUP term {t.name}: summary statistics enter marker sets and fixed effects only "
                                      "(src/mme.jl:140-147, 314-322)")
        out.append(t.name)
    return out


GRM_COLUMNS_PER_CALL = 4096  # columns handed to the GRM builder per call (a multiple of 64: the result does not depend on the split)


def _grm_build(smp, M, method):
    """G of the raw genotypes M (N x P, any dtype read_genotypes returns) on smp's device, in column ranges: no concatenated host copy."""
    N, P = M.shape
    smp.grm_begin(N, method)
    for c0 in range(0, P, GRM_COLUMNS_PER_CALL):
        smp.grm_columns(M[:, c0:c0 + GRM_COLUMNS_PER_CALL])
    smp.grm_end()


def makeG(M, method=1, device=0):
    """VanRaden's genomic relationship matrix (src/misc.jl:145-160), built on the device in fp64 (matrix cores), returned as numpy.
    M: raw allele counts, N x P (uint8, float32 and float64 give the same bits on equal values).  Unlike the reference, M is not centred
    in place, and method 2 refuses a monomorphic column instead of filling G with NaN."""
    if method not in (1, 2):
        raise ValueError("enter a valid method")
    M = np.asarray(M)
    if M.ndim != 2:
        raise ValueError("makeG: an N x P genotype matrix")
    smp = Sampler(device=device)
    try:
        _grm_build(smp, M, method)
        return smp.grm_get()
    finally:
        smp.close()


def design_columns(name, col):
    """One model term -> (N x k design, level names): Float columns are centred, Int / String columns dummy coded with the first
    level as the base (the reference's rules, src/prepMatVec.jl docstring :33-37 and :46-60, through StatsModels)."""
    col = np.asarray(col)
    if col.dtype.kind == "f":
        x = col.astype(np.float64)
        return (x - x.mean())[:, None], [name]
    levels = sorted(set(col.tolist()))
    if len(levels) < 2:
        raise ValueError(f"factor {name} has a single level")
    X = np.column_stack([(col == lv).astype(np.float64) for lv in levels[1:]])
    return X, [f"{name}: {lv}" for lv in levels[1:]]


def design_codes(name, col):
    """A factor term -> (codes, names) without a dense matrix: codes[i] is the column of record i among the term's dummy columns, -1 for
    the base level (the first of the sorted levels); names and level order are design_columns'.  Float columns are covariates, not
    factors: ValueError."""
    col = np.asarray(col)
    if col.dtype.kind == "f":
        raise ValueError(f"{name} is a Float column (a covariate): design_columns centres it; only factors have level codes")
    levels, inv = np.unique(col, return_inverse=True)
    if len(levels) < 2:
        raise ValueError(f"factor {name} has a single level")
    return inv.astype(np.int64).ravel() - 1, [f"{name}: {lv}" for lv in levels.tolist()[1:]]


def _fixed_unit_width(cols, userData):
    """Number of design columns of a fixed unit (a term, or the terms of a blockThese group) without building them."""
    n = 0
    for c in cols:
        col = np.asarray(userData[c])
        n += 1 if col.dtype.kind == "f" else len(set(col.tolist())) - 1
    return n


def _add_fixed_unit_sparse(smp, cols, userData):
    """One fixed unit as a sparse set (Sampler.add_fixed_set_sparse): the terms' columns in model order, a factor's dummy columns from its
    level codes, a covariate's centred column in full.  Returns the column names."""
    from ._lib import factors_csc
    names, cps, rows, vals, N = [], [], [], [], None
    for c in cols:
        col = np.asarray(userData[c])
        if col.dtype.kind == "f":
            x = col.astype(np.float64)
            n_, _, cp, rw, vl = factors_csc([], (x - x.mean())[:, None])
            nm = [c]
        else:
            codes, nm = design_codes(c, col)
            n_, _, cp, rw, vl = factors_csc([codes])
        N = n_
        cps.append(np.diff(cp)); rows.append(rw); vals.append(vl); names += nm
    cp = np.concatenate([[0], np.cumsum(np.concatenate(cps))]).astype(np.int64)
    smp.add_fixed_set_sparse(N, len(cp) - 1, cp, np.concatenate(rows), np.concatenate(vals))
    return names


# ----------------------------------------------------------------------------------------------
# marker-matrix builders (src/prepMatVec.jl:113-134, src/misc.jl:163-215)
# ----------------------------------------------------------------------------------------------
def read_genotypes(path):
    """Space-delimited text, one row per individual, no header (prepMatVec.jl:116); columns holding a missing
    value are dropped (prepMatVec.jl:118).  Returns a float64 (N, P) Fortran-ordered matrix, NOT centred.
    Beyond the reference: an (N, P) array, or a `.npy` file (memory-mapped), is taken as it is -- uint8 allele counts stay
    uint8 (one byte per genotype; at 50k x 600k the text parse alone would take hours)."""
    if isinstance(path, (str, os.PathLike)) and str(path).endswith(".npy"):
        path = np.load(path, mmap_mode="r")
    elif isinstance(path, (str, os.PathLike)) and is_panel_file(path):
        return read_panel_file(path)
    elif isinstance(path, (str, os.PathLike)) and is_bed_file(path):   # a PLINK fileset, file order, missing calls at the column mean
        info = read_plink(path)
        return decode_bed(info["bed"], info["n"])
    if isinstance(path, np.ndarray):
        if path.dtype == np.uint8:
            return np.asfortranarray(path)
        M = np.asarray(path, dtype=np.float64)
    else:
        M = np.genfromtxt(path, delimiter=" ", dtype=np.float64)
        if M.ndim == 1:
            M = M[:, None]
    keep = ~np.isnan(M).any(axis=0)
    return np.asfortranarray(M[:, keep])


def is_panel_file(path):
    """True for the binary panel format of include/nextgp_hip.h (magic NGPPNL01)."""
    try:
        with open(path, "rb") as f:
            return f.read(8) == b"NGPPNL01"
    except OSError:
        return False


def read_panel_file(path):
    """Binary panel file -> (N, P) uint8 Fortran-ordered codes (host side; Sampler.load_panel_file streams the same file
    straight to the device)."""
    with open(path, "rb") as f:
        hd = f.read(32)
        if hd[:8] != b"NGPPNL01":
            raise ValueError(f"not a panel file: {path}")
        N, P = np.frombuffer(hd, dtype="<i8", count=2, offset=8)
        bits = int(np.frombuffer(hd, dtype="<i4", count=1, offset=24)[0])
        N, P = int(N), int(P)
        if bits == 8:
            G = np.fromfile(f, dtype=np.uint8, count=N * P).reshape((N, P), order="F")
        elif bits == 2:
            nb = (N + 3) // 4
            raw = np.fromfile(f, dtype=np.uint8, count=nb * P).reshape((nb, P), order="F")
            G = np.empty((4 * nb, P), dtype=np.uint8, order="F")
            for k in range(4):
                G[k::4, :] = (raw >> (2 * k)) & 3
            G = np.asfortranarray(G[:N, :])
            if (G == 3).any():
                raise ValueError("panel file holds a missing genotype (code 3): impute before loading")
        else:
            raise ValueError(f"panel file with {bits} bits per genotype")
    return G


# ----------------------------------------------------------------------------------------------
# PLINK binary filesets (.bed / .bim / .fam): DESIGN.md section 2, "PLINK .bed panels"
# ----------------------------------------------------------------------------------------------
BED_POLICIES = ("error", "mean", "round")


def _bed_path(path):
    """x.bed for "x.bed" or the prefix "x"."""
    p = os.fspath(path)
    return p if p.endswith(".bed") else p + ".bed"


def is_bed_file(path):
    """True for a SNP-major PLINK .bed file (magic 6c 1b 01); the sample-major form (6c 1b 00) raises ValueError."""
    if not isinstance(path, (str, os.PathLike)):
        return False
    try:
        with open(path, "rb") as f:
            magic = f.read(3)
    except OSError:
        return False
    if magic == b"\x6c\x1b\x00":
        raise ValueError(f"{path} is a sample-major .bed file (magic 6c 1b 00): only the SNP-major form (6c 1b 01) is read; convert it with PLINK")
    return magic == b"\x6c\x1b\x01"


def _read_table(path, ncol, what):
    rows = []
    with open(path) as f:
        for ln, line in enumerate(f, 1):
            t = line.split()
            if not t:
                continue
            if len(t) < ncol:
                raise ValueError(f"{path}, line {ln}: {what} needs {ncol} columns")
            rows.append(t)
    return rows


def read_plink(path):
    """A PLINK binary fileset, `x.bed` or the prefix `x`, without decoding it: {"bed": np.memmap of the packed columns, (P, ceil(n/4))
    uint8, one row per SNP; "n", "P"; "fid", "iid" (.fam); "chr", "snp", "pos", "a1", "a2" (.bim); "path"}."""
    bed = _bed_path(path)
    stem = bed[:-4]
    for ext in (".bed", ".bim", ".fam"):
        if not os.path.isfile(stem + ext):
            raise ValueError(f"PLINK fileset {stem}: {stem + ext} is absent (a .bed needs its .bim and .fam)")
    if not is_bed_file(bed):
        raise ValueError(f"{bed} is not a PLINK .bed file (magic 6c 1b 01)")
    fam = _read_table(stem + ".fam", 2, "a .fam line")
    bim = _read_table(stem + ".bim", 6, "a .bim line")
    n, P = len(fam), len(bim)
    nb = (n + 3) // 4
    size = os.path.getsize(bed)
    if n < 1 or P < 1 or size != 3 + P * nb:
        raise ValueError(f"{bed} holds {size} bytes; {P} SNPs (.bim) of {n} samples (.fam) need 3 + {P} x {nb} = {3 + P * nb}")
    return dict(bed=np.memmap(bed, dtype=np.uint8, mode="r", offset=3, shape=(P, nb)), n=n, P=P, path=bed,
                fid=[t[0] for t in fam], iid=[t[1] for t in fam], chr=[t[0] for t in bim], snp=[t[1] for t in bim],
                pos=[int(float(t[3])) for t in bim], a1=[t[4] for t in bim], a2=[t[5] for t in bim])


def write_plink(prefix, G, iid=None, snp=None, chr=None, missing=None):
    """Writes prefix.bed / .bim / .fam from an N x P array of A1 counts 0/1/2; missing: an optional N x P boolean mask of missing calls.
    iid, snp, chr default to 1..N, snp1..snpP and chromosome 1; alleles are written as A (A1) and B (A2).  Returns the .bed path."""
    G = np.asarray(G)
    if G.ndim != 2 or G.shape[0] < 1 or G.shape[1] < 1:
        raise ValueError("write_plink: an N x P array of genotype codes")
    N, P = G.shape
    miss = np.zeros((N, P), dtype=bool) if missing is None else np.asarray(missing, dtype=bool)
    if miss.shape != (N, P):
        raise ValueError("write_plink: the missing mask has the shape of G")
    if not np.all(np.isin(G[~miss], (0, 1, 2))):
        raise ValueError("write_plink: genotype codes are the A1 counts 0, 1, 2")
    code = np.array([3, 2, 0], dtype=np.uint8)[np.where(miss, 0, G).astype(np.int64)]   # A1 count -> two-bit value
    code[miss] = 1
    nb = (N + 3) // 4
    pad = np.zeros((4 * nb, P), dtype=np.uint8)
    pad[:N] = code
    packed = (pad[0::4] | (pad[1::4] << 2) | (pad[2::4] << 4) | (pad[3::4] << 6)).T   # (P, nb)
    iid = [str(i + 1) for i in range(N)] if iid is None else [str(a) for a in iid]
    snp = [f"snp{j + 1}" for j in range(P)] if snp is None else [str(a) for a in snp]
    chr = ["1"] * P if chr is None else [str(a) for a in chr]
    if len(iid) != N or len(snp) != P or len(chr) != P:
        raise ValueError("write_plink: one iid per row, one snp and chr per column")
    stem = _bed_path(prefix)[:-4]
    with open(stem + ".bed", "wb") as f:
        f.write(b"\x6c\x1b\x01")
        f.write(np.ascontiguousarray(packed).tobytes())
    with open(stem + ".fam", "w") as f:
        for a in iid:
            f.write(f"{a} {a} 0 0 0 -9\n")
    with open(stem + ".bim", "w") as f:
        for j in range(P):
            f.write(f"{chr[j]}\t{snp[j]}\t0\t{j + 1}\tA\tB\n")
    return stem + ".bed"


def bed_round_code(total, n_obs):
    """The code a missing call takes under "round": the nearest code to the mean of the observed calls, ties up, in integers."""
    total, n_obs = np.asarray(total, dtype=np.int64), np.asarray(n_obs, dtype=np.int64)
    return np.where(n_obs > 0, (2 * total + n_obs) // np.maximum(2 * n_obs, 1), 0)


def decode_bed(bed, n_file, rows=None, cols=None, allele=1, missing="mean", counts=False):
    """Host decoder of packed .bed columns (read_plink()["bed"]): the (N, P) matrix of allele counts of the selected rows (file
    samples, any order, repeats allowed; None: all) and columns, with the imputation rules of the device kernels (ngp_bed.h):
    "error" refuses a missing call among the selected rows, "round" fills in (2 sum + n_obs) // (2 n_obs) of its column (uint8 result,
    as under "error"), "mean" the mean of the observed calls (float64 result); a column without an observed call is all zero.
    counts=True also returns the (P, 4) numbers of 0, 1, 2 and missing calls."""
    if missing not in BED_POLICIES:
        raise ValueError(f"missing-call policy {missing!r}: one of {BED_POLICIES}")
    if allele not in (1, 2):
        raise ValueError("allele: 1 (count A1) or 2 (count A2)")
    bed = np.asarray(bed) if cols is None else np.asarray(bed)[cols]
    n_file = int(n_file)
    if bed.ndim != 2 or bed.dtype != np.uint8 or bed.shape[1] < (n_file + 3) // 4:
        raise ValueError("decode_bed: a uint8 array of (P, stride >= ceil(n_file / 4)), one row per SNP")
    idx = np.arange(n_file) if rows is None else np.asarray(rows, dtype=np.int64)
    if idx.ndim != 1 or (len(idx) and (idx.min() < 0 or idx.max() >= n_file)):
        raise ValueError(f"decode_bed: rows outside the file's {n_file} samples")
    lut = np.array([2, 3, 1, 0] if allele == 1 else [0, 3, 1, 2], dtype=np.uint8)   # two-bit value -> count, 3 = missing
    G = lut[(bed[:, idx >> 2] >> (2 * (idx & 3)).astype(np.uint8)) & 3].T             # (N, P)
    miss = G == 3
    cnt = np.stack([(G == v).sum(axis=0) for v in range(4)], axis=1).astype(np.int64)
    total, n_obs = cnt[:, 1] + 2 * cnt[:, 2], cnt[:, 0] + cnt[:, 1] + cnt[:, 2]
    if missing == "error":
        if miss.any():
            j = int(np.flatnonzero(cnt[:, 3])[0])
            raise ValueError(f"column {j} holds {int(cnt[j, 3])} missing calls")
        out = np.asfortranarray(G)
    elif missing == "round":
        out = np.asfortranarray(np.where(miss, bed_round_code(total, n_obs).astype(np.uint8)[None, :], G))
    else:
        mu = np.where(n_obs > 0, total / np.maximum(n_obs, 1), 0.0)
        out = np.asfortranarray(np.where(miss, mu[None, :], G.astype(np.float64)))
    return (out, cnt) if counts else out


class _BedSource:
    """A marker set that stays packed: the memmap of a .bed file's columns and the file samples of the panel's rows.  It has the
    `shape` of the matrix it stands for; panel_columns_bed decodes it on the device, decode() on the host."""
    ndim = 2

    def __init__(self, info, rows, allele, missing):
        self.info, self.rows, self.allele, self.missing = info, rows, int(allele), missing
        self.shape = (info["n"] if rows is None else len(rows), info["P"])
        self.dtype = np.dtype(np.float64 if missing == "mean" else np.uint8)
        self.counts = None

    def decode(self):
        out, self.counts = decode_bed(self.info["bed"], self.info["n"], rows=self.rows, allele=self.allele, missing=self.missing, counts=True)
        return out


def _is_bed(M):
    return isinstance(M, _BedSource)


def _bed_rows(info, ids):
    """The file sample of every record: ids matched, as strings, to the .fam IID (the first sample of an IID listed twice)."""
    at = {}
    for k, a in enumerate(info["iid"]):
        at.setdefault(a, k)
    rows = np.empty(len(ids), dtype=np.int64)
    for i, a in enumerate(ids):
        if a not in at:
            raise ValueError(f"genoID: {a!r} (record {i + 1}) is not an IID of {info['path'][:-4]}.fam")
        rows[i] = at[a]
    return rows


def snp_stats(info, counts):
    """Per-SNP figures of a loaded .bed set from the (P, 4) counts: {"snp", "a1", "a2", "n0", "n1", "n2", "nMissing", "freq"}; freq is
    the frequency of the counted allele among the observed calls (NaN without one)."""
    c = np.asarray(counts, dtype=np.int64)
    n_obs = c[:, 0] + c[:, 1] + c[:, 2]
    freq = np.where(n_obs > 0, (c[:, 1] + 2 * c[:, 2]) / np.maximum(2 * n_obs, 1), np.nan)
    return dict(snp=list(info["snp"]), a1=list(info["a1"]), a2=list(info["a2"]), n0=c[:, 0].copy(), n1=c[:, 1].copy(), n2=c[:, 2].copy(),
                nMissing=c[:, 3].copy(), freq=freq)


def write_snp_stats(path, st):
    with open(path, "w") as f:
        f.write("snp a1 a2 n0 n1 n2 nMissing freq\n")
        for j in range(len(st["snp"])):
            f.write(f"{st['snp'][j]} {st['a1'][j]} {st['a2'][j]} {int(st['n0'][j])} {int(st['n1'][j])} {int(st['n2'][j])} {int(st['nMissing'][j])} {float(st['freq'][j])!r}\n")


def write_bim_map(path, info):
    """The map file prep2RegionData reads (header snpID,snpOrder,chrID) from a fileset's .bim."""
    with open(path, "w") as f:
        f.write("snpID,snpOrder,chrID\n")
        for j, (s, c) in enumerate(zip(info["snp"], info["chr"])):
            f.write(f"{s},{j + 1},{c}\n")


def prep2RegionData(outPutFolder, markerSet, mapFile, fixedRegSize):
    """Region ranges from a map file with header snpID,snpOrder,chrID (src/misc.jl:163-215).
    99 = one region per chromosome, 9999 = whole genome, anything else = windows of that many SNPs inside each
    chromosome.  Writes groupInfo_<set>.txt like the reference and returns 0-based [start, stop) pairs."""
    import csv
    with open(mapFile, newline="") as f:
        rows = list(csv.DictReader(f))
    chrs = [r["chrID"] for r in rows]
    groups, g = [], 0
    if fixedRegSize == 9999:
        groups = [1] * len(rows)
    else:
        order = []
        for c in chrs:
            if c not in order:
                order.append(c)
        gid = {}
        for c in order:
            idx = [i for i, x in enumerate(chrs) if x == c]
            if fixedRegSize == 99:
                g += 1
                for i in idx:
                    gid[i] = g
            else:
                for k, i in enumerate(idx):
                    gid[i] = g + 1 + k // int(fixedRegSize)
                g += (len(idx) + int(fixedRegSize) - 1) // int(fixedRegSize)
        groups = [gid[i] for i in range(len(rows))]
    if outPutFolder is not None:
        with open(os.path.join(outPutFolder, f"groupInfo_{markerSet}.txt"), "w") as f:
            f.write("snpID\tsnpOrder\tchrID\tgroupID\n")
            for r, gg in zip(rows, groups):
                f.write(f"{r['snpID']}\t{r['snpOrder']}\t{r['chrID']}\t{gg}\n")
    regions, start = [], 0
    for i in range(1, len(groups) + 1):
        if i == len(groups) or groups[i] != groups[start]:
            regions.append((start, i))
            start = i
    return regions


def _regions_for(prior, P, map_path, out_folder, set_name):
    """M[set][:regionArray] (src/mme.jl:324-358)."""
    if isinstance(prior, (BayesBType, BayesLogVarType)):   # one region per locus (src/mme.jl:356, :421)
        return [(j, j + 1) for j in range(P)]
    if isinstance(prior, (BayesCType, BayesRType, BayesRCType)):  # one variance for the set (nVarCov = 1, src/mme.jl:370, :381; BayesRCπ: one per annotation, no regions)
        return [(0, P)]
    if not map_path:
        if prior.r == 1:
            return [(j, j + 1) for j in range(P)]
        if prior.r == 9999:
            return [(0, P)]
        raise ValueError("Please enter a valid region size (1 or 9999)")  # src/mme.jl:343
    return prep2RegionData(out_folder, set_name, map_path, prior.r)


# ----------------------------------------------------------------------------------------------
# output files (src/outFiles.jl:17-21, headers src/mme.jl:545-595, rows src/samplers.jl:57-103)
# ----------------------------------------------------------------------------------------------
def _out(folder, name, row):
    with open(os.path.join(folder, f"{name}Out"), "a") as f:
        f.write("\t".join(row) + "\n")


def random_file_names(g):
    """(u file, varU file, varU header) of the (1|g) set: Julia prints the key :(1|g) as "1 | g" (u$zSet / varU$zSet, src/samplers.jl:63-73,
    src/outFiles.jl:17-21) and heads the varU file with join(zSet.args)[2:end] = "1g" (src/mme.jl:548-556)."""
    return f"u1 | {g}", f"varU1 | {g}", f"1{g}"


def _rd_files(rd):
    """(u file, varU file, varU header) of a random-effect set: a (1|g) term, or a GBLUP term, whose key is the Symbol of its SNP term:
    u<name> with the header Ind1 .. IndN and varU<name> headed <name> (src/mme.jl:549-552; the reference sizes the Ind names by the
    number of MARKERS, src/prepMatVec.jl:126 -- a slip, not copied: one name per individual)."""
    return rd["files"] if "files" in rd else random_file_names(rd["g"])


def _rd_k(rd):
    return len(rd["members"]) if "members" in rd else 1


def _rd_headers(rd):
    """[(file, header fields)] of a random-effect set.  A correlated (Tuple) set writes one u<member> file per component, each headed by
    the levels, and ONE varU file named as Julia prints the key, varU(:ID, :Dam), headed ID_Dam_1 .. ID_Dam_k^2 (src/mme.jl:557-563)."""
    if "members" not in rd:
        un, vn, vh = _rd_files(rd)
        return [(un, rd["levels"]), (vn, [vh])]
    mem, k = rd["members"], len(rd["members"])
    return [(f"u{m}", rd["levels"]) for m in mem] + [(_tuple_var_file(mem), ["_".join(mem) + f"_{i + 1}" for i in range(k * k)])]


def _tuple_var_file(members):
    return "varU(" + ", ".join(f":{m}" for m in members) + ")"


def _rd_rows(rd, u, varU):
    """[(file, fields)] of one kept sample of a random-effect set: u (q, or q x k flat with the components of a level adjacent) and varU
    (one value, or k x k row-major; written column by column: hcat(reduce(hcat, varU)...), src/samplers.jl:63-74)."""
    if "members" not in rd:
        un, vn, _ = _rd_files(rd)
        return [(un, _fmt(u)), (vn, _fmt(varU))]
    mem, k = rd["members"], len(rd["members"])
    U = np.asarray(u, dtype=np.float64).reshape(-1, k)
    return [(f"u{m}", _fmt(U[:, c])) for c, m in enumerate(mem)] + [(_tuple_var_file(mem), _fmt(np.asarray(varU, dtype=np.float64).reshape(k, k).T.ravel()))]


def _var_names(s):
    """Header of var<set>Out: reg_r (src/mme.jl:593-595); for correlated sets one column per entry of the region's k x k matrix."""
    if s["k"] > 1:
        return [f"reg_{r + 1}_{a + 1}{b + 1}" for r in range(s["nreg"]) for a in range(s["k"]) for b in range(s["k"])]
    return [f"reg_{r + 1}" for r in range(s["nvb"])]


def _fmt(x):
    return [repr(float(v)) for v in np.atleast_1d(x)]


def summaryMCMC(param, outFolder=None):
    """Posterior mean = column mean of <outFolder>/<param>Out, first row is the header (src/misc.jl:241-244)."""
    outFolder = outFolder or os.path.join(os.getcwd(), "outMCMC")
    return np.loadtxt(os.path.join(outFolder, f"{param}Out"), delimiter="\t", skiprows=1, ndmin=2).mean(axis=0, keepdims=True)


# ----------------------------------------------------------------------------------------------
# convergence diagnostics (ngp_enable_diagnostics; DESIGN.md section 2, "Convergence diagnostics")
# ----------------------------------------------------------------------------------------------
def pool_diagnostics(per_chain):
    """Chains' diagnostics (Sampler.diagnostics()) pooled on the host.  The sequences of the split-R-hat are every half with n_s >= 2 of
    every chain: W = mean(var_s), n_bar = mean(n_s), B/n = var(mean_s, ddof=1), var+ = (n_bar - 1) / n_bar W + B/n, rhat = sqrt(var+ / W)
    (NaN with fewer than two sequences or W = 0).  mean: the n-weighted mean of the chains' means; sd = sqrt(var+) (with a single
    sequence: of its variance); ess = sum of the chains'; mcse = sd / sqrt(ess); truncated: the OR over the chains."""
    per_chain = list(per_chain)
    D = len(per_chain[0]["mean"])
    seq = [(float(c["half_n"][h]), np.asarray(c["half_mean"][h], dtype=np.float64), np.asarray(c["half_var"][h], dtype=np.float64))
           for c in per_chain for h in range(2) if c["half_n"][h] >= 2]
    ns = np.array([float(c["n"]) for c in per_chain])
    with np.errstate(all="ignore"):
        mean = sum(n * np.asarray(c["mean"], dtype=np.float64) for n, c in zip(ns, per_chain)) / ns.sum()
        ess = sum(np.asarray(c["ess"], dtype=np.float64) for c in per_chain)
        W = np.mean([v for _, _, v in seq], axis=0) if seq else np.full(D, np.nan)
        if len(seq) >= 2:
            n_bar = float(np.mean([n for n, _, _ in seq]))
            var_plus = (n_bar - 1.0) / n_bar * W + np.var(np.array([m for _, m, _ in seq]), axis=0, ddof=1)
            rhat = np.where(W > 0, np.sqrt(var_plus / W), np.nan)
        else:
            var_plus, rhat = W, np.full(D, np.nan)
        sd = np.sqrt(var_plus)
        truncated = np.any([np.asarray(c["truncated"]) > 0 for c in per_chain], axis=0).astype(np.float64)
        return dict(n=int(ns.sum()), mean=mean, sd=sd, mcse=sd / np.sqrt(ess), ess=ess, rhat=rhat, truncated=truncated)


def _diagnostics_option(diagnostics):
    """runLMEM(diagnostics=False | True | {"lags": L}) -> None or the lags.  Host checks only."""
    if diagnostics is False or diagnostics is None:
        return None
    if diagnostics is True:
        return 64
    if isinstance(diagnostics, dict) and set(diagnostics) == {"lags"}:
        L = diagnostics["lags"]
        if isinstance(L, (int, np.integer)) and not isinstance(L, bool) and 2 <= int(L) <= 256 and int(L) % 2 == 0:
            return int(L)
        raise ValueError("diagnostics: lags must be an even integer, 2 .. 256")
    raise ValueError('diagnostics: False, True or {"lags": L}')


def _diagnostics_names(D, sets, fixed_names, intercept, randoms=(), nthr=0):
    """One name per monitored scalar, "<Out-file stem>:<column header>", in the order of the sample record (csrc/ngp_state.h,
    diag_layout), from the headers _write_headers gives the *Out files and the indexing samples_to_out_files cuts their rows with."""
    fx = list(fixed_names)
    head = ["varE:e", f"b:{fx[0]}" if intercept and fx else "b:intercept"] + [f"b:{nm}" for nm in (fx[1:] if intercept else fx)]
    for rd in randoms:   # u: the levels in order; the k components of a level of a correlated set adjacent
        if "members" not in rd:
            head += [f"{_rd_files(rd)[0]}:{lv}" for lv in rd["levels"]]
        else:
            head += [f"u{m}:{lv}" for lv in rd["levels"] for m in rd["members"]]
    for rd in randoms:   # varU: row-major in the record, column by column in the file
        file, fields = _rd_headers(rd)[-1]
        k = _rd_k(rd)
        head += [f"{file}:{fields[b * k + a]}" for a in range(k) for b in range(k)]
    tail = []
    for s in sets:
        tail += [f"var{s['name']}:{nm}" for nm in _var_names(s)]
    for s in sets:       # piHat[2] of every set; only BayesB / BayesC sets write it (as pi<set>Out)
        stem = f"pi{s['name']}" if isinstance(s["prior"], (BayesBType, BayesCType)) else f"piHat{s['name']}"
        tail += [f"{stem}:pi1", f"{stem}:pi2"]
    for s in sets:
        K = len(s["prior"].pi) * s.get("A", 1) if isinstance(s["prior"], (BayesRType, BayesRCType)) else 0
        tail += [f"pi{s['name']}:pi{v + 1}" for v in range(K)]
    for s in sorted((s for s in sets if isinstance(s["prior"], BayesLogVarType)), key=lambda s: s["lv"]):
        # (c<set>Out has ncov columns; the slots behind them are constants of the record, named apart so that a file's rows are its columns)
        tail += [f"c{s['name']}:c{v + 1}" if v < s["ncov"] else f"cUnused{s['name']}:slot{v + 1}" for v in range(16)] + [f"varZeta{s['name']}:varZeta"]
    tail += [f"threshold:t{c + 2}" for c in range(nthr)]
    P = D - len(head) - len(tail)
    if P < 0:
        raise ValueError("internal: the monitored vector is shorter than the names of the model's parameters")
    beta = [f"beta:col{j + 1}" for j in range(P)]   # (columns no set owns: the padding between correlated sets)
    for s in sets:
        for m, nm in enumerate(s["members"]):
            for j, c in enumerate(np.asarray(s["cols"])[:, m]):
                beta[int(c)] = f"beta{nm}:M{j + 1}"
    return head + beta + tail


def _worst(names, d):
    ess, rhat = np.asarray(d["ess"], dtype=np.float64), np.asarray(d.get("rhat", np.full(len(names), np.nan)), dtype=np.float64)
    lo = [int(i) for i in np.argsort(np.where(np.isnan(ess), np.inf, ess), kind="stable")[:10]]
    hi = [int(i) for i in np.argsort(-np.where(np.isnan(rhat), -np.inf, rhat), kind="stable")[:10] if not np.isnan(rhat[i])]
    return dict(ess=[names[i] for i in lo], rhat=[names[i] for i in hi])


def write_convergence_file(path, names, d):
    """convergence.txt: a header, then one line per parameter: name mean sd mcse ess rhat truncated (tab-separated, every digit)."""
    rhat = d.get("rhat", np.full(len(names), np.nan))
    with open(path, "w") as f:
        f.write("\t".join(["name", "mean", "sd", "mcse", "ess", "rhat", "truncated"]) + "\n")
        for i, nm in enumerate(names):
            f.write("\t".join([nm] + [repr(float(d[k][i])) for k in ("mean", "sd", "mcse", "ess")] + [repr(float(rhat[i])), str(int(d["truncated"][i]))]) + "\n")


def read_convergence_file(path):
    """dict(names, mean, sd, mcse, ess, rhat, truncated) of a convergence.txt."""
    rows = [ln.rstrip("\n").split("\t") for ln in open(path)][1:]
    out = dict(names=[r[0] for r in rows])
    for j, k in enumerate(("mean", "sd", "mcse", "ess", "rhat", "truncated")):
        out[k] = np.array([float(r[j + 1]) for r in rows], dtype=np.float64)
    return out


def convergencyMCMC(param, summary=False, outFolder=None):
    """The reference's convenience function (docs/src/index.md:62-88) without MCMCChains: the posterior-mean row of <param>Out, as
    summaryMCMC gives it; with summary=True also the convergence.txt rows of that file's columns (a run with diagnostics=True wrote
    them from the device's streaming sums -- the *Out file is not needed for them) as dict(names, mean, sd, mcse, ess, rhat, truncated)."""
    outFolder = outFolder or os.path.join(os.getcwd(), "outMCMC")
    if not summary:
        return summaryMCMC(param, outFolder)
    cv = read_convergence_file(os.path.join(outFolder, "convergence.txt"))
    pick = [i for i, nm in enumerate(cv["names"]) if nm.split(":", 1)[0] == param]
    rows = dict(names=[cv["names"][i].split(":", 1)[1] for i in pick], **{k: cv[k][pick] for k in ("mean", "sd", "mcse", "ess", "rhat", "truncated")})
    mean = summaryMCMC(param, outFolder) if os.path.exists(os.path.join(outFolder, f"{param}Out")) else rows["mean"][None, :]
    return mean, rows


def samples_to_out_files(sample_path, outFolder, sets, intercept, has_fixed, randoms=()):
    """Binary sample stream (ngp_set_sample_file) -> the rows of the reference's *Out text files (src/samplers.jl:56-104), appended
    behind the header rows: the same text, number for number, as writing them at every kept iteration.  Record by record -- one
    kept iteration in memory at a time, every *Out file open for appending -- so a long chain of a large model converts in
    constant memory and an interrupted conversion leaves the rows written so far (the caller keeps the binary file until the
    conversion has succeeded)."""
    from ._lib import iter_sample_file
    handles = {}

    def row(name, fields):
        f = handles.get(name)
        if f is None:
            f = handles[name] = open(os.path.join(outFolder, f"{name}Out"), "a")
        f.write("\t".join(fields) + "\n")

    n = 0
    try:
        for S in iter_sample_file(sample_path):
            n += 1
            row("b", (_fmt(S["b"]) if intercept else []) + (_fmt(S["b_fixed"]) if has_fixed else []))
            row("varE", _fmt(S["varE"]))
            vu_off = 0
            for r, rd in enumerate(randoms):                 # src/samplers.jl:60-75
                kk = _rd_k(rd) ** 2
                for name, fields in _rd_rows(rd, S["u"][r], S["varU"][vu_off:vu_off + kk]):
                    row(name, fields)
                vu_off += kk
            vb_off, cls_off = 0, 0
            for k, s in enumerate(sets):
                K = len(s["prior"].pi) * s.get("A", 1) if isinstance(s["prior"], (BayesRType, BayesRCType)) else 0
                for m, nm in enumerate(s["members"]):
                    row(f"beta{nm}", _fmt(S["beta"][s["cols"][:, m]]))
                    row(f"delta{nm}", [str(int(v)) for v in S["delta"][s["cols"][:, m]]])
                if isinstance(s["prior"], (BayesBType, BayesCType)):
                    row(f"pi{s['name']}", _fmt(S["piHat"][2 * k:2 * k + 2]))
                if K:
                    row(f"pi{s['name']}", _fmt(S["class_pi"][cls_off:cls_off + K]))
                if isinstance(s["prior"], BayesRCType):       # src/samplers.jl:85-87
                    row(f"annot{s['name']}", [str(int(v)) for v in S["annotCat"][s["id"]]])
                if isinstance(s["prior"], BayesLogVarType):   # src/samplers.jl:89-92
                    row(f"c{s['name']}", _fmt(S["lv_c"][s["lv"]]))
                    row(f"varZeta{s['name']}", _fmt(S["lv_varZeta"][s["lv"]]))
                row(f"var{s['name']}", _fmt(S["varBeta"][vb_off:vb_off + s["nvb"]]))
                vb_off += s["nvb"]
                cls_off += K
            if "thr" in S:                                    # an ordered trait of C >= 3 classes: t_2 .. t_{C-1} of this draw
                row("threshold", _fmt(S["thr"]))
    finally:
        for f in handles.values():
            f.close()
    return n


# ----------------------------------------------------------------------------------------------
# runLMEM (src/MCMC.jl:31-41)
# ----------------------------------------------------------------------------------------------
def runLMEM(formula, userData, nChain, nBurn, nThin, myHints=None, blockThese=None, outFolder="outMCMC", VCV=None, userPedData=None,
            summaryStat=None, seed=1, chain=0, device=0, samples="text", overwrite=False, engine=None, storage=None, chains=1, max_shards=None,
            predict=None, predict_ids=None, windows=None, windowThreshold=0.01, genomicVariance=False, holdout=None, missing="error", folds=None,
            foldSeed=1, trait="gaussian", censored=None, thresholdStep="albert-chib", classProb=False, singleStep=None, diagnostics=False, genoID=None, missingGeno=None, alleleCount=1, sparseFixed="auto"):
    """Runs the chain on the GPU and writes the reference's *Out files.

    Differences from the reference, all deliberate: (1) `seed`/`chain` key the random streams (the reference never
    seeds); (2) an existing non-empty outFolder is refused unless overwrite=True (the reference deletes it,
    src/misc.jl:221-227); (3) samples="none" skips the per-iteration text rows and only returns posterior means;
    (4) storage="u8" keeps the panel one byte per genotype on the device, centred analytically (ngp_set_storage: a quarter of
    the memory, no fp32 rounding of the panel) -- every SNP set must then hold integer codes 0..255 (uint8 arrays, binary panel
    files, or text files whose values are such integers); (5) chains=K runs K independent chains (chain ids chain .. chain+K-1, the
    same seed) over ONE copy of the panel on the device -- one fused sweep launch per iteration where the engine serves it (the result's
    "fused" says whether it did; a warning otherwise)
    (ngp_share_panel + ngp_run_many), side by side otherwise; every chain is bit for bit the chain it is alone with that layout,
    writes its own *Out files to outFolder/chain<c>/, and the returned means are pooled over the chains (res["chains"] holds each);
    (6) with userPedData (a pedigree file, or rows of ID / Sire / Dam) the data stay in the caller's record order -- the reference
    re-sorts the data frame by pedigree position; the levels of a PED(col) set are the animals in pedigree (parents-first) order either
    way, and a record whose col is 0 (unknown: an all-zero row of Z in the reference) is refused.
    (7) correlated (Tuple) random effects -- VCV={("ID", "Dam"): Random("A", V)} with V a k x k covariance over the PED terms named, the
    direct-maternal model; a 0 in such a column is a record without a level -- are drawn from the EXACT Gibbs conditional: the
    reference's sampleZ!(::Tuple) leaves Z_ID'Z_Dam u_Dam of the other levels in a level's right-hand side (src/functions.jl:81-82), the
    device subtracts it ("Correlated random-effect sets").  The two agree when no record links two different levels.  One
    u<member>Out file per component and one varU(:ID, :Dam)Out (the matrix column by column); res["random"][("ID", "Dam")] holds u
    (k x q), varU (k x k) and levels.  Refused: a GBLUP term or a (1|g) term inside a tuple, summaryStat on a tuple.
    (8) predict={name: source for every SNP(...) term} predicts new individuals on the device: each source (a text file, an .npy
    file, an NGPPNL01 file or an array) holds the term's columns for the SAME Np individuals; they are centred with the TRAINING column
    means and every kept draw accumulates X_new beta (ngp_begin_prediction_panel; DESIGN.md section 2, "Prediction").  The result gains
    res["predict"] = {"ids", "mean", "sd", "sets": {name: {"mean", "sd"}}} (mean and SD of the breeding value over the kept draws, all
    marker sets together and per set; correlated sets count as the one set they are, under their joined name) and outFolder/gebvPredict.txt
    holds the same columns: ID mean sd mean_<set> sd_<set> ...  predict_ids names the individuals (default 1..Np).  With chains=K the
    sums are pooled over the chains and res["chains"][c]["predict"] is each chain's own.  GBLUP terms together with predict= raise
    NotImplementedError; without predict= nothing differs.
    (9) windows={name: W | [(a, b), ...]} (or genomicVariance=True with windows={} for set and total slots only) forms the genomic
    variance of every kept draw on the device (ngp_enable_genomic_variance; DESIGN.md section 2, "Genomic variance"): var(X beta) over the
    training individuals per window, per marker set and in all, the share q = V / V_g of each, r = V_g / (V_g + varE), and the window
    posterior probability of association WPPA = share of the kept draws with q > windowThreshold.  An integer W means windows of W SNPs
    -- inside each chromosome where the SNP term has a map file (prep2RegionData), plain windows of W columns otherwise; a list holds
    half-open 0-based column ranges of the set.  Files in the *Out format (summaryMCMC reads them): windowVar<set>Out (columns win_1 ...)
    and genVarOut (one column per set, then total, then ratio), per chain under chain<c>/ with chains=K; gwas<set>.txt in outFolder:
    window, first and last SNP (1-based), mean V, mean q, SD of q, WPPA.  res["variance"] holds the same, pooled over the chains
    (res["chains"][c]["variance"]: each chain's own).  Not available for a member of a correlated (Tuple) unit or a GBLUP term.
    (10) held-out records (ngp_set_holdout; DESIGN.md section 2, "Held-out records"): holdout=rows (0-based records) keeps these records
    in the panel but never reads their response -- each iteration redraws it from its conditional, each kept draw accumulates the
    record's fitted value (intercept, fixed, random and marker terms).  missing="holdout" does the same for the records whose response is
    NaN (the default "error" refuses them as before).  res["holdout"] = {"rows", "y", "yhat", "sd", "n"} and outFolder/holdoutPredict.txt
    (record y yhat sd, records counted from 1) hold the result, pooled over the chains with chains=K.  folds=K (2..8) is K-fold
    cross-validation in one run: the records with a response are dealt into K folds (deal_folds: np.random.default_rng(foldSeed)
    .permutation, round-robin), K chains (the same seed, chain ids chain .. chain+K-1) run over ONE copy of the panel as chains=K does,
    chain c holding out fold c.  res["cv"] = {"fold", "yhat", "sd" (N entries, NaN where not validated), "accuracy" (Pearson correlation
    of yhat and y), "slope" (regression of y on yhat), "mse", "per_fold", "pooled_over_folds": True -- the returned marker means are
    pooled over the fold-chains}, and cvPredict.txt holds record fold y yhat sd.  folds= with chains= or holdout= raises ValueError.
    (11) liability traits (ngp_set_liability_classes / ngp_set_liability_bounds; DESIGN.md section 2, "Liability traits").
    trait="categorical": a threshold (probit) model -- the sorted distinct values of the response become the classes 1..C (2..8), the
    latent liability of every record is redrawn each iteration, the residual variance is 1 (VCV["e"], if given, must have the value 1,
    else ValueError; varEOut is all ones), the thresholds t_2 .. t_{C-1} are drawn for C >= 3 (t_1 = 0): res["thresholds"] = {"mean",
    "sd"} (empty for two classes), pooled over the chains, res["classes"] the response value of every class.  Effects, predict=,
    holdout=, missing= and folds= work as they are and report on the LIABILITY scale (res["cv"]'s accuracy then compares liabilities
    with class values: a rank measure only).  censored={"lower": column or array, "upper": column or array}: a Tobit model -- a record
    with lower == upper is exact and takes that value, NaN or an infinity means open on that side, and the response column is ignored on
    the censored records; varE is sampled as usual.  The two exclude one another.  With samples="text" and C >= 3 thresholdOut holds the
    thresholds of every kept draw (columns t2 .. t{C-1}; per chain under chain<c>/ with chains=K); its column means are res["thresholds"]["mean"]
    (the text round-trips every double).
    (12) ordered traits on the scale of the trait (ngp_set_threshold_step / ngp_enable_class_probabilities; DESIGN.md section 2,
    "Cowles' threshold step", "Class probabilities"), both with trait="categorical" only (ValueError otherwise).
    thresholdStep="cowles" (three classes or more, else ValueError) moves the thresholds by Cowles' joint Metropolis-Hastings step,
    which mixes where a class holds thousands of records and the default "albert-chib" step barely moves; res["thresholds"] gains
    "acceptance" (accepted / proposed, pooled over the chains) and "sigma" (the proposal SD after burn-in, the mean over the chains).
    classProb=True, together with any of folds= / holdout= / missing="holdout" (ValueError without one), accumulates P(class) of every
    held-out record per kept draw: res["holdout"]["prob"] (records x C, beside "rows") and outFolder/holdoutProb.txt; with folds=K
    res["cv"]["prob"] (N x C, NaN where not validated), "brier", "logloss", "class_accuracy" (arg-max class) and, for two classes,
    "auc" (class_metrics), each also in every entry of "per_fold", and cvProb.txt: record fold class p1 .. pC (records from 1, fold -1
    and class 0 where there is none).  holdoutPredict.txt and cvPredict.txt keep their columns.
    (13) single-step GBLUP (ngp_grm_single_step / ngp_add_random_set_hybrid; DESIGN.md section 2, "Hybrid random-effect sets"): a
    PED(col) term with VCV={col: Random("H", v, type=1|2)} and singleStep={col: {"geno": path | array, "ids": [...], "w": 0.05}} has one
    breeding value per animal of the pedigree over H^-1 = A^-1 + [0 0; 0 inv((1 - w) G + w A22) - inv(A22)]; ids names the genotyped
    animals in the row order of geno, all of them in the pedigree (an unknown or repeated ID: ValueError).  The set's levels are
    renumbered -- the animals without a genotype first, in pedigree order, then the genotyped ones in ids order -- and u<col>Out's header
    and res["random"][col]["levels"] name them in that order.  G is built on the device (type: VanRaden's method), A22 by Colleau's
    method on the host; chains=K share the dense block by reference.  "H" without singleStep[col], singleStep for a term whose prior is
    not "H": ValueError; "H" inside a tuple key and summaryStat on the term: NotImplementedError.  G is not scaled to A22.
    diagnostics=True (or {"lags": L}, L even in 2..256; True means 64) follows every monitored scalar -- the doubles of a kept sample:
    varE, b, the fixed and random effects, every marker effect and variance, pi -- with a streaming lag-window autocovariance on the
    device (ngp_enable_diagnostics; DESIGN.md section 2, "Convergence diagnostics").  res["diagnostics"] = {"names", "n", "mean", "sd",
    "mcse", "ess", "rhat", "truncated", "chains": [each chain's own], "worst": {"ess": the ten lowest-ESS names, "rhat": the ten largest}};
    names are "<Out-file stem>:<column header>" (betaM1:M7, varM1:reg_1, varE:e).  outFolder/convergence.txt holds one line per
    parameter: name mean sd mcse ess rhat truncated.  chains=K pools the chains into a split-R-hat (pool_diagnostics; the halves part at
    the middle of the planned kept draws); folds=K pools nothing -- its chains see different data -- and reports per chain only
    (convergence.txt under chain<c>/).  truncated = 1: the positive sequence had not ended inside the window, the ESS is an upper
    bound -- raise lags or thin more.  convergencyMCMC(param, summary=True, outFolder=...) returns a file's rows of it.
    (14) PLINK binary filesets (ngp_panel_columns_bed; DESIGN.md section 2, "PLINK .bed panels"): SNP(M1, "geno.bed") -- recognised by
    the file's magic -- sends the packed columns to the device as they are in the file; no host matrix of the panel is formed.
    genoID names the data column whose values are matched, as strings, to the .fam IID: the fileset may hold more individuals than the
    records, in any order, and an animal with several records is gathered several times (an ID absent from the .fam: ValueError;
    genoID=None: file order, as many samples as records).  missingGeno says what a missing call becomes: "mean" (the default: the mean
    of the column's observed calls, a centred 0), "round" (the nearest code to that mean; the default, and the only imputing policy,
    with storage="u8") or "error".  alleleCount=1 counts A1 (the .bim's first allele), 2 counts A2.  Nothing is filtered: the numbers of
    0, 1, 2 and missing calls and the allele frequency of every SNP go to outFolder/snpStats<set>.txt (snp a1 a2 n0 n1 n2 nMissing
    freq) and res["sets"][name]["snpStats"].  A term without a map file takes its chromosomes from the .bim (map_<set>.txt is written
    into outFolder and serves regions and windows=).  predict={name: "cand.bed"} loads candidates the same way (predict_ids defaults
    to the .fam IIDs; the .bim must list the training set's SNPs; a missing call takes the training mean, or its rounded code).
    GBLUP terms, singleStep genotypes and members of a correlated (Tuple) unit are decoded on the host (decode_bed) by the same rules.
    (15) sparse fixed-effect sets (ngp_add_fixed_set_sparse; DESIGN.md section 2, "Sparse fixed-effect sets"): a fixed unit -- a term, or
    a blockThese group -- whose design has more than 64 columns (a herd or contemporary-group factor) goes to the device as a sparse
    matrix built from the level codes; no dense design is formed.  sparseFixed=True sends every unit of several columns that way,
    False none (a unit wider than 64 columns is then refused by the library, as before).  The chain does not depend on the route: a
    sparse set is bit for bit the dense set of the same design.  bOut headers and fixed_names keep their form ("herd: b").

    Returns a dict of posterior means taken from the on-device sums."""
    VCV = dict(VCV or {})
    summaryStat = dict(summaryStat or {})
    diag_lags = _diagnostics_option(diagnostics)   # (checked before any device work)
    if missingGeno is None:
        missingGeno = "round" if storage in ("u8", 1) else "mean"
    if missingGeno not in BED_POLICIES:
        raise ValueError(f"missingGeno: one of {BED_POLICIES}, got {missingGeno!r}")
    if missingGeno == "mean" and storage in ("u8", 1):
        raise ValueError('missingGeno="mean" with storage="u8": byte tiles hold genotype codes, a column mean is none; use "round" (or "error")')
    if alleleCount not in (1, 2):
        raise ValueError("alleleCount: 1 (count A1) or 2 (count A2)")
    if not (sparseFixed is True or sparseFixed is False or sparseFixed == "auto"):
        raise ValueError(f'sparseFixed: "auto", True or False, got {sparseFixed!r}')
    parsed = parse_formula(formula, random_effects=True, pedigree=True)
    lhs, intercept, snps = parsed
    has_ped = userPedData is not None and len(userPedData) > 0
    if parsed.ped and not has_ped:
        raise ValueError(f"PED({parsed.ped[0]}) needs userPedData: the pedigree file (ID Sire Dam), or its rows")
    if not snps and not parsed.ped:
        raise ValueError("the accelerated path needs at least one SNP(...) term")
    ss_terms = single_step_terms(singleStep, VCV, parsed, summaryStat)   # (checked before any device work)
    y = np.asarray(userData[lhs], dtype=np.float64)
    liab = _liability_spec(trait, censored, y, userData, VCV)   # (checked before any device work)
    if liab is not None and liab["kind"] == "bounds":          # exact records take their value; the censored ones are not read
        y = liab["y"]
    masks, cv_fold, chains = _holdout_masks(y, holdout, missing, folds, foldSeed, chains)   # (checked before any device work)
    if liab is not None and liab["kind"] == "classes" and missing != "holdout" and np.any(liab["codes"] == 0):
        raise ValueError('trait="categorical": a record has no response (NaN); missing="holdout" predicts such records')
    _ordered_options(trait, liab, thresholdStep, classProb, masks)
    if liab is not None and liab["kind"] == "bounds" and masks is not None and any(len(np.intersect1d(m, liab["rows"])) for m in masks):
        raise ValueError("censored: a censored record cannot be held out as well (holdout=, folds=); records without any bound are missing records")
    ped = None
    if has_ped:   # makePed (src/misc.jl:98-115) once for all PED terms and all chains
        ids = []
        ped_tuples = _random_tuples(VCV, parsed, summaryStat)
        in_ped_tuple = {m for key in ped_tuples for m in key}
        for col in parsed.ped:
            c = [str(a) for a in np.asarray(userData[col]).tolist()]
            if col in in_ped_tuple:   # a 0 in a tuple's column is a record without a level (ngp_add_random_set_tuple, level -1)
                c = [a for a in c if a != "0"]
            if "0" in c:
                raise NotImplementedError(f"PED({col}): a record whose {col} is 0 (unknown) has an all-zero row of Z in the reference; "
                                          "ngp_add_random_set takes a level for every record, so such records are not on the accelerated path")
            ids += c
        table, Ainv = makePed(userPedData, ids)
        ped = dict(table=table, Ainv=Ainv, tuples=ped_tuples, single={col: _single_step_prepare(sp, table, Ainv) for col, sp in ss_terms.items()})
    # weighted residuals, E.str == "D" (src/mme.jl:71-75): w = inv.(d), set on the handle before its panel (the rows are scaled at upload)
    w_res = _residual_weights(VCV.get("e", Random("I", 100.0)), len(y))
    if w_res is not None and storage in ("u8", 1):
        raise NotImplementedError('weighted residuals (Random(d, v)) with storage="u8": compact storage takes no residual weights '
                                  '(its byte tiles are centred analytically); use the default fp32 tiles')
    # folderHandler (src/misc.jl:221-232) -- without the silent rm -r
    if os.path.isdir(outFolder) and os.listdir(outFolder):
        if not overwrite:
            raise FileExistsError(f"output folder {outFolder} exists and is not empty (pass overwrite=True to clear it)")
        for fn in os.listdir(outFolder):
            os.remove(os.path.join(outFolder, fn))
    os.makedirs(outFolder, exist_ok=True)
    # prep: SNP branch (src/prepMatVec.jl:113-134); marker sets become consecutive column ranges of ONE panel.  A term whose prior is
    # Random("G", v) is GBLUP (:122-126): its genotypes go to the GRM builder, never into the panel
    gb_names = gblup_terms(snps, VCV, summaryStat)
    geno_ids = None if genoID is None else [str(a) for a in np.asarray(userData[genoID]).tolist()]
    mats_all = [_genotype_source(t.path, geno_ids, alleleCount, missingGeno) for t in snps]
    tuple_names = {nm for key in VCV if isinstance(key, tuple) for nm in key}
    bed_sets = {t.name: M for t, M in zip(snps, mats_all) if _is_bed(M)}   # (their counts are reported below)
    for t, M in zip(snps, mats_all):
        if _is_bed(M) and not t.map and t.name not in tuple_names and t.name not in gb_names:   # chromosomes from the .bim
            t.map = os.path.join(outFolder, f"map_{t.name}.txt")
            write_bim_map(t.map, M.info)
    # only a plain marker set stays packed for the device: GBLUP genotypes and members of a correlated unit are decoded on the host
    mats_all = [M.decode() if _is_bed(M) and (t.name in gb_names or t.name in tuple_names) else M for t, M in zip(snps, mats_all)]
    for M in mats_all:
        if M.shape[0] != len(y):
            raise ValueError("genotype rows must match the phenotype records (marker files are ordered as the data, runTime.jl:23)")
    gblup = {t.name: dict(M=M, prior=VCV[t.name]) for t, M in zip(snps, mats_all) if t.name in gb_names}
    mats = [M for t, M in zip(snps, mats_all) if t.name not in gb_names]
    snps = [t for t in snps if t.name not in gb_names]
    pmats = _prediction_sources(predict, predict_ids, snps, mats, gb_names, alleleCount, missingGeno, tuple_names)   # (checked before any device work)
    gv_windows = _variance_windows(windows, windowThreshold, genomicVariance, snps, mats, gb_names, VCV)   # (the same)
    if gv_windows is not None and w_res is not None:
        raise NotImplementedError("genomic variance with weighted residuals (Random(d, v)): the tiles hold row-scaled values whose variance is "
                                  "not var(X beta) (ngp_enable_genomic_variance refuses it)")
    if not snps:
        storage = None   # (storage concerns panels only: a model without marker sets has none)
    if storage in ("u8", 1):  # codes stay codes: integer-valued float input is converted, anything else refused
        conv = []
        for M in mats:
            if not _is_bed(M) and M.dtype != np.uint8:
                if not (np.all(M == np.rint(M)) and M.min() >= 0 and M.max() <= 255):
                    raise ValueError('storage="u8" needs integer genotype codes in 0..255 in every SNP set')
                M = np.asfortranarray(M.astype(np.uint8))
            conv.append(M)
        mats = conv
        if pmats is not None:
            for i, M in enumerate(pmats):
                if not _is_bed(M) and M.dtype != np.uint8:
                    if not (np.all(M == np.rint(M)) and M.min() >= 0 and M.max() <= 255):
                        raise ValueError('storage="u8" needs integer genotype codes in 0..255 in every prediction source')
                    pmats[i] = np.asfortranarray(M.astype(np.uint8))
    if mats and not all(M.dtype == np.uint8 for M in mats if not _is_bed(M)):  # one byte per genotype only when every set comes that way
        mats = [M if _is_bed(M) else np.asarray(M, dtype=np.float64) for M in mats]
    if pmats is not None and not all(M.dtype == np.uint8 for M in pmats if not _is_bed(M)):
        pmats = [M if _is_bed(M) else np.asarray(M, dtype=np.float64) for M in pmats]
    # Correlated marker sets: a VCV key that is a TUPLE of set names (src/mme.jl:448-489) joins those sets into one unit whose loci
    # draw their k effects together (src/functions.jl:140-154).  On the device the k columns of a locus sit side by side, from a
    # 64-column boundary on (ngp_add_marker_set_tuple): the panel is assembled accordingly, everything else in formula order.
    by_name = {t.name: i for i, t in enumerate(snps)}
    tuples = [key for key in VCV if isinstance(key, tuple) and not (ped and key in ped["tuples"])]
    in_tuple = {}
    for key in tuples:
        if not all(nm in by_name for nm in key):
            raise ValueError(f"correlated marker sets {key}: every member needs its SNP(...) term")
        if len({mats[by_name[nm]].shape[1] for nm in key}) != 1:
            raise ValueError("correlated marker sets must have the same loci (src/mme.jl:453)")
        if len({snps[by_name[nm]].map for nm in key}) != 1:
            raise ValueError("correlated marker sets must have the same map file!")          # src/mme.jl:453
        if any(nm in summaryStat for nm in key):
            raise ValueError("Not available to use summary statistics in correlated effects")  # src/mme.jl:469
        for nm in key:
            in_tuple[nm] = key
    units, pieces, ncols = _panel_pieces(snps, mats, by_name, in_tuple)
    ppieces = _panel_pieces(snps, pmats, by_name, in_tuple)[1] if pmats is not None else None   # the same columns for the new individuals
    K = int(chains)
    if K < 1 or K > 8:
        raise ValueError("chains: 1..8")
    if K > 1 and samples == "text-sync":
        raise ValueError('chains > 1: samples "text", "binary" or "none"')
    skw = dict(mode=engine[0], lag=engine[1]) if engine else {}
    smp = Sampler(device=device, seed=seed, chain=chain, storage=storage, **skw)
    if w_res is not None:  # (the chains that share this panel take its weights with it)
        smp.set_residual_weights(w_res)
    if max_shards:  # an explicit shard count (ngp_set_max_shards): e.g. the layout of a fused run, to repeat one of its chains alone
        smp.set_max_shards(int(max_shards))
    elif K > 1:  # the layout with which K chains share one fused sweep launch (fp32 tiles), or the device side by side
        # (compact storage: the fused kernel serves two or three chains; more run side by side on disjoint CU shares)
        smp.set_max_shards(smp.shards_for_pass(K) if (storage is None or K <= 3) else smp.shards_for_chains(K))
    kinds = {np.asarray(pc).dtype == np.uint8 for pc in pieces if pc.shape[1] and not _is_bed(pc)}
    has_bed = any(_is_bed(pc) for pc in pieces)   # (a packed piece goes up in its own call beside pieces of any other kind)
    if not snps:   # GBLUP terms only: records, no genotype panel (ngp_set_records)
        smp.set_records(len(y))
    elif has_bed or (storage is None and kinds == {False}) or kinds == {True}:
        # the sets go to the device one after another (ngp_begin_panel / ngp_panel_columns_* / ngp_end_panel): no concatenated host copy
        smp.begin_panel(len(y), ncols)
        c0 = 0
        for pc in pieces:
            if _is_bed(pc):                      # packed .bed columns: decoded, gathered and imputed on the device
                pc.counts = smp.panel_columns_bed(c0, pc.info["bed"], pc.info["n"], rows=pc.rows, allele=pc.allele, missing=pc.missing, centre=True)
            elif pc.shape[1] and np.any(pc):     # (padding columns stay the zero columns they are born as)
                smp.panel_columns(c0, pc, centre=True)  # centring: src/prepMatVec.jl:129
            c0 += pc.shape[1]
        smp.end_panel()
    else:
        smp.set_panel(np.asfortranarray(np.concatenate(pieces, axis=1)), centre=True)  # centring: src/prepMatVec.jl:129
    if ppieces is not None:   # the prediction panel beside it, centred with the training means; the chains that share the panel see it
        smp.begin_prediction_panel(pmats[0].shape[0])
        c0 = 0
        for pc in ppieces:
            if _is_bed(pc):
                pc.counts = smp.prediction_columns_bed(c0, pc.info["bed"], pc.info["n"], rows=None, allele=pc.allele, missing=pc.missing, centre=True)
            elif pc.shape[1] and np.any(pc):
                smp.prediction_columns(c0, pc, centre=True)
            c0 += pc.shape[1]
        smp.end_prediction_panel()
    samplers = [smp]
    for c in range(1, K):  # the other chains share the first one's panel by reference (no copy, no second upload)
        sc = Sampler(device=device, seed=seed, chain=chain + c, storage=storage, **skw)
        sc.share_panel(smp)
        samplers.append(sc)
    region_cache = {}

    def regions_of(prior, P, map_path, name):
        if name not in region_cache:
            region_cache[name] = _regions_for(prior, P, map_path, outFolder, name)
        return region_cache[name]

    if masks is not None:   # every chain sets its own mask (a chain that shares the panel does not inherit one), in front of set_y
        for sc, rows in zip(samplers, masks):
            sc.set_holdout(rows)
    if liab is not None:    # behind the mask (held-out records carry no liability) and in front of set_y
        for sc in samplers:
            if liab["kind"] == "classes":
                sc.set_classes(np.maximum(liab["codes"], 1), liab["C"])   # (a record without a response is held out: its entry is not read)
                if thresholdStep == "cowles":
                    sc.set_threshold_step("cowles", 0.0)
                if classProb:
                    sc.enable_class_probabilities(True)
            else:
                sc.set_censored(liab["rows"], liab["lo"], liab["hi"])
    built = [_build_model(sc, VCV, summaryStat, parsed, userData, blockThese, intercept, units, snps, by_name, regions_of, y, nChain, nBurn, nThin,
                          gblup=gblup, k_owner=None if sc is samplers[0] else samplers[0], ped=ped, sparseFixed=sparseFixed)
             for sc in samplers]
    sets, fixed_names = built[0]
    randoms = samplers[0].randoms
    if gv_windows is not None:   # behind set_y: the pass is switched on with empty sums; one trace row per kept draw
        for sc in samplers:
            for st in sets:
                if gv_windows.get(st["name"]):
                    sc.set_variance_windows(st["id"], gv_windows[st["name"]])
            sc.enable_genomic_variance(True, float(windowThreshold), max(0, (int(nChain) - int(nBurn)) // int(nThin)))
    if diag_lags is not None:   # behind set_y, with an empty state; the halves of the split-R-hat part at the middle of the planned draws
        for sc in samplers:
            sc.enable_diagnostics(True, diag_lags, max(0, (int(nChain) - int(nBurn)) // int(nThin)) // 2)
    folders = [outFolder] if K == 1 else [os.path.join(outFolder, f"chain{chain + c}") for c in range(K)]
    for f in folders:
        os.makedirs(f, exist_ok=True)
    if liab is not None and liab["kind"] == "classes" and liab["C"] >= 3 and samples == "text":   # header row of thresholdOut
        for f in folders:
            _out(f, "threshold", [f"t{c}" for c in range(2, liab["C"])])
    res = _run_model(samplers, folders, sets, fixed_names, intercept, nChain, nBurn, nThin, samples, randoms)
    for nm, src in bed_sets.items():   # what the fileset held among the records: counted, never filtered
        st = snp_stats(src.info, src.counts)
        write_snp_stats(os.path.join(outFolder, f"snpStats{nm}.txt"), st)
        if nm in res["sets"]:
            res["sets"][nm]["snpStats"] = st
    if pmats is not None:
        if predict_ids is not None:
            ids = [str(a) for a in predict_ids]
        else:   # a candidate fileset names its own individuals
            ids = list(pmats[0].info["iid"]) if _is_bed(pmats[0]) else [str(i + 1) for i in range(pmats[0].shape[0])]
        sums = [sc.prediction_sums() for sc in samplers]
        names = [s["name"] for s in sets]
        for r, ps in zip(res.get("chains", []), sums):
            r["predict"] = _prediction_result(ps, ids, names)
        pooled = dict(sum=sum(ps["sum"] for ps in sums), sum2=sum(ps["sum2"] for ps in sums), nKept=sum(ps["nKept"] for ps in sums))
        res["predict"] = _prediction_result(pooled, ids, names)
        write_prediction_file(os.path.join(outFolder, "gebvPredict.txt"), res["predict"])
    if masks is not None:
        _holdout_results(res, samplers, masks, cv_fold, y, outFolder)
    if liab is not None and liab["kind"] == "classes":
        states = [sc.liability_state() for sc in samplers]
        for r, ls in zip(res.get("chains", []), states):
            r["thresholds"] = _threshold_summary(ls["sum_thr"], ls["sum_thr2"], r["nKept"])
        res["thresholds"] = _threshold_summary(sum(ls["sum_thr"] for ls in states), sum(ls["sum_thr2"] for ls in states), res["nKept"])
        res["classes"] = liab["values"]
        if thresholdStep == "cowles":
            steps = [sc.threshold_step() for sc in samplers]
            for r, ts in zip(res.get("chains", []), steps):
                r["thresholds"].update(acceptance=ts["accepted"] / max(ts["tries"], 1), sigma=ts["sigma"])
            res["thresholds"].update(acceptance=sum(ts["accepted"] for ts in steps) / max(sum(ts["tries"] for ts in steps), 1),
                                     sigma=float(np.mean([ts["sigma"] for ts in steps])))
        if classProb:
            _class_prob_results(res, samplers, masks, cv_fold, liab["codes"], liab["C"], outFolder)
    if gv_windows is not None:
        by_id = sorted(sets, key=lambda st: st["id"])                       # slot order: the device's set order
        names = [st["name"] for st in by_id]
        wins = [gv_windows.get(nm) or [] for nm in names]
        sums = []
        for sc, folder in zip(samplers, folders):
            gs = sc.genomic_variance_sums()
            V, r = sc.genomic_variance_trace()
            write_variance_out_files(folder, names, wins, V, r)
            sums.append(gs)
        for rr, gs in zip(res.get("chains", []), sums):
            rr["variance"] = _variance_result(gs, names, wins, float(windowThreshold))
        pooled = {k: sum(gs[k] for gs in sums) for k in ("sumV", "sumV2", "sumQ", "sumQ2", "count", "ratio", "nKept")}
        res["variance"] = _variance_result(pooled, names, wins, float(windowThreshold))
        write_gwas_files(outFolder, res["variance"])
    if diag_lags is not None:
        nthr = liab["C"] - 2 if liab is not None and liab["kind"] == "classes" and liab["C"] >= 3 else 0
        names = _diagnostics_names(samplers[0].diagnostics_layout()[0], sets, fixed_names, intercept, randoms, nthr)
        per_chain = []
        for sc in samplers:
            sc._diag_names = names
            per_chain.append(sc.diagnostics())
        if cv_fold is not None:   # the chains of folds=K see different data: nothing is pooled
            res["diagnostics"] = dict(names=names, chains=per_chain, pooled=False)
            for c, (d, f) in enumerate(zip(per_chain, folders)):
                write_convergence_file(os.path.join(f, "convergence.txt"), names, d)
        else:
            pooled = pool_diagnostics(per_chain)
            res["diagnostics"] = dict(names=names, chains=per_chain, worst=_worst(names, pooled), pooled=True, **pooled)
            write_convergence_file(os.path.join(outFolder, "convergence.txt"), names, pooled)
    return res


def _liability_spec(trait, censored, y, userData, VCV):
    """runLMEM(trait=..., censored=...): None, or {"kind": "classes", "codes", "C", "values"} / {"kind": "bounds", "rows", "lo", "hi", "y"}.
    Host checks only; a ValueError here comes before any device work."""
    from ._lib import censored_bounds, class_codes
    if trait not in ("gaussian", "categorical"):
        raise ValueError('trait: "gaussian" or "categorical"')
    if trait == "categorical":
        if censored is not None:
            raise ValueError('trait="categorical" together with censored=: a record is a class or a censored value, not both')
        e = VCV.get("e")
        if e is not None and not (np.ndim(e.v) == 0 and e.v == 1.0):
            raise ValueError('trait="categorical": the residual variance of the probit scale is 1; VCV["e"] must have the value 1 (or be left out)')
        codes, values = class_codes(y)
        return dict(kind="classes", codes=codes, C=len(values), values=values)
    if censored is None:
        return None
    if not isinstance(censored, dict) or set(censored) != {"lower", "upper"}:
        raise ValueError('censored: {"lower": column or array, "upper": column or array}')
    lower, upper = (np.asarray(userData[censored[k]] if isinstance(censored[k], str) else censored[k], dtype=np.float64) for k in ("lower", "upper"))
    if lower.shape != y.shape or upper.shape != y.shape:
        raise ValueError("censored: lower and upper have one entry per record")
    rows, lo, hi = censored_bounds(lower, upper)
    if len(rows) == 0:
        raise ValueError("censored: no record is censored (lower == upper everywhere)")
    ye = np.where(np.isnan(lower) | np.isinf(lower), upper, lower).astype(np.float64)   # exact records: lower == upper
    ye[rows] = 0.0                                                                     # (not read on the censored records)
    return dict(kind="bounds", rows=rows, lo=lo, hi=hi, y=ye)


def _ordered_options(trait, liab, thresholdStep, classProb, masks):
    """runLMEM(thresholdStep=..., classProb=...): host checks only; a ValueError here comes before any device work."""
    from ._lib import THRESHOLD_STEPS
    if thresholdStep not in THRESHOLD_STEPS:
        raise ValueError(f"thresholdStep: one of {sorted(THRESHOLD_STEPS)}")
    if classProb not in (True, False):
        raise ValueError("classProb: True or False")
    if trait != "categorical":
        if thresholdStep != "albert-chib":
            raise ValueError('thresholdStep: only a trait="categorical" model has thresholds')
        if classProb:
            raise ValueError('classProb: only a trait="categorical" model has classes')
        return
    if thresholdStep == "cowles" and liab["C"] < 3:
        raise ValueError('thresholdStep="cowles": two classes have no threshold to move (three classes or more)')
    if classProb and masks is None:
        raise ValueError('classProb: the probabilities are those of held-out records; give folds=, holdout= or missing="holdout"')


def _class_prob_results(res, samplers, masks, cv_fold, codes, C, outFolder):
    """res["holdout"]["prob"] / holdoutProb.txt (the records every chain holds out, sums pooled over the chains) and, for folds=K,
    res["cv"]["prob"], its scores and cvProb.txt (every record with a response, by the chain that held its fold out)."""
    from ._lib import class_metrics
    N = len(codes)
    hstates = [sc.holdout_state() for sc in samplers]
    sums = [sc.class_probability_sums() for sc in samplers]   # [C][m of the chain], rows in the order of the chain's mask

    def write(path, rows, fold, prob):
        with open(os.path.join(outFolder, path), "w") as f:
            f.write("record\tfold\tclass\t" + "\t".join(f"p{c}" for c in range(1, C + 1)) + "\n")
            for i, p in zip(rows, prob):
                f.write(f"{i + 1}\t{-1 if fold is None else fold[i]}\t{int(codes[i])}\t" + "\t".join(repr(float(v)) for v in p) + "\n")

    for r, hs, sp in zip(res.get("chains", []), hstates, sums):
        n = hs["n_fit"][hs["rows"]]
        r["holdout"]["prob"] = (sp[:, n > 0] / n[n > 0]).T
    if "holdout" in res:   # the rows every chain holds out: the chains' sums added, divided by the draws of all of them
        rows = res["holdout"]["rows"]
        tot = np.zeros((C, len(rows))); n = np.zeros(len(rows))
        for hs, sp in zip(hstates, sums):
            at = np.searchsorted(hs["rows"], rows)
            tot += sp[:, at]; n += hs["n_fit"][rows]
        res["holdout"]["prob"] = (tot / n).T
        write("holdoutProb.txt", rows, None, res["holdout"]["prob"])
    if cv_fold is None:
        return
    prob = np.full((N, C), np.nan)
    for c, (hs, sp) in enumerate(zip(hstates, sums)):
        own = np.flatnonzero(cv_fold == c)
        own = own[hs["n_fit"][own] > 0]
        prob[own] = (sp[:, np.searchsorted(hs["rows"], own)] / hs["n_fit"][own]).T
    val = np.flatnonzero((cv_fold >= 0) & ~np.isnan(prob[:, 0]))
    res["cv"]["prob"] = prob
    res["cv"].update({k: v for k, v in class_metrics(prob[val], codes[val]).items() if k != "n"})
    for pf in res["cv"]["per_fold"]:
        v = val[cv_fold[val] == pf["fold"]]
        pf.update({k: s for k, s in class_metrics(prob[v], codes[v]).items() if k != "n"})
    write("cvProb.txt", val, cv_fold, prob[val])


def _threshold_summary(sum_thr, sum_thr2, nKept):
    """Mean and SD of the thresholds t_2 .. t_{C-1} over the kept draws (t_1 = 0 is not listed)."""
    n = max(int(nKept), 1)
    mean = np.asarray(sum_thr)[1:] / n
    return dict(mean=mean, sd=np.sqrt(np.maximum(0.0, np.asarray(sum_thr2)[1:] / n - mean * mean)))


def _holdout_masks(y, holdout, missing, folds, foldSeed, chains):
    """runLMEM(holdout=..., missing=..., folds=..., foldSeed=...): (the held-out rows of every chain or None, the fold of every record or
    None, the number of chains).  Host checks only; a ValueError here comes before any device work."""
    from ._lib import deal_folds
    if missing not in ("error", "holdout"):
        raise ValueError('missing: "error" or "holdout"')
    N = len(y)
    if folds is not None:
        if int(chains) != 1:
            raise ValueError("folds= together with chains=: the K folds ARE the chains of the run")
        if holdout is not None:
            raise ValueError("folds= together with holdout=: every record with a response is held out by its fold's chain")
        if int(folds) != folds or not 2 <= int(folds) <= 8:
            raise ValueError("folds: 2..8")
    if holdout is None and missing == "error" and folds is None:
        return None, None, chains
    rows = np.zeros(0, dtype=np.int64)
    if holdout is not None:
        h = np.asarray(holdout)
        if h.ndim != 1 or len(h) == 0 or h.dtype.kind not in "iu":
            raise ValueError("holdout: a non-empty list of 0-based record numbers")
        rows = np.unique(h.astype(np.int64))
        if len(rows) != len(h):
            raise ValueError("holdout: a record is listed twice")
        if rows[0] < 0 or rows[-1] >= N:
            raise ValueError(f"holdout: records are numbered 0..{N - 1}")
    if missing == "holdout":
        rows = np.union1d(rows, np.flatnonzero(np.isnan(y))).astype(np.int64)
    if folds is None:
        if len(rows) >= N:
            raise ValueError("holdout: at least one record must keep its response")
        return ([rows] * int(chains) if len(rows) else None), None, chains
    fold = deal_folds(y, int(folds), foldSeed)
    return [np.union1d(rows, np.flatnonzero(fold == c)).astype(np.int64) for c in range(int(folds))], fold, int(folds)


def _holdout_results(res, samplers, masks, cv_fold, y, outFolder):
    """res["holdout"] / holdoutPredict.txt (the records every chain holds out, sums pooled over the chains) and, for folds=K,
    res["cv"] / cvPredict.txt (every record with a response, predicted by the chain that held its fold out)."""
    from ._lib import holdout_summary
    states = [sc.holdout_state() for sc in samplers]
    common = masks[0] if cv_fold is None else np.setdiff1d(masks[0], np.flatnonzero(cv_fold == 0))   # what EVERY chain holds out
    for r, hs in zip(res.get("chains", []), states):
        r["holdout"] = holdout_summary(hs)
    if len(common):
        keep = np.zeros(len(y)); keep[common] = 1.0   # (a fold-chain's own fold does not belong to what all chains hold out)
        hm = holdout_summary({k: sum(hs[k] for hs in states) * keep for k in ("sum_fit", "sum_fit2", "n_fit")})
        res["holdout"] = dict(rows=hm["rows"], y=y[hm["rows"]], yhat=hm["mean"], sd=hm["sd"], n=hm["n"])
        with open(os.path.join(outFolder, "holdoutPredict.txt"), "w") as f:
            f.write("record\ty\tyhat\tsd\n")
            for i, yh, sd in zip(hm["rows"], hm["mean"], hm["sd"]):
                f.write(f"{i + 1}\t{repr(float(y[i]))}\t{repr(float(yh))}\t{repr(float(sd))}\n")
    if cv_fold is None:
        return
    yhat = np.full(len(y), np.nan); sd = np.full(len(y), np.nan)
    for c, hs in enumerate(states):
        own = holdout_summary(hs)
        sel = np.isin(own["rows"], np.flatnonzero(cv_fold == c))
        yhat[own["rows"][sel]] = own["mean"][sel]; sd[own["rows"][sel]] = own["sd"][sel]

    def score(v):
        a, b = yhat[v], y[v]
        da, db = a - a.mean(), b - b.mean()
        saa = float(da @ da)
        return dict(n=int(len(v)), accuracy=float(da @ db / np.sqrt(saa * float(db @ db))) if saa > 0 and db @ db > 0 else float("nan"),
                    slope=float(da @ db / saa) if saa > 0 else float("nan"), mse=float(np.mean((b - a) ** 2)))

    allv = score(np.flatnonzero(cv_fold >= 0))
    res["cv"] = dict(fold=cv_fold, yhat=yhat, sd=sd, accuracy=allv["accuracy"], slope=allv["slope"], mse=allv["mse"],
                     per_fold=[dict(fold=c, **score(np.flatnonzero(cv_fold == c))) for c in range(len(states))], pooled_over_folds=True)
    with open(os.path.join(outFolder, "cvPredict.txt"), "w") as f:
        f.write("record\tfold\ty\tyhat\tsd\n")
        for i in np.flatnonzero(cv_fold >= 0):
            f.write(f"{i + 1}\t{cv_fold[i]}\t{repr(float(y[i]))}\t{repr(float(yhat[i]))}\t{repr(float(sd[i]))}\n")


def _variance_windows(windows, threshold, genomic_variance, snps, mats, gb_names, VCV):
    """runLMEM(windows=..., windowThreshold=..., genomicVariance=...): {set name: [(a, b), ...]} with 0-based half-open column ranges
    of the set, or None when the pass is off.  Host checks only; a ValueError here comes before any device work."""
    if windows is None and not genomic_variance:
        return None
    windows = {} if windows is None else windows
    if not hasattr(windows, "keys"):
        raise ValueError("windows: a mapping from the name of a SNP(...) term to a window size or a list of (start, stop) column ranges")
    thr = float(threshold)
    if not (0.0 <= thr <= 1.0):
        raise ValueError(f"windowThreshold is a share of the genomic variance, in [0, 1]: got {threshold}")
    if not snps:
        raise ValueError("genomic variance needs at least one SNP(...) marker set")
    ncol = {t.name: M.shape[1] for t, M in zip(snps, mats)}
    in_tuple = {nm for key in VCV if isinstance(key, tuple) for nm in key}
    out = {}
    for name, spec in windows.items():
        if name in gb_names:
            raise ValueError(f"windows[{name!r}]: a GBLUP term has no marker effects whose variance a window could carry")
        if name not in ncol:
            raise ValueError(f"windows for an unknown set {name!r}: the SNP(...) marker sets are {sorted(ncol)}")
        if name in in_tuple:
            raise NotImplementedError(f"windows[{name!r}]: a member of a correlated (Tuple) unit shares its loci's columns with the other members")
        P = ncol[name]
        if isinstance(spec, (int, np.integer)) and not isinstance(spec, bool):
            W = int(spec)
            if W < 1:
                raise ValueError(f"windows[{name!r}]: a window size of at least one SNP, got {W}")
            t = [t for t in snps if t.name == name][0]
            if t.map:   # windows inside each chromosome, as the variance regions of BayesPR are cut (src/misc.jl:163-215)
                w = prep2RegionData(None, name, t.map, W)
                if not w or w[-1][1] != P:
                    raise ValueError(f"windows[{name!r}]: the map file {t.map} lists {w[-1][1] if w else 0} SNPs, the set holds {P}")
            else:
                w = [(a, min(a + W, P)) for a in range(0, P, W)]
        else:
            try:
                w = [(int(a), int(b)) for a, b in spec]
            except (TypeError, ValueError):
                raise ValueError(f"windows[{name!r}]: a window size or a list of (start, stop) column ranges") from None
            at = 0
            for k, (a, b) in enumerate(w):
                if a < at or b <= a or b > P:
                    raise ValueError(f"windows[{name!r}] must be ascending, disjoint, non-empty and inside the set's {P} columns (window {k}: {(a, b)})")
                at = b
        out[name] = w
    return out


def _variance_result(gs, names, wins, threshold):
    """res["variance"] from genomic-variance sums (one chain's, or several chains' added up)."""
    from ._lib import genomic_variance_summary
    sm = genomic_variance_summary(gs)
    nw = sum(len(w) for w in wins)
    out = dict(nKept=sm["nKept"], threshold=threshold, ratio=dict(mean=sm["ratio"][0], sd=sm["ratio"][1]),
               total=dict(meanV=float(sm["meanV"][-1]), sdV=float(sm["sdV"][-1])), sets={})
    o = 0
    for k, (nm, w) in enumerate(zip(names, wins)):
        sl = slice(o, o + len(w))
        out["sets"][nm] = dict(meanV=float(sm["meanV"][nw + k]), sdV=float(sm["sdV"][nw + k]), meanQ=float(sm["meanQ"][nw + k]), sdQ=float(sm["sdQ"][nw + k]),
                               windows=dict(first=np.array([a + 1 for a, _ in w], dtype=np.int64), last=np.array([b for _, b in w], dtype=np.int64),
                                            meanV=sm["meanV"][sl], sdV=sm["sdV"][sl], meanQ=sm["meanQ"][sl], sdQ=sm["sdQ"][sl], wppa=sm["wppa"][sl]))
        o += len(w)
    return out


def write_variance_out_files(folder, names, wins, V, r):
    """The per-draw trace in the reference's *Out format (a header row, then one tab-separated row per kept draw): windowVar<set>Out with
    the columns win_1 ... for every set that has windows, and genVarOut with one column per set, then total, then ratio."""
    nw = sum(len(w) for w in wins)
    o = 0
    for nm, w in zip(names, wins):
        if w:
            with open(os.path.join(folder, f"windowVar{nm}Out"), "w") as f:
                f.write("\t".join(f"win_{k + 1}" for k in range(len(w))) + "\n")
                for row in V:
                    f.write("\t".join(_fmt(row[o:o + len(w)])) + "\n")
        o += len(w)
    with open(os.path.join(folder, "genVarOut"), "w") as f:
        f.write("\t".join(list(names) + ["total", "ratio"]) + "\n")
        for row, rr in zip(V, r):
            f.write("\t".join(_fmt(row[nw:]) + _fmt(rr)) + "\n")


def write_gwas_files(folder, variance):
    """gwas<set>.txt for every set with windows: window, first and last SNP (1-based, inside the set), mean V, mean q, SD of q, WPPA."""
    for nm, st in variance["sets"].items():
        w = st["windows"]
        if len(w["first"]) == 0:
            continue
        with open(os.path.join(folder, f"gwas{nm}.txt"), "w") as f:
            f.write("window\tfirstSNP\tlastSNP\tmeanV\tmeanQ\tsdQ\tWPPA\n")
            for k in range(len(w["first"])):
                f.write("\t".join([str(k + 1), str(int(w["first"][k])), str(int(w["last"][k]))] + _fmt([w["meanV"][k], w["meanQ"][k], w["sdQ"][k], w["wppa"][k]])) + "\n")


def _panel_pieces(snps, mats, by_name, in_tuple):
    """The column pieces of ONE panel from the matrices of the SNP terms (the rows may be the records' or new individuals'): a set
    takes the next columns; the members of a correlated (Tuple) unit are interleaved from a 64-column boundary on and own their blocks
    to the end of the last one.  Returns (units, pieces, ncols); units: ("set", name, col0, P) | ("tuple", key, col0, nloc), in formula
    order of their first member."""
    units, pieces, ncols = [], [], 0
    nrows = mats[0].shape[0] if mats else 0
    done_t = set()
    for t in snps:
        if t.name in in_tuple:
            key = in_tuple[t.name]
            if key in done_t:
                continue
            done_t.add(key)
            pad = (-ncols) % 64
            if pad:
                pieces.append(np.zeros((nrows, pad), dtype=mats[0].dtype)); ncols += pad
            blk = tuple_panel([np.asfortranarray(mats[by_name[nm]]) for nm in key])
            nloc = mats[by_name[key[0]]].shape[1]
            units.append(("tuple", key, ncols, nloc))
            pieces.append(blk); ncols += blk.shape[1]
            pad = (-ncols) % 64                  # the set owns its blocks to the end of the last one
            if pad:
                pieces.append(np.zeros((nrows, pad), dtype=mats[0].dtype)); ncols += pad
        else:
            units.append(("set", t.name, ncols, mats[by_name[t.name]].shape[1]))
            pieces.append(mats[by_name[t.name]]); ncols += mats[by_name[t.name]].shape[1]
    return units, pieces, ncols


def _genotype_source(path, ids, allele, missing):
    """The genotypes of one SNP(...) term: a PLINK fileset stays packed (_BedSource; ids: the records' IIDs, or None for file order),
    everything else is read into a host matrix (read_genotypes)."""
    if isinstance(path, (str, os.PathLike)) and not str(path).endswith(".npy") and is_bed_file(path):
        info = read_plink(path)
        return _BedSource(info, None if ids is None else _bed_rows(info, ids), allele, missing)
    return read_genotypes(path)


def _prediction_sources(predict, predict_ids, snps, mats, gb_names, allele=1, missing="mean", tuple_names=()):
    """runLMEM(predict=...): the genotype matrices of the new individuals, one per marker-set term in the order of `snps`, or None
    without predict=.  Host checks only; a ValueError here comes before any device work."""
    if predict is None:
        if predict_ids is not None:
            raise ValueError("predict_ids without predict=")
        return None
    if gb_names:
        raise NotImplementedError(f"predict= with the GBLUP term(s) {sorted(gb_names)}: a breeding value of a new individual under GBLUP needs its "
                                  "relationships to the records (makeG over both, src/misc.jl:145-160); prediction on the device covers marker sets")
    if not hasattr(predict, "keys"):
        raise ValueError("predict: a mapping from the name of every SNP(...) term to its genotype source")
    want = [t.name for t in snps]
    if sorted(predict.keys()) != sorted(want):
        raise ValueError(f"predict needs exactly one source per SNP(...) term {want}, got {sorted(predict.keys())}")
    pm = [_genotype_source(predict[nm], None, allele, missing) for nm in want]
    for nm, M, T in zip(want, pm, mats):
        if _is_bed(M) and _is_bed(T) and M.info["snp"] != T.info["snp"]:
            raise ValueError(f"predict[{nm!r}]: the SNP IDs of {M.info['path'][:-4]}.bim differ from the training set's ({T.info['path'][:-4]}.bim)")
        if M.ndim != 2 or M.shape[1] != T.shape[1]:
            raise ValueError(f"predict[{nm!r}] holds {M.shape[1] if M.ndim == 2 else '?'} columns, the term {T.shape[1]}")
    if len({M.shape[0] for M in pm}) != 1 or pm[0].shape[0] < 1:
        raise ValueError(f"every prediction source needs the same individuals: rows {[M.shape[0] for M in pm]}")
    if predict_ids is not None and len(predict_ids) != pm[0].shape[0]:
        raise ValueError(f"predict_ids names {len(predict_ids)} individuals, the prediction sources hold {pm[0].shape[0]}")
    for i, nm in enumerate(want):   # members of a correlated unit are interleaved on the host
        if _is_bed(pm[i]) and nm in tuple_names:
            src = pm[i]
            pm[i] = src.decode()
            if src.counts[:, 3].any():
                raise NotImplementedError(f"predict[{nm!r}]: missing calls of candidates in a correlated (Tuple) unit -- the host decoder knows "
                                          "the candidates' column means, not the training means a missing call takes; impute them first")
    return pm


def _prediction_result(ps, ids, names):
    from ._lib import prediction_summary
    pr = prediction_summary(ps)
    return dict(ids=list(ids), nKept=pr["nKept"], mean=pr["mean"], sd=pr["sd"], sets={nm: pr["sets"][k] for k, nm in enumerate(names)})


def write_prediction_file(path, pred):
    """gebvPredict.txt: one row per predicted individual, tab-separated: ID mean sd mean_<set> sd_<set> ... (values with the digits
    that read back to the same Float64)."""
    with open(path, "w") as f:
        f.write("\t".join(["ID", "mean", "sd"] + [f"{c}_{nm}" for nm in pred["sets"] for c in ("mean", "sd")]) + "\n")
        for i, a in enumerate(pred["ids"]):
            row = [pred["mean"][i], pred["sd"][i]] + [pred["sets"][nm][c][i] for nm in pred["sets"] for c in ("mean", "sd")]
            f.write("\t".join([str(a)] + [repr(float(v)) for v in row]) + "\n")


def read_prediction_file(path):
    """gebvPredict.txt back as {"ids", "mean", "sd", "sets": {name: {"mean", "sd"}}}."""
    with open(path) as f:
        head = f.readline().rstrip("\n").split("\t")
        rows = [ln.rstrip("\n").split("\t") for ln in f if ln.strip()]
    cols = {h: np.array([float(r[k]) for r in rows]) for k, h in enumerate(head) if k > 0}
    names = [h[len("mean_"):] for h in head[3:] if h.startswith("mean_")]
    return dict(ids=[r[0] for r in rows], mean=cols["mean"], sd=cols["sd"], sets={nm: dict(mean=cols[f"mean_{nm}"], sd=cols[f"sd_{nm}"]) for nm in names})


def _random_tuples(VCV, parsed, summaryStat):
    """The VCV keys that are tuples of PED(col) terms, e.g. ("ID", "Dam"): correlated random effects over one pedigree with a k x k
    covariance (src/mme.jl:207-239), checked.  Tuples of SNP terms are correlated MARKER sets and are not listed here."""
    out = []
    for key in VCV:
        if not isinstance(key, tuple) or not any(m in parsed.ped for m in key):
            continue
        if any(m in {t.name for t in parsed[2]} for m in key):   # (a SNP term among the members: gblup_terms / the marker tuples refuse it)
            continue
        for m in key:
            if m in parsed.random or str(m).replace(" ", "").strip("()").startswith("1|"):
                raise NotImplementedError(f"VCV key {key}: a (1|g) term inside a correlated (Tuple) random effect; the reference accepts Symbols only "
                                          "(isa(zSet, Tuple{Vararg{Symbol}}), src/mme.jl:207): write the member as PED(col)")
            if m not in parsed.ped:
                raise ValueError(f"correlated random effects {key}: every member needs its PED(...) term")
        k = len(key)
        if not 2 <= k <= 4 or len(set(key)) != k:
            raise ValueError(f"correlated random effects {key}: 2..4 different PED terms")
        if key in summaryStat or any(m in summaryStat for m in key):
            raise ValueError("Not available to use summary statistics in correlated effects")   # src/mme.jl:233-235
        prior = VCV[key]
        if not isinstance(prior, RandomEffectType) or np.shape(prior.v) != (k, k):
            raise ValueError(f"prior of {key}: Random(\"A\", V) with V the {k} x {k} covariance matrix")
        if not (prior.str is None or (isinstance(prior.str, str) and prior.str in ("A", "I", ""))):
            raise NotImplementedError(f"correlated random effects {key} with structure {prior.str!r}: \"A\" (the pedigree's) or \"I\" (src/mme.jl:28-33)")
        for m in key:
            if m in VCV:
                raise ValueError(f"PED({m}) has a prior of its own and is a member of {key}: one or the other")
        out.append(key)
    if len({m for key in out for m in key}) != sum(len(key) for key in out):
        raise ValueError("a PED term may be a member of one correlated (Tuple) random effect only")
    return out


def _residual_weights(e_prior, N):
    """Residual structure of Random(str, v) under key "e" (src/mme.jl:63-79): None for "I" (or empty), else the weights
    w = 1 ./ d of a "D" structure given as the length-N vector d (E.iVarStr = inv.(str), the same IEEE division)."""
    st = e_prior.str
    if st is None or (isinstance(st, str) and st in ("I", "")):
        return None
    if isinstance(st, str) or np.ndim(st) != 1:
        raise NotImplementedError(f"residual structure {st!r}: only \"I\" and a vector \"D\" (d_ii per record) exist (src/mme.jl:63-79)")
    d = np.asarray(st, dtype=np.float64)
    if len(d) == 0:
        return None
    if len(d) != N:
        raise ValueError(f"residual structure D: {len(d)} entries for {N} records")
    if not np.all(np.isfinite(d)) or np.any(d <= 0.0):
        raise ValueError("residual structure D: every d_ii must be finite and > 0")
    return 1.0 / d


def _build_model(smp, VCV, summaryStat, parsed, userData, blockThese, intercept, units, snps, by_name, regions_of, y, nChain, nBurn, nThin,
                 gblup=None, k_owner=None, ped=None, sparseFixed="auto"):
    """Priors, fixed-effect sets, random-effect sets, marker sets, y and the schedule of ONE chain's handle (its panel is set); returns
    (sets, fixed_names).  gblup: {term name: dict(M, prior)} of the GBLUP terms; k_owner: the chain whose dense K this one shares;
    ped: dict(table, Ainv) of makePed when the model has userPedData."""
    # residual prior (src/mme.jl:63-94)
    e_prior = VCV.get("e", Random("I", 100.0))  # (a "D" structure's weights were set on the handle before its panel: runLMEM)
    e_df = 4.0
    e_scale = 0.0005 if e_prior.v == 0.0 else e_prior.v * (e_df - 2.0) / e_df
    smp.set_residual_prior(e_df, e_scale)
    smp.set_intercept(intercept)
    # fixed effects beyond the intercept (src/prepMatVec.jl:150-165, blocks src/mme.jl:96-108): every term its own set, the terms of a
    # blockThese group one multi-column set (sampleb!, src/functions.jl:22-36); blocks first, in the user's order, then the rest in
    # model order (the reference walks a Julia Dict, whose order is not defined: documented difference)
    covs = list(parsed.covariates)
    fixed_names = ["(Intercept)"] if intercept else []
    # a unit goes to the device as a sparse set (ngp_add_fixed_set_sparse: the same chain, bit for bit) when it has more than 64 design
    # columns (sparseFixed="auto"), or whenever it has several (True); never with False.  No dense design is built for such a unit.
    def as_sparse(cols):
        w = _fixed_unit_width(cols, userData)
        return w >= 2 and (sparseFixed is True or (sparseFixed == "auto" and w > 64))
    used = set()
    for blk in (blockThese or []):
        blk = [c for c in covs if c in set(blk)]          # columns inside a block keep the model's order
        if not blk:
            continue
        if as_sparse(blk):
            fixed_names += _add_fixed_unit_sparse(smp, blk, userData)
        else:
            designs = [design_columns(c, userData[c]) for c in blk]
            smp.add_fixed_set(np.column_stack([d[0] for d in designs]))
            for d in designs:
                fixed_names += d[1]
        used.update(blk)
    for c in covs:
        if c in used:
            continue
        if as_sparse([c]):
            fixed_names += _add_fixed_unit_sparse(smp, [c], userData)
            continue
        Xc, names = design_columns(c, userData[c])
        if c in summaryStat and Xc.shape[1] == 1:         # src/mme.jl:140-147
            m, vv = float(np.atleast_1d(summaryStat[c][0])[0]), float(np.atleast_1d(summaryStat[c][1])[0])
            smp.add_fixed_set(Xc, lhs0=[1.0 / vv], rhs0=[m / vv])
        else:
            smp.add_fixed_set(Xc)
        fixed_names += names
    # (1|g) random-effect sets, after the fixed effects, in formula order (src/samplers.jl:43-46; set-up src/mme.jl:165-272)
    # A GBLUP term is a random-effect set too (Z = I over K = inv(G), src/prepMatVec.jl:122-126) and takes its place among them in
    # formula order (the reference walks keys(Z) of a Dict, whose order is not defined: the documented difference of the fixed-effect sets)
    smp.randoms = []
    gblup = gblup or {}
    for kind, g in (parsed.order or [("1|", g) for g in parsed.random]):
        if kind == "snp":
            if g not in gblup:
                continue
            prior, N = gblup[g]["prior"], len(y)
            rdf = 3.0 + 1.0                                          # src/mme.jl:261
            v = float(prior.v)
            if k_owner is None:   # G on the matrix cores, inverted on the device, handed to the set without a copy
                _grm_build(smp, gblup[g]["M"], prior.type)
                smp.grm_invert()
                Ksrc = None
            else:                 # the other chains read the first chain's matrix
                Ksrc = (k_owner, [rd["id"] for rd in k_owner.randoms if rd.get("key") == g][0])
            rid = smp.add_random_set_dense(None, N, K=Ksrc, df=rdf, scale=v * (rdf - 2.0) / rdf, varU0=v)   # src/mme.jl:265-272
            smp.randoms.append(dict(id=rid, g=g, key=g, levels=[f"Ind{i + 1}" for i in range(N)], q=N, files=(f"u{g}", f"varU{g}", g)))
            continue
        if kind == "ped" and any(g in key for key in ped["tuples"]):
            # a correlated (Tuple) set, (ID, Dam): k PED terms over one K with a k x k covariance (src/mme.jl:207-239), placed where
            # its first member stands in the formula.  The device draws the exact Gibbs conditional, not the reference's lines
            # (include/nextgp_hip.h, ngp_add_random_set_tuple).
            key = [key for key in ped["tuples"] if g in key][0]
            if g != [m for _, m in (parsed.order or []) if m in key][0]:
                continue
            table, prior, k = ped["table"], VCV[key], len(key)
            levels = np.array([[table["pos"][str(a)] if str(a) != "0" else -1 for a in np.asarray(userData[m]).tolist()] for m in key], dtype=np.int32)
            K = ped["Ainv"] if isinstance(prior.str, str) and prior.str == "A" else None
            rdf = 3.0 + k                                            # src/mme.jl:265
            V = np.asarray(prior.v, dtype=np.float64)
            n = len(table["origID"])
            rid = smp.add_random_set_tuple(levels, n, K=K, df=rdf, scale=V * (rdf - k - 1.0), varU0=V)   # src/mme.jl:271
            smp.randoms.append(dict(id=rid, g=key[0], key=key, members=list(key), levels=list(table["origID"]), q=n))
            continue
        if kind == "ped":   # PED(col): every animal of the pedigree is a level, K = A^-1 (src/prepMatVec.jl:136-153, src/mme.jl:26-46)
            table = ped["table"]
            level = np.array([table["pos"][str(a)] for a in np.asarray(userData[g]).tolist()], dtype=np.int32)
            prior = VCV.get(g)
            if prior is None:
                prior = Random("I", 100.0)                           # src/mme.jl:40-44: the identity over the pedigree's levels
            if not isinstance(prior, RandomEffectType):
                raise ValueError(f"prior of PED({g}): Random(\"A\", v)")
            if g in ped.get("single", {}):   # Random("H", v): single-step GBLUP, the hybrid engine over A^-1 and the genotyped corner
                ss = ped["single"][g]
                rdf = 3.0 + 1.0                                      # src/mme.jl:261
                v = float(prior.v)
                n = len(table["origID"])
                if k_owner is None:   # G on the matrix cores, the corner block on the device, handed to the set without a copy
                    _grm_build(smp, ss["M"], prior.type)
                    smp.grm_single_step(ss["A22"], ss["w"])
                    Dsrc = None
                else:                 # the other chains read the first chain's block
                    Dsrc = (k_owner, [rd["id"] for rd in k_owner.randoms if rd.get("key") == g][0])
                rid = smp.add_random_set_hybrid(ss["inv"][level].astype(np.int32), n, ss["S"], ss["ng"], D=Dsrc, df=rdf, scale=v * (rdf - 2.0) / rdf,
                                                varU0=v)
                smp.randoms.append(dict(id=rid, g=g, key=g, levels=list(ss["levels"]), q=n, files=(f"u{g}", f"varU{g}", g)))
                continue
            if isinstance(prior.str, str) and prior.str == "A":
                K = ped["Ainv"]
            elif prior.str is None or (isinstance(prior.str, str) and prior.str in ("I", "")):
                K = None
            else:
                raise NotImplementedError(f"PED({g}) with structure {prior.str!r}: \"A\" (the pedigree's) or \"I\" (src/mme.jl:28-33)")
            rdf = 3.0 + 1.0                                          # src/mme.jl:261
            v = float(prior.v)
            n = len(table["origID"])
            rid = smp.add_random_set(level, n, K=K, df=rdf, scale=v * (rdf - 2.0) / rdf, varU0=v)   # src/mme.jl:265-272
            smp.randoms.append(dict(id=rid, g=g, key=g, levels=list(table["origID"]), q=n, files=(f"u{g}", f"varU{g}", g)))
            continue
        pr = VCV.get(f"1|{g}", VCV.get(f"(1|{g})"))
        if ped is None and isinstance(pr, RandomEffectType) and isinstance(pr.str, str) and pr.str == "A":
            raise ValueError(f"(1|{g}) with Random(\"A\", v) needs a pedigree: pass userPedData (and write the term as PED({g}))")
        level, names = random_levels(userData[g])
        K, rdf, rscale, v = random_prior(VCV, g, len(names))
        rid = smp.add_random_set(level, len(names), K=K, df=rdf, scale=rscale, varU0=v)
        smp.randoms.append(dict(id=rid, g=g, levels=names, q=len(names)))
    # marker sets (src/mme.jl:287-347, 492-520; correlated sets :448-489)
    sets = []
    for unit in units:
        if unit[0] == "tuple":
            _, key, col0, nloc = unit
            prior = VCV[key]
            k = len(key)
            if not isinstance(prior, BayesPRType) or np.shape(prior.v) != (k, k):
                raise NotImplementedError(f"correlated marker sets {key}: BayesPR(r, v) with v the {k} x {k} covariance matrix (src/mme.jl:448-489)")
            df = 3.0 + k                                                   # src/mme.jl:493
            vm = np.asarray(prior.v, dtype=np.float64)
            scale = vm * (df - k - 1.0) if k > 1 else vm * (df - 2.0) / df  # src/mme.jl:501
            t0 = snps[by_name[key[0]]]
            regions = regions_of(prior, nloc, t0.map, "_".join(key))
            sid = smp.add_marker_set_tuple(col0, nloc, k, df, scale, regions, vm)
            smp.set_chain_form(1)   # a model with correlated sets: block chains in the inverse form (its Tuple blocks 3.8 -> 3.0 us)
            cols = tuple_columns(col0, nloc, k)
            sets.append(dict(id=sid, name="_".join(key), members=list(key), cols=cols, P=nloc, prior=prior, nreg=len(regions), nvb=len(regions) * k * k, k=k))
            continue
        _, name, col0, P = unit
        t = snps[by_name[name]]
        prior = VCV.get(t.name)
        if prior is None:  # src/mme.jl:324-329, 504, 518
            prior = BayesPR(9999, 0.05)
        if not isinstance(prior, (BayesPRType, BayesBType, BayesCType, BayesRType, BayesRCType, BayesLogVarType)):
            raise NotImplementedError(f"prior {type(prior).__name__} for {t.name}: only BayesPR, BayesB, BayesC, BayesR, BayesRCπ and BayesLV are on the accelerated path")
        df = 4.0                                  # 3 + size(v,1), src/mme.jl:493
        scale = prior.v * (df - 2.0) / df         # src/mme.jl:501
        regions = regions_of(prior, P, t.map, t.name)
        lhs0 = rhs0 = None
        if t.name in summaryStat:                 # src/mme.jl:316-322
            m, v = np.asarray(summaryStat[t.name][0], float), np.asarray(summaryStat[t.name][1], float)
            lhs0 = np.where(np.isinf(1.0 / v), 0.0, 1.0 / v)
            rhs0 = np.nan_to_num(lhs0 * m)
        if isinstance(prior, BayesBType):
            sid = smp.add_marker_set(col0, P, METHOD_BAYESB, df, scale, regions, [prior.v] * P, pi0=prior.pi, estPi=prior.estimatePi,
                                     lhs0=lhs0, rhs0=rhs0)
        elif isinstance(prior, BayesCType):
            sid = smp.add_marker_set(col0, P, METHOD_BAYESC, df, scale, regions, [prior.v], pi0=prior.pi, estPi=prior.estimatePi,
                                     lhs0=lhs0, rhs0=rhs0)
        elif isinstance(prior, BayesLogVarType):  # src/mme.jl:418-439
            Cm, cnames = lv_design_matrix(prior.f, prior.covariates)
            if Cm.shape[0] != P:
                raise ValueError(f"BayesLV prior of {t.name}: {Cm.shape[0]} covariate rows for {P} SNPs")
            est = prior.estimateVarZeta
            sid = smp.add_marker_set_lv(col0, P, prior.v, Cm, prior.varZeta, est_mode=0 if est is False else 1 if est is True else 2,
                                        est_fraction=float(est) if isinstance(est, float) else 0.0, lhs0=lhs0, rhs0=rhs0)
            n_lv = sum(1 for q in sets if "lv" in q)
            sets.append(dict(id=sid, name=t.name, members=[t.name], cols=np.arange(col0, col0 + P)[:, None], P=P, prior=prior, nreg=P, nvb=P, k=1,
                             lv=n_lv, ncov=Cm.shape[1], cnames=cnames))
            continue
        elif isinstance(prior, BayesRCType):  # src/mme.jl:384-403
            if prior.annot.shape[0] != P:
                raise ValueError(f"BayesRCπ prior of {t.name}: {prior.annot.shape[0]} annotation rows for {P} SNPs")
            A = prior.annot.shape[1]
            sid = smp.add_marker_set_rc(col0, P, df, scale, prior.v, prior.class_, prior.pi, prior.annot, estPi=prior.estimatePi, lhs0=lhs0, rhs0=rhs0)
            sets.append(dict(id=sid, name=t.name, members=[t.name], cols=np.arange(col0, col0 + P)[:, None], P=P, prior=prior, nreg=A, nvb=A, k=1, A=A))
            continue
        elif isinstance(prior, BayesRType):  # src/mme.jl:374-383
            sid = smp.add_marker_set_r(col0, P, df, scale, prior.v, prior.class_, prior.pi, estPi=prior.estimatePi, lhs0=lhs0, rhs0=rhs0)
        else:
            sid = smp.add_marker_set(col0, P, METHOD_BAYESPR, df, scale, regions, [prior.v] * len(regions), lhs0=lhs0, rhs0=rhs0)
        sets.append(dict(id=sid, name=t.name, members=[t.name], cols=np.arange(col0, col0 + P)[:, None], P=P, prior=prior, nreg=len(regions),
                         nvb=P if isinstance(prior, BayesBType) else len(regions), k=1))
    smp.set_y(y)
    smp.set_schedule(nChain, nBurn, nThin)
    return sets, fixed_names


def _run_model(samplers, folders, sets, fixed_names, intercept, nChain, nBurn, nThin, samples, randoms=()):
    """Header rows, the chain(s), the *Out rows and the posterior means (pooled over the chains when there are several)."""
    if samples not in ("text", "text-sync", "binary", "none"):
        raise ValueError('samples: "text", "text-sync", "binary" or "none"')
    if len(samplers) > 1:
        paths = [os.path.join(f, "samples.ngpsmp") for f in folders]
        for sc, f, pth in zip(samplers, folders, paths):
            if samples == "text":
                _write_headers(f, sets, fixed_names, randoms)
            if samples in ("text", "binary"):
                sc.set_sample_file(pth)
        samplers[0].get_timing()
        Sampler.run_many(samplers, nChain)  # ONE fused sweep launch per iteration for all chains where the engine serves it
        fused = samplers[0].get_timing()["sweep_launches"] == nChain
        if not fused and sets:  # (a model without marker sets sweeps nothing; the layout was chosen for a fused launch: side by side each chain's grid takes most of the device, so they take turns)
            import warnings
            warnings.warn(f"runLMEM(chains={len(samplers)}): this layout / engine is not served by the fused sweep kernel (fp32 tiles: shards of at most "
                          "64 rows with lag 6 or 8, or two chains on 64-224-row shards with lag 4-6; compact storage: two or three chains); the chains "
                          "ran one launch each per iteration. Results are the same; pass max_shards=Sampler.shards_for_chains(K) for side-by-side runs.")
        results = []
        for sc, f, pth in zip(samplers, folders, paths):
            if samples in ("text", "binary"):
                sc.set_sample_file(None)
            if samples == "text":
                samples_to_out_files(pth, f, sets, intercept, len(fixed_names) > int(intercept), randoms)
                os.remove(pth)
            results.append(_posterior_means(sc, sets, fixed_names, intercept, randoms))
        pooled = _pool_results(results)
        pooled["fused"] = bool(fused)
        return pooled
    smp, outFolder = samplers[0], folders[0]
    # header rows (src/mme.jl:543-595)
    if samples in ("text", "text-sync"):
        _write_headers(outFolder, sets, fixed_names, randoms)
    return _run_one(smp, outFolder, sets, fixed_names, intercept, nChain, nBurn, nThin, samples, randoms)


def _write_headers(outFolder, sets, fixed_names, randoms=()):
    """Header rows of the *Out files (src/mme.jl:543-595)."""
    _out(outFolder, "b", fixed_names)
    _out(outFolder, "varE", ["e"])
    for rd in randoms:   # src/mme.jl:548-563; the u header lists the levels in the order of u (random_levels)
        for name, fields in _rd_headers(rd):
            _out(outFolder, name, fields)
    for s in sets:
        names = [f"M{i + 1}" for i in range(s["P"])]  # src/prepMatVec.jl:131
        for nm in s["members"]:
            _out(outFolder, f"beta{nm}", names)
            _out(outFolder, f"delta{nm}", names)
        if isinstance(s["prior"], (BayesBType, BayesCType)):  # src/samplers.jl:80-82
            _out(outFolder, f"pi{s['name']}", ["pi1", "pi2"])
        if isinstance(s["prior"], BayesRType):               # one column per class (src/mme.jl:589-591)
            _out(outFolder, f"pi{s['name']}", [f"pi{v + 1}" for v in range(len(s["prior"].pi))])
        if isinstance(s["prior"], BayesRCType):              # annotation-major, and the category of every SNP (src/mme.jl:573-576)
            _out(outFolder, f"pi{s['name']}", [f"pi{v + 1}" for v in range(len(s["prior"].pi) * s["A"])])
            _out(outFolder, f"annot{s['name']}", names)
        if isinstance(s["prior"], BayesLogVarType):          # src/mme.jl:577-580
            _out(outFolder, f"c{s['name']}", [f"c{v + 1}" for v in range(s["ncov"])])
            _out(outFolder, f"varZeta{s['name']}", ["varZeta"])
        _out(outFolder, f"var{s['name']}", _var_names(s))


def _run_one(smp, outFolder, sets, fixed_names, intercept, nChain, nBurn, nThin, samples, randoms=()):
    # the chain (src/samplers.jl:29-105): kept iterations = burnIn+thin : thin : chainLength
    done = 0
    smp_path = os.path.join(outFolder, "samples.ngpsmp")
    if samples in ("text", "binary"):
        smp.set_sample_file(smp_path)       # kept samples stream out while the chain runs: ONE ngp_run for the whole chain
    if samples == "text-sync":
        for it in range(nBurn + nThin, nChain + 1, nThin):
            smp.run(it - done)
            done = it
            st = smp.get_state()
            _out(outFolder, "b", (_fmt(st["b"]) if intercept else []) + (_fmt(smp.get_fixed()["b"]) if len(fixed_names) > int(intercept) else []))
            _out(outFolder, "varE", _fmt(st["varE"]))
            for rd in randoms:
                rr = smp.get_random_tuple(rd["id"])
                for name, fields in _rd_rows(rd, rr["u"], rr["varU"]):
                    _out(outFolder, name, fields)
            vb_off = 0
            for k, s in enumerate(sets):
                for m, nm in enumerate(s["members"]):
                    _out(outFolder, f"beta{nm}", _fmt(st["beta"][s["cols"][:, m]]))
                    _out(outFolder, f"delta{nm}", [str(int(v)) for v in st["delta"][s["cols"][:, m]]])
                if isinstance(s["prior"], (BayesBType, BayesCType)):
                    _out(outFolder, f"pi{s['name']}", _fmt(st["piHat"][2 * k:2 * k + 2]))
                if isinstance(s["prior"], (BayesRType, BayesRCType)):
                    _out(outFolder, f"pi{s['name']}", _fmt(smp.get_class_state(s["id"])["piHat"]))
                if isinstance(s["prior"], BayesRCType):
                    _out(outFolder, f"annot{s['name']}", [str(int(v)) for v in smp.rc_state(s["id"])["annotCat"]])
                if isinstance(s["prior"], BayesLogVarType):
                    lv = smp.lv_state(s["id"])
                    _out(outFolder, f"c{s['name']}", _fmt(lv["c"]))
                    _out(outFolder, f"varZeta{s['name']}", _fmt(lv["varZeta"]))
                _out(outFolder, f"var{s['name']}", _fmt(st["varBeta"][vb_off:vb_off + s["nvb"]]))
                vb_off += s["nvb"]
    smp.run(nChain - done)
    if samples in ("text", "binary"):
        smp.set_sample_file(None)
    if samples == "text":
        samples_to_out_files(smp_path, outFolder, sets, intercept, len(fixed_names) > int(intercept), randoms)
        os.remove(smp_path)
    return _posterior_means(smp, sets, fixed_names, intercept, randoms)


def _posterior_means(smp, sets, fixed_names, intercept, randoms=()):
    ps = smp.get_posterior_sums()
    n = max(ps["nKept"], 1)
    res = dict(nKept=ps["nKept"], b=ps["sum_b"] / n, varE=ps["sum_varE"] / n, sets={}, fixed_names=fixed_names,
               fixed=smp.get_fixed()["sum_b"] / n if len(fixed_names) > int(intercept) else np.zeros(0))
    vb_off = 0
    for k, s in enumerate(sets):
        for m, nm in enumerate(s["members"]):
            cm = s["cols"][:, m]
            res["sets"][nm] = dict(beta=ps["sum_beta"][cm] / n, delta=ps["sum_delta"][cm] / n,
                                   var=ps["sum_varBeta"][vb_off:vb_off + s["nvb"]] / n, pi=ps["sum_pi"][2 * k:2 * k + 2] / n)
            if s["k"] > 1:   # correlated sets: the posterior mean of every region's k x k covariance matrix
                res["sets"][nm]["var"] = (ps["sum_varBeta"][vb_off:vb_off + s["nvb"]] / n).reshape(s["nreg"], s["k"], s["k"])
        if isinstance(s["prior"], BayesRType):
            res["sets"][s["name"]]["pi"] = smp.get_class_state(s["id"])["sum_pi"] / n
        if isinstance(s["prior"], BayesRCType):       # pi per annotation and the posterior membership probabilities of every SNP
            rc = smp.rc_state(s["id"])
            res["sets"][s["name"]]["pi"] = rc["sum_pi"] / n
            res["sets"][s["name"]]["annot"] = rc["sum_annot"] / n
        if isinstance(s["prior"], BayesLogVarType):   # posterior means of the variance model's coefficients and of varZeta
            lv = smp.lv_state(s["id"])
            res["sets"][s["name"]]["c"] = lv["sum_c"] / n
            res["sets"][s["name"]]["varZeta"] = lv["sum_varZeta"] / n
        vb_off += s["nvb"]
    res["random"] = {}
    for rd in randoms:   # posterior means of u (levels in random_levels order) and varU, keyed as Julia prints the term
        if "members" in rd:   # a correlated (Tuple) set: u is k x q (one row per member, as the reference holds it), varU k x k
            rr = smp.get_random_tuple(rd["id"])
            res["random"][rd["key"]] = dict(u=rr["sum_u"].T / n, varU=rr["sum_varU"] / n, levels=rd["levels"])
            continue
        rr = smp.get_random(rd["id"])
        res["random"][rd.get("key", f"1 | {rd['g']}")] = dict(u=rr["sum_u"] / n, varU=rr["sum_varU"] / n, levels=rd["levels"])
    res["sampler"] = smp
    return res


def _pool_results(results):
    """Posterior means pooled over chains of equal length (the mean of the chains' means); res["chains"] keeps every chain's own."""
    w = np.array([r["nKept"] for r in results], dtype=np.float64)
    w = w / w.sum() if w.sum() > 0 else np.full(len(results), 1.0 / len(results))
    def avg(get):
        return sum(wi * np.asarray(get(r), dtype=np.float64) for wi, r in zip(w, results))
    pooled = dict(nKept=int(sum(r["nKept"] for r in results)), b=float(avg(lambda r: r["b"])), varE=float(avg(lambda r: r["varE"])),
                  fixed_names=results[0]["fixed_names"], fixed=avg(lambda r: r["fixed"]), sets={}, chains=results,
                  sampler=results[0]["sampler"], samplers=[r["sampler"] for r in results])
    for nm in results[0]["sets"]:
        pooled["sets"][nm] = {k: avg(lambda r, k=k: r["sets"][nm][k]) for k in results[0]["sets"][nm]}
    pooled["random"] = {nm: dict(u=avg(lambda r: r["random"][nm]["u"]), varU=(lambda v: float(v) if np.ndim(v) == 0 else v)(avg(lambda r: r["random"][nm]["varU"])),
                                 levels=results[0]["random"][nm]["levels"]) for nm in results[0].get("random", {})}
    return pooled
