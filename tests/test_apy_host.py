"""APY GBLUP, host side: the interface's symbols, the level order and runLMEM's refusals of apy= (no GPU needed)."""
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
APY_SYMBOLS = ["ngp_grm_begin_apy", "ngp_grm_apy", "ngp_grm_get_apy", "ngp_add_random_set_apy"]


@pytest.mark.parametrize("sym", APY_SYMBOLS)
def test_symbols(ngp, sym):
    assert sym in ngp.SYMBOLS
    with open(os.path.join(ROOT, "include", "nextgp_hip.h")) as f:
        assert f"int32_t {sym}(ngp_handle *h" in f.read()


@pytest.mark.parametrize("core", [3, [5, 0, 2]])
def test_level_order(ngp, core):
    order, nc = ngp.api.apy_order(7, core, apySeed=1)
    assert nc == 3 and sorted(order.tolist()) == list(range(7)) and np.all(np.diff(order[nc:]) > 0)
    if isinstance(core, list):
        assert order[:nc].tolist() == core
    else:
        assert order[:nc].tolist() == sorted(np.random.default_rng(1).choice(7, size=3, replace=False).tolist())
    for bad in (0, 8, [1, 1], [7]):
        with pytest.raises(ValueError):
            ngp.api.apy_order(7, bad)


G2 = 'y ~ 1 + SNP(M1, "a.txt") + SNP(M2, "b.txt")'


@pytest.mark.parametrize("formula,vcv,apy,extra,exc,word", [
    ("y ~ 1 + PED(ID)", {"ID": ("H", 1.0)}, {"ID": 3}, {}, NotImplementedError, "single-step"),
    (G2, {("M1", "M2"): ("G", np.eye(2))}, {"M1": 3}, {}, NotImplementedError, "tuple key"),
    (G2, {("M1", "M2"): ("G", np.eye(2))}, {("M1", "M2"): 3}, {}, NotImplementedError, "Tuple"),
    (G2, {"M1": ("G", 1.0)}, {"M1": 3}, dict(snpEffects=True), NotImplementedError, "snpEffects"),
    (G2, {"M1": ("G", 1.0)}, {"M1": 3}, dict(snpEffects=["M1"]), NotImplementedError, "snpEffects"),
    (G2, {"M1": ("G", 1.0)}, {"M1": 3}, dict(predict={"M1": "young.txt"}), NotImplementedError, "predict"),
    (G2, {"M1": ("G", 1.0)}, {"M2": 3}, {}, ValueError, "Random"),
])
def test_refusals(ngp, formula, vcv, apy, extra, exc, word):
    api = ngp.api
    VCV = {k: api.Random(*v) for k, v in vcv.items()}
    with pytest.raises(exc, match=word):
        api.apy_terms(apy, VCV, api.parse_formula(formula, random_effects=True, pedigree=True), **extra)
    assert api.apy_terms({"M1": [2, 0]}, {"M1": api.Random("G", 1.0)}, api.parse_formula(G2), snpEffects=["M2"], predict={"M2": "x"}) == {"M1": [2, 0]}


def test_runLMEM_refuses_before_it_reads_a_file(ngp, tmp_path):
    with pytest.raises(NotImplementedError, match="snpEffects"):
        ngp.runLMEM('y ~ 1 + SNP(M1, "no_such_file.txt")', dict(y=np.arange(5.0)), 10, 2, 1, outFolder=str(tmp_path / "o"),
                    VCV={"M1": ngp.Random("G", 1.0)}, apy={"M1": 3}, apySeed=1, snpEffects=True)
