"""nextgp.jl_amd -- MI355X-native marker-effect Gibbs sampler behind NextGP.jl's runLMEM interface.

The directory name contains a dot, so it is loaded by path (see `ngp_pkg.py` at the repo root):
    from ngp_pkg import load_pkg; ngp = load_pkg()
"""
from ._lib import (LIB_PATH, METHOD_BAYESB, METHOD_BAYESC, METHOD_BAYESPR, METHOD_BAYESLV, METHOD_BAYESR, METHOD_TUPLE, SYMBOLS, NextGPHipError, Sampler, load,  # noqa: F401
                   THRESHOLD_STEPS, censored_bounds, check_bounds, check_classes, class_codes, class_metrics, deal_folds, dense_csc, factors_csc, genomic_variance_names, genomic_variance_summary, holdout_summary, pedigree_a22, pedigree_ainv, prediction_summary, read_panel_header, read_sample_file, tuple_columns, tuple_panel, tuple_span, write_panel_file)
from .api import (BayesB, BayesC, BayesLV, BayesPR, BayesR, BayesRCπ, BayesRCpi, BayesRCplus, Random, SNP, design_codes, design_columns, gblup_terms, makeA, makeG, makePed, lv_design_matrix, is_panel_file, parse_formula, permute_csr, prep2RegionData,
                  read_genotypes, read_panel_file, read_prediction_file, runLMEM, samples_to_out_files, single_step_order, single_step_terms, summaryMCMC, write_gwas_files, write_prediction_file,
                  write_variance_out_files, convergencyMCMC, pool_diagnostics, read_convergence_file, write_convergence_file,
                  is_bed_file, read_plink, write_plink, decode_bed)  # noqa: F401,E402
from . import multichain  # noqa: F401,E402
