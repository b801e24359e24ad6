/*
 * nextgp_hip.h -- C ABI of libnextgp_hip.so, the MI355X (gfx950) replacement for the
 * marker-effect Gibbs hot path of NextGP.jl.
 *
 * Every entry point is what a Julia `ccall((:sym, "libnextgp_hip"), Cint, (...), ...)` binds;
 * INTEGRATION.md shows the reference-side shim.  All functions return 0 on success and a
 * negative code on failure; the message is retrievable with ngp_last_error().  No C++
 * exception, signal handler or exit() crosses this boundary.  Arrays are Julia-native:
 * column-major, contiguous, Float64 / Int64.  The library never retains a caller pointer
 * beyond the call; anything it keeps (panel, y, priors) is copied to device memory.
 *
 * Reference interfaces replaced (file:line under /root/reference):
 *   - coarse seam: samplers.runSampler!            src/samplers.jl:23-106 (called at src/MCMC.jl:39)
 *   - fine seam:   M[set].funct callback           src/samplers.jl:52, stored at src/mme.jl:326,333,355
 *                  = sampleBayesPR!/sampleBayesB!  src/functions.jl:118-137, 157-195
 *   - marker-matrix builders                       src/prepMatVec.jl:113-134, src/mme.jl:282-347,443-446,492-520
 */
#ifndef NEXTGP_HIP_H
#define NEXTGP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NGP_ABI_VERSION 4

#define NGP_OK 0
#define NGP_ERR_ARG (-1)     /* bad argument (null, size mismatch, non-finite value) */
#define NGP_ERR_STATE (-2)   /* call sequence error (panel / y / sets missing) */
#define NGP_ERR_HIP (-3)     /* HIP runtime error (message carries hipGetErrorString) */
#define NGP_ERR_NOMEM (-4)
#define NGP_ERR_NODEVICE (-5) /* no usable gfx950 device: the library has NO CPU fallback */
#define NGP_ERR_DEBUG (-6)    /* the call ran in a diagnostic timing mode (ngp_debug_set_mode): its results are invalid */

#define NGP_METHOD_BAYESPR 0 /* src/runTime.jl:30-45 */
#define NGP_METHOD_BAYESB 1  /* src/runTime.jl:48-61 */
#define NGP_METHOD_BAYESC 2  /* src/runTime.jl:64-77, sampler src/functions.jl:197-235 */
#define NGP_METHOD_BAYESR 3  /* src/runTime.jl:78-93, sampler src/functions.jl:238-289; added with ngp_add_marker_set_r */
#define NGP_METHOD_TUPLE 4   /* correlated sets, BayesPR's Tuple method: src/functions.jl:140-154; added with ngp_add_marker_set_tuple */
#define NGP_METHOD_BAYESLV 5 /* src/runTime.jl:116-133, sampler src/functions.jl:421-486; added with ngp_add_marker_set_lv */
#define NGP_METHOD_BAYESRC 6 /* BayesRCpi, annotation-informed BayesR: sampler src/functions.jl:291-360; added with ngp_add_marker_set_rc */
#define NGP_LV_MAXCOV 16     /* most columns of a BayesLV set's covariate matrix */

typedef struct ngp_handle ngp_handle;

int32_t ngp_abi_version(void);

/* One handle = one chain on one device (reference: one Julia task, src/samplers.jl:23).
 * seed/chain_id key every random stream (the reference never seeds its RNG). */
int32_t ngp_create(int32_t device, uint64_t seed, uint32_t chain_id, ngp_handle **out);
int32_t ngp_destroy(ngp_handle *h);
/* Message of the last failing call on h (h == NULL: last failing ngp_create). Valid until the next call. */
const char *ngp_last_error(ngp_handle *h);

/* Sweep engine, to be chosen BEFORE the panel is set (it fixes the tiling and the Gram window):
 * mode 1 (default) = one persistent kernel per iteration with look-ahead `lag` (1..8 blocks of 64 SNPs),
 * mode 0 = one streaming + one recursion launch per 64-SNP block (lag 1).  Both replace the same
 * reference loop (src/functions.jl:124-136) and draw the same chain; only summation order differs. */
int32_t ngp_configure(ngp_handle *h, int32_t mode, int32_t lag);
int32_t ngp_get_config(ngp_handle *h, int32_t *mode, int32_t *lag);
/* Persistent sweep only: look-ahead lags 1..near are corrected inside the sampler workgroup, lags near+1..lag-1 by the
 * reducer workgroups (another summation order, which the blocked oracle needs to know).  1..4, 0 = automatic (3 with the phase streamer,
 * 4 on its shards taller than 128 rows; 2 with the row-owning streamer from 64-row shards on); to be chosen before the panel is set.  ngp_get_near_lags reports the value in force. */
int32_t ngp_set_near_lags(ngp_handle *h, int32_t near);
int32_t ngp_get_near_lags(ngp_handle *h, int32_t *near);
/* Form of the block chain of BayesPR blocks (every lane BayesPR or unowned; replaces the per-SNP loop of src/functions.jl:124-136).
 * 0 (default): the 64 serial steps.  1: dlt = T e0 with T = inv(I + diag(c) strictLower(G)) of the block formed explicitly before every
 * sweep (k_tinv) -- the forward substitution the 64 steps carry out, as one 64 x 64 product.  The same Markov chain in real
 * arithmetic; the floating-point order differs, so the blocked oracle is told (ora_set_tform).  Measured:
 * pays where the sampler's serial chain is the bound (compact storage), costs 2-4 % where its CU's memory traffic is.  Any time
 * before ngp_run, also between two runs of one chain: the next ngp_run / ngp_run_many / ngp_sweep_set takes the form in force, and
 * ngp_get_chain_form reports the form the next sweep runs. */
int32_t ngp_set_chain_form(ngp_handle *h, int32_t form);
int32_t ngp_get_chain_form(ngp_handle *h, int32_t *form);
/* Diagnostic only: enable != 0 makes the persistent kernel write 100 MHz time stamps (sampler: 4 words per
 * block at [4u..4u+3]; streamer 0: 2 words per block from word 2^20); out/n copies the first n words back.  The stamps exist in the
 * diagnostic kernel only, which does not carry the rule of BayesRCpi sets: enabling them on a model with such a set is NGP_ERR_ARG
 * (and ngp_add_marker_set_rc refuses a handle whose stamps or timing mode are on). */
int32_t ngp_debug_stamps(ngp_handle *h, int32_t enable, uint64_t *out, int64_t n);

/* Marker panel, N individuals x P SNPs, column-major with leading dimension ld >= N
 * (replaces M[set][:data] + the M[set][:Mp] copy, src/prepMatVec.jl:116-131, src/mme.jl:305-311).
 * centre != 0: subtract the column mean first (src/prepMatVec.jl:129).  Stored as fp32, re-tiled. */
int32_t ngp_set_panel_f64(ngp_handle *h, const double *M, int64_t N, int64_t P, int64_t ld, int32_t centre);
int32_t ngp_set_panel_f32(ngp_handle *h, const float *M, int64_t N, int64_t P, int64_t ld, int32_t centre);
/* The same panel in column ranges: the reference keeps ONE Float64 matrix per marker set (M[set].data, src/mme.jl:296-311) and the
 * sweep wants ONE panel with the sets side by side -- so the sets are handed over one after another, no concatenated copy on the
 * host.  ngp_begin_panel fixes N x P (layout, allocation; a new model like every ngp_set_panel_*), ngp_panel_columns_* writes
 * columns [col0, col0 + ncol) from a column-major matrix (any order, any boundaries; columns never written stay zero columns),
 * ngp_end_panel builds mpm and the Gram window.  Conversion, centring and tiling run on the device from 256 MiB staging chunks
 * (ngp_set_panel_f64 / _f32 are these three calls).  Nothing else may be called on the handle between begin and end. */
int32_t ngp_begin_panel(ngp_handle *h, int64_t N, int64_t P);
int32_t ngp_panel_columns_f64(ngp_handle *h, int64_t col0, const double *M, int64_t ncol, int64_t ld, int32_t centre);
int32_t ngp_panel_columns_f32(ngp_handle *h, int64_t col0, const float *M, int64_t ncol, int64_t ld, int32_t centre);
/* ... and from one byte per genotype (codes 0..255; the tiles of ngp_set_panel_u8 bit for bit): the only form the compact storage
 * (ngp_set_storage) takes, and a quarter of the host footprint and PCIe transfer for the fp32 tiles. */
int32_t ngp_panel_columns_u8(ngp_handle *h, int64_t col0, const uint8_t *G, int64_t ncol, int64_t ld, int32_t centre);
/* ... and from the packed columns of a PLINK .bed file (SNP-major, magic 6c 1b 01; `packed` points behind the three magic bytes):
 * ncol columns, stride >= ceil(n_file / 4) bytes apart, sample i of the file in bits 2 (i mod 4) .. 2 (i mod 4) + 1 of byte i / 4,
 * two-bit values 0 = two copies of A1, 1 = missing, 2 = heterozygous, 3 = no copy of A1.  The stored genotype is the count of
 * A1 (allele 1) or of A2 (allele 2).  rows: NULL (n_file == N, row i is sample i) or N host indices into the file's samples, any
 * order, repeats allowed.  The columns cross PCIe packed and are decoded, gathered and tiled on the device (staging as above);
 * the caller's buffer may end ceil(n_file / 4) bytes into its last column, and pad bits and pad bytes are never read as genotypes.
 * missing: what a missing call among the selected rows becomes --
 *   ERROR  the call fails (NGP_ERR_ARG, "column <j> holds <n> missing calls") before the tiles of that chunk are written;
 *   MEAN   the column's mean over the observed calls, mu_obs: the stored mean is mu_obs and (centred) the tile value exactly 0.
 *          fp32 storage only (byte tiles hold codes);
 *   ROUND  the nearest code to mu_obs, (2 sum + n_obs) / (2 n_obs) in integers (ties up; 0 for a column without observed call):
 *          tiles and stored mean are those of ngp_panel_columns_u8 on the imputed codes, bit for bit.
 * counts: NULL or ncol x 4 int64, the numbers of 0, 1, 2 and missing among the N selected rows of every column. */
#define NGP_BED_MISSING_ERROR 0
#define NGP_BED_MISSING_MEAN  1
#define NGP_BED_MISSING_ROUND 2
int32_t ngp_panel_columns_bed(ngp_handle *h, int64_t col0, const uint8_t *packed, int64_t ncol, int64_t stride, int64_t n_file,
                              const int64_t *rows, int32_t allele, int32_t missing, int32_t centre, int64_t *counts);
int32_t ngp_end_panel(ngp_handle *h);
/* Same panel from one byte per genotype (0/1/2 allele counts, or any value 0..255): a quarter of the fp32 host footprint and
 * of the PCIe transfer; centring and the fp32 conversion happen on the device and give bit for bit the tiles of
 * ngp_set_panel_f64 on the same values (integer column sum / N). */
int32_t ngp_set_panel_u8(ngp_handle *h, const uint8_t *G, int64_t N, int64_t P, int64_t ld, int32_t centre);
/* Binary panel file -- replaces the text genotype file the reference parses into a Float64 matrix (CSV.read + Matrix,
 * src/prepMatVec.jl:116-131: hours at 50k x 600k) by a header and the genotype codes, column after column:
 *   bytes 0-7 "NGPPNL01" | int64 N | int64 P | int32 bits (8 or 2) | int32 0 | P columns of N bytes (bits 8) or of
 *   ceil(N/4) bytes, individual i in bits 2(i mod 4)..2(i mod 4)+1 of byte i/4 (bits 2: allele counts 0, 1, 2; code 3 refused).
 * ngp_write_panel_file writes one (no handle, host only; 0 or NGP_ERR_ARG), ngp_read_panel_header reads N, P, bits,
 * ngp_load_panel_file streams the file through a pinned buffer in chunks of whole column blocks straight into the tiles of the
 * handle's storage (fp32 centred tiles or, with NGP_STORAGE_U8, the bytes themselves): same tiles, bit for bit, as
 * ngp_set_panel_u8 on the same codes. */
int32_t ngp_write_panel_file(const char *path, const uint8_t *G, int64_t N, int64_t P, int64_t ld, int32_t bits);
int32_t ngp_read_panel_header(const char *path, int64_t *N, int64_t *P, int32_t *bits);
int32_t ngp_load_panel_file(ngp_handle *h, const char *path, int32_t centre);
/* Synthetic panel generated on the device: g_ij ~ Binomial(2,p_j), p_j ~ U(maf_lo,maf_hi). */
int32_t ngp_generate_panel(ngp_handle *h, int64_t N, int64_t P, double maf_lo, double maf_hi, uint64_t panel_seed);
/* Device tiling chosen for the panel: rows per shard R, shards S, 64-SNP blocks NBLK (the blocked
 * oracle needs R and S to reproduce the reduction tree). */
int32_t ngp_get_layout(ngp_handle *h, int64_t *R, int64_t *S, int64_t *nblk);
/* Wall time of the last ngp_generate_panel, in its three parts (milliseconds): device allocation with its zeroing, tile generation,
 * Gram window -- the set-up of a 120 GB panel is dominated by the first, which varies from box to box. */
int32_t ngp_get_setup_timing(ngp_handle *h, double *alloc_ms, double *tiles_ms, double *gram_ms);
/* x'x per SNP (M[set][:mpm], src/mme.jl:305-307); out has P entries. */
int32_t ngp_get_mpm(ngp_handle *h, double *out, int64_t P);
/* One 64x64 Gram block X_t'X_t (row-major); parity probe. */
int32_t ngp_get_gram(ngp_handle *h, int64_t t, double *out);
/* out = X * beta (N entries), X the stored fp32 panel: used to simulate phenotypes and to check
 * the invariant ycorr = y - 1b - X beta. */
int32_t ngp_xbeta(ngp_handle *h, const double *beta, int64_t P, double *out, int64_t N);

/* A marker set = columns [col0, col0+ncol) with its prior (src/mme.jl:324-361, 492-520).
 * method NGP_METHOD_*; df, scale as computed at src/mme.jl:493,501; regions are 0-based
 * [reg_start[r], reg_stop[r]) relative to the set (M[set][:regionArray], src/mme.jl:335-358);
 * varBeta0 holds nreg initial variances (src/mme.jl:516); BayesB needs nreg == ncol (one region
 * per locus, src/mme.jl:356), pi0 = prior inclusion probability, estPi (src/mme.jl:359); BayesC has nreg == 1 (one
 * variance for the whole set, src/functions.jl:205,231) and, like the reference, ignores rhs0 (src/functions.jl:220);
 * lhs0/rhs0 (ncol each or NULL) are the summary-statistics terms (src/mme.jl:314-322).
 * For every ngp_add_marker_set*: a call that is refused or fails leaves the handle as it was -- no set, no set id, the columns free. */
int32_t ngp_add_marker_set(ngp_handle *h, int64_t col0, int64_t ncol, int32_t method, double df, double scale,
                           const int64_t *reg_start, const int64_t *reg_stop, int64_t nreg, const double *varBeta0,
                           double pi0, int32_t estPi, const double *lhs0, const double *rhs0, int32_t *set_id);

/* BayesR marker set (set-up src/mme.jl:374-383): ONE variance for the set (varBeta0, nVarCov = 1), K = 2..16 variance classes with
 * multipliers vClass[v] of that variance (multiplier 0: the effect is exactly 0) and class probabilities pi[v] (sum 1);
 * estPi: pi ~ Dirichlet(nLoci + 1) after every sweep (src/functions.jl:284-288).  delta then holds the CLASS of a locus,
 * counted from 1 as the reference writes it (src/functions.jl:262).  The reference's class search compares cumulative
 * probabilities with a FRESH uniform per comparison (src/functions.jl:261); that is reproduced, one keyed uniform per (locus,
 * comparison).  ngp_get_state / ngp_get_posterior_sums report [0.5, 0.5]-style placeholders in piHat / sum_pi for such a set;
 * its K probabilities are read and restored with ngp_get_class_state / ngp_set_class_state, and travel in the packed
 * posterior (ngp_posterior_len) and in snapshots. */
int32_t ngp_add_marker_set_r(ngp_handle *h, int64_t col0, int64_t ncol, double df, double scale, double varBeta0, const double *vClass,
                             const double *pi, int32_t K, int32_t estPi, const double *lhs0, const double *rhs0, int32_t *set_id);
int32_t ngp_get_class_state(ngp_handle *h, int32_t set_id, double *piHat, double *sum_pi, int64_t *K);
int32_t ngp_set_class_state(ngp_handle *h, int32_t set_id, const double *piHat, const double *sum_pi, int64_t K);

/* Correlated marker sets -- sampleBayesPR!(::Tuple) (src/functions.jl:140-154), sampleVarCovBetaPR (:513-516), set-up
 * src/mme.jl:448-489: k = 1..4 sets (e.g. breeds) share nloc loci; every locus draws its k effects jointly, beta_l ~ MvNormal(inv(LHS)
 * RHS, inv(LHS)) with LHS = X_l'X_l / varE + inv(varBeta_r), and every region r draws its k x k variance matrix
 * varBeta_r ~ InverseWishart(df + n_r, scale + B_r'B_r).  df = 3 + k and scale = v (df - k - 1) (k x k, row-major) are the caller's
 * (src/mme.jl:493, 501); varBeta0 = v, ONE k x k matrix every region starts from (src/mme.jl:516); regions are ranges of LOCI.
 * Panel layout: the k columns of a locus are adjacent -- component m of locus l is panel column col0 + 64 (l / Lb) + k (l % Lb) + m,
 * Lb = floor(64 / k), col0 a multiple of 64 (a locus never straddles a 64-column block; for k = 3 column 63 of every block of the
 * set is unused and must hold zeros).  In ngp_get_state / ngp_get_posterior_sums the set contributes nreg k x k matrices
 * (row-major) to varBeta, and its effects sit at their panel columns.  k = 1 is the Symbol method of BayesPR, bit for bit (with
 * scale = the Symbol path's scale * df).  (In the reference snapshot this method is unreachable -- SURVEY.md fact 6 -- so parity is
 * against the specification in oracle/.)  MvNormal / InverseWishart: Cholesky and Bartlett constructions on the keyed draws. */
int32_t ngp_add_marker_set_tuple(ngp_handle *h, int64_t col0, int64_t nloc, int32_t k, double df, const double *scale,
                                 const int64_t *reg_start, const int64_t *reg_stop, int64_t nreg, const double *varBeta0, int32_t *set_id);

/* A fixed-effect set beyond the intercept (X[xSet] of src/prepMatVec.jl:150-165; set-up src/mme.jl:120-152): the columns of one
 * model term or of one `blockThese` group, N x ncol column-major (ncol <= 64), sampled after the intercept in the order the
 * sets are added (the `keys(X)` order of src/samplers.jl:39; to put the intercept elsewhere switch it off and add a column of
 * ones).  One column: sampleX! (src/functions.jl:41-47) with summary-statistics terms lhs0 / rhs0 (NULL = 0); several columns:
 * sampleb! (src/functions.jl:22-36), Gauss-Seidel over X'X + min|diag| / 10000 (src/mme.jl:149-152).  ngp_get_fixed returns the
 * current effects and their posterior sums (all columns of all sets, in order); ngp_set_fixed restores them (resume). */
int32_t ngp_add_fixed_set(ngp_handle *h, const double *X, int64_t N, int64_t ncol, int64_t ld, const double *lhs0, const double *rhs0,
                          int32_t *set_id);
/* The same kind of set given as a sparse matrix: a classification factor of thousands of levels (herd, contemporary group), or a
 * block of crossed factors and covariates.  CSC: col_ptr holds ncol + 1 offsets (col_ptr[0] = 0), row / val col_ptr[ncol] entries, the
 * rows strictly ascending inside a column.  2 <= ncol <= 2^20 (the draw key is (set + 1) << 20 | column, as for the dense set),
 * fewer than 2^31 entries, every column at least one, every value finite; else NGP_ERR_ARG and the handle is unchanged.  Single
 * columns and the summary-statistics terms stay with ngp_add_fixed_set.  The set takes its place among the fixed-effect sets in the
 * order added, dense and sparse mixed (16 in all), and appends its columns to what ngp_get_fixed / ngp_set_fixed, the packed
 * posterior, sample records, snapshots and diagnostics carry.  It is bit for bit the dense set of the same design wherever both
 * exist (a snapshot of one loads into the other): the stored entries are visited in the dense kernel's order and the partial sums
 * combined along its tree ("Sparse fixed-effect sets").  Cost per iteration: one pass over the stored entries
 * and over the stored entries of X'X, instead of N x ncol.  Under residual weights the values are scaled on the host (s_i val). */
int32_t ngp_add_fixed_set_sparse(ngp_handle *h, int64_t N, int64_t ncol, const int64_t *col_ptr, const int32_t *row, const double *val,
                                 int32_t *set_id);
int32_t ngp_get_fixed(ngp_handle *h, double *b, double *sum_b, int64_t *ncols_total);
int32_t ngp_set_fixed(ngp_handle *h, const double *b, const double *sum_b, int64_t ncols_total);

/* A (1|g) random-effect set (src/mme.jl:165-272, sampled by sampleZ! / sampleVarU, src/functions.jl:57-72, 92-97, 498-501): record i
 * belongs to level level[i] in 0..q-1 (Z one-hot, N x q); K = the structure's precision (Z.iVarStr: I, A^-1 or inv(Sigma)) as CSR
 * (k_ptr q + 1 entries, k_col / k_val k_ptr[q] entries, any column order within a row), all three NULL = identity.  Refused
 * (NGP_ERR_ARG, the handle unchanged): a level outside 0..q-1, a non-finite entry, a K that is not exactly symmetric, a diagonal entry
 * missing or <= 0, df <= 0, scale < 0, varU0 <= 0.  Levels without records are valid (zpz = 0: drawn from the prior conditional).
 * df = 3 + 1 and scale = v (df - 2) / df are the caller's (src/mme.jl:265-272), varU0 = v.  Sets are sampled after the fixed-effect
 * sets, in the order they are added; each iteration: Yi = Z'ycorr / varE + zpz u / varE without touching ycorr, Gauss-Seidel over K in
 * level order (Z'Z taken as diagonal, as the reference does), ycorr -= Z du, varU = (scale df + u'Ku) / chi2(df + q).  Under weighted
 * residuals zpz_l = sum of w over the level's records and Z'W ycorr is used.  Summation orders and draw keys: DESIGN.md, "Random-effect
 * sets".  A handle that shares a panel has its own random-effect sets.  With them, the packed posterior (ngp_posterior_len), the records
 * of ngp_set_sample_file and snapshots carry u and varU (see there); handles without them keep every layout unchanged. */
int32_t ngp_add_random_set(ngp_handle *h, const int32_t *level, int64_t q, const int64_t *k_ptr, const int32_t *k_col, const double *k_val,
                           double df, double scale, double varU0, int32_t *set_id);
/* Current u (q), their posterior sums (q), varU and its sum; any pointer may be NULL.  ngp_set_random restores them (resume). */
int32_t ngp_get_random(ngp_handle *h, int32_t set_id, double *u, double *sum_u, double *varU, double *sum_varU);
int32_t ngp_set_random(ngp_handle *h, int32_t set_id, const double *u, const double *sum_u, double varU, double sum_varU);
/* Fine seam of one random-effect set: sampleZ!(zSet, Z, u, ycorr, varE, varU) (src/functions.jl:92-97) on the caller's arrays, updated
 * in place (ycorr N, u q, varU one double).  Keyed like ngp_sweep_set: the set's own call counter is the iteration of its draws. */
int32_t ngp_sample_random_set(ngp_handle *h, int32_t set_id, double varE, double *ycorr, double *u, double *varU);
/* The Gauss-Seidel engine of a CSR set whose K has off-diagonal entries (a pedigree's A^-1).  mode 1: serial, one lane walks the levels
 * in order; mode 2: level-scheduled -- depth(l) = 0 for a row without an entry left of its diagonal, else 1 + max depth(c) over its
 * columns c < l; rows of equal depth are independent and run one thread per row, the depths in order (one launch per depth of more than
 * 1024 rows, one single-workgroup launch per run of narrower depths); mode 0: automatic (scheduled when q exceeds 2 levels per depth, the measured
 * crossover: DESIGN.md, "Random-effect sets"; serial otherwise).
 * Both engines do the same operations on the same values in the same order per row: no result depends on the mode, nor does the
 * signature of snapshots.  Refused (NGP_ERR_ARG): a mode outside 0..2, a set with a diagonal or a dense K.  ngp_get_random_schedule
 * returns the engine in force (0 none: diagonal or dense K, 1 serial, 2 scheduled), the number of depths and the Gauss-Seidel launches
 * per step; any pointer may be NULL. */
int32_t ngp_set_random_schedule(ngp_handle *h, int32_t set_id, int32_t mode);
int32_t ngp_get_random_schedule(ngp_handle *h, int32_t set_id, int32_t *engine, int64_t *depths, int64_t *launches);
/* A correlated (Tuple) random-effect set (src/mme.jl:207-239; sampleZ!(::Tuple), src/functions.jl:75-89, 100-110, 503-506): k = 1..4
 * components over ONE K with a k x k covariance -- (ID, Dam): direct and maternal genetic effects over one pedigree.  level is k x N,
 * component-major: level[m N + i] in 0..q-1, or -1 for a record without a level in component m (an unknown dam: the reference's
 * all-zero row of Z; ngp_add_random_set keeps refusing it).  K as for ngp_add_random_set, shared by the components.  scale and varU0
 * are k x k row-major and refused unless finite and symmetric positive definite; the caller passes df = 3 + k and
 * scale = v (df - k - 1) (src/mme.jl:265-271).  u and its sums are q x k with the k components of a level adjacent, varU and its sum
 * k x k row-major.  Tuple sets share the id sequence of the other random-effect sets and are sampled in the order added;
 * ngp_set_random_schedule / ngp_get_random_schedule apply (a tuple set always runs a Gauss-Seidel engine; its depths are those of the union
 * of the patterns of K and of the record links between levels).  ngp_get_random / ngp_set_random / ngp_sample_random_set refuse a set
 * with k > 1; the three functions below take any set (k = 1: a set of ngp_add_random_set or ngp_add_random_set_dense).
 *
 * THE STEP IS NOT THE REFERENCE'S LINES.  sampleZ!(::Tuple) forms Yi = Zp[i] ycorr on a ycorr that holds every component's Z u and
 * subtracts only the K (x) inv(varU) couplings: a record of animal a with dam d leaves u_Dam[d] in animal a's right-hand side
 * (Z_ID[:, a]'Z_Dam[:, d] != 0 is ignored).  The device draws the exact Gibbs conditional: K_lc (x) inv(varU) + W_lc / varE for c != l,
 * W_lc[a][b] = sum of 1 (of w_i under weighted residuals) over the records with level_a = l and level_b = c.  The two agree exactly
 * when no record links two different levels (all components on one level vector).  Per step: level sums and the k x k conditional per
 * level, Gauss-Seidel in level order, ycorr -= sum_m du_m[level_m], varU ~ InverseWishart(df + q, scale + U K U').  Summation orders and
 * draw keys: DESIGN.md, "Correlated random-effect sets".  A matrix that is not positive definite on the device shows as NaN in the
 * chain, as for Tuple marker sets.  k = 1 gives ngp_add_random_set's chain bit for bit with scale_tuple = scale * df.  Packed posterior,
 * sample records and snapshots carry u (q k) and varU (k k) where a (1|g) set has q and 1; the q word of the sample file's header and of the
 * snapshot signature carries k - 1 in its bits from 32 up. */
int32_t ngp_add_random_set_tuple(ngp_handle *h, const int32_t *level, int32_t k, int64_t q, const int64_t *k_ptr, const int32_t *k_col,
                                 const double *k_val, double df, const double *scale, const double *varU0, int32_t *set_id);
int32_t ngp_get_random_tuple(ngp_handle *h, int32_t set_id, double *u, double *sum_u, double *varU, double *sum_varU);
int32_t ngp_set_random_tuple(ngp_handle *h, int32_t set_id, const double *u, const double *sum_u, const double *varU, const double *sum_varU);
int32_t ngp_sample_random_set_tuple(ngp_handle *h, int32_t set_id, double varE, double *ycorr, double *u, double *varU);
/* A^-1 of a pedigree on the host (no device, no handle; messages through ngp_last_error(NULL)): n animals, sire[i] / dam[i] the 1-based
 * positions of the parents in the same list, 0 = unknown, parents in front of their offspring (any other order, an index outside 0..n, an
 * animal that is its own parent: NGP_ERR_ARG).  Inbreeding coefficients F (f_out, n entries, may be NULL) by Meuwissen and Luo's method;
 * Henderson's rules per animal i with known parents p (one parent listed twice counts twice): d = 1 - sum_p (1 + F_p) / 4, a = 1 / d,
 * K_ii += a, K_ip += -a/2, K_pi += -a/2, K_pp' += a/4 for every pair, in animal order -- reproducible and exactly symmetric.  CSR out:
 * k_ptr (n + 1 entries, may be NULL), k_col / k_val (cap entries; columns ascending within a row).  nnz_out is always set; a cap smaller
 * than it is NGP_ERR_ARG with k_ptr and f_out filled and k_col / k_val untouched: call with cap = 0 to count, then again to fill. */
int32_t ngp_pedigree_ainv(int64_t n, const int32_t *sire, const int32_t *dam, double *f_out, int64_t *k_ptr, int32_t *k_col, double *k_val,
                          int64_t cap, int64_t *nnz_out);
/* A22 = A[idx, idx] of the same pedigree WITHOUT the dense A (host only): Colleau's indirect method, one column per listed animal in O(n)
 * over A = T diag(d) T'.  f: the n inbreeding coefficients ngp_pedigree_ainv returns; idx: m 0-based positions (any order; outside 0..n-1:
 * NGP_ERR_ARG); A22: m x m out with leading dimension ld >= m, exactly symmetric (the triangle k >= j of column j is mirrored).  Per
 * column, x = e_idx[j]: backward from the animal to the oldest x[sire] += x[i]/2, x[dam] += x[i]/2; x[i] *= d_i (1, 0.75 - F_p/4,
 * 0.5 - (F_s + F_d)/4 with no, one, two known parents); forward w[i] = x[i] + (w[sire] + w[dam])/2; A22[j][k] = w[idx[k]].  The columns
 * are spread over min(16, m) host threads -- a fixed count, never the machine's -- and no bit depends on it. */
int32_t ngp_pedigree_a22(int64_t n, const int32_t *sire, const int32_t *dam, const double *f, const int64_t *idx, int64_t m, double *A22,
                         int64_t ld);

/* Phenotypes; resets the chain: ycorr = y (src/mme.jl:57), b = 0, beta = 0, delta = 1, u = 0, varU = varU0, iter = 0, every variance and pi back to
 * the values given to ngp_add_marker_set (src/mme.jl:351-360, 516), all posterior sums and nKept zero. */
int32_t ngp_set_y(ngp_handle *h, const double *y, int64_t N);
/* E.df, E.scale (src/mme.jl:87-94). */
int32_t ngp_set_residual_prior(ngp_handle *h, double df, double scale);
/* Weighted residuals, the reference's E.str == "D" (src/mme.jl:71-75): w = E.iVarStr, w_i = 1 / d_ii, N entries, each finite and > 0
 * (else NGP_ERR_ARG).  To be called BEFORE the panel (any ngp_set_panel_*, ngp_begin_panel, ngp_generate_panel, ngp_load_panel_file,
 * ngp_share_panel; NGP_ERR_STATE afterwards); the panel's N must then equal this N (NGP_ERR_ARG at the panel call).  w = NULL with
 * N = 0 removes the weights again (before the panel).  Compact storage (NGP_STORAGE_U8) takes no weights (NGP_ERR_ARG either way round).
 * The chain is the reference's weighted chain run on the row-scaled problem, s_i = sqrt(w_i) (IEEE sqrt on the host):
 *   tiles      x~_ij = (float)(s_i * ((double)x_ij - mu_j))   (one fp64 multiply after the centring, then the usual rounding to fp32;
 *                                                              mu_j the unweighted column mean that ngp_get_storage reports; padding 0)
 *   residual   y~_i = s_i * ycorr_i on the way in (ngp_set_y, ngp_set_state, ngp_sweep_set[_dev]);
 *              ycorr_i = y~_i / s_i on the way out (ngp_get_state, ngp_sweep_set[_dev]); ngp_xbeta returns (X~ beta)_i / s_i
 *   fixed sets X~ = s_i * X_ij on the device; X~'X~ and its ridge (src/mme.jl:133-152) from the scaled columns
 *   intercept  rhs from sum_i s_i y~_i, lhs from sum_w = w_0 + w_1 + ... + w_{N-1} (fp64, left to right, summed once here)
 * so x'Wx (ngp_get_mpm, the Gram window), x'W ycorr and sum w ycorr^2 (varE) come out of the unchanged sweep.  Weights of all ones
 * reproduce the unweighted chain bit for bit.  A handle that shares a panel (ngp_share_panel) takes the owner's weights; snapshots hold
 * the scaled residual and refuse a handle with other weights.  ngp_get_residual_weights copies w back (NGP_ERR_STATE: none set). */
int32_t ngp_set_residual_weights(ngp_handle *h, const double *w, int64_t N);
int32_t ngp_get_residual_weights(ngp_handle *h, double *w, int64_t N);
/* Whether the model has the intercept column (src/functions.jl:41-47); default on. */
int32_t ngp_set_intercept(ngp_handle *h, int32_t on);
/* chainLength, burnIn, outputFreq of runSampler! (src/samplers.jl:23-26): iterations
 * burnIn+thin : thin : chainLength are accumulated into the posterior sums. */
int32_t ngp_set_schedule(ngp_handle *h, int64_t chainLength, int64_t burnIn, int64_t thin);

/* Coarse seam: advance the chain by niter full iterations on the device
 * (varE -> intercept -> every marker set -> variance / pi draws; src/samplers.jl:29-55). */
int32_t ngp_run(ngp_handle *h, int64_t niter);

/* Chain state after the last iteration.  Any pointer may be NULL.  ycorr: N; beta, delta: P;
 * varBeta: sum of nreg over sets; piHat: 2 per set ([1-pi, pi], src/mme.jl:360). */
int32_t ngp_get_state(ngp_handle *h, double *ycorr, double *beta, int64_t *delta, double *varBeta, double *piHat, double *varE,
                      double *b, int64_t *iter);
/* Resume support: overwrite the chain state (same shapes as ngp_get_state). */
int32_t ngp_set_state(ngp_handle *h, const double *ycorr, const double *beta, const int64_t *delta, const double *varBeta,
                      const double *piHat, double varE, double b, int64_t iter);
/* varE and intercept of each iteration of the last ngp_run (n <= niter entries). */
int32_t ngp_get_trace(ngp_handle *h, double *varE, double *b, int64_t n);
/* Sums over kept iterations (posterior mean = sum / nKept; replaces summaryMCMC, src/misc.jl:241-244). */
int32_t ngp_get_posterior_sums(ngp_handle *h, double *sum_beta, double *sum_beta2, double *sum_delta, double *sum_varBeta,
                               double *sum_pi, double *sum_varE, double *sum_b, int64_t *nKept);
/* Same sums packed into a DEVICE buffer [sum_beta P | sum_beta2 P | sum_delta P | sum_varBeta nvb |
 * sum_pi 2*nsets | class-probability sums of the BayesR sets, K each | sums of the fixed effects beyond the intercept, all
 * columns of all sets in order (ngp_get_fixed) | with random-effect sets: sums of u, set after set, then the sums of varU, one per set |
 * sum_varE | sum_b | nKept] so the host can all-reduce them over RCCL without a PCIe round trip.  len = 3P + nvb + 2 nsets + sum K +
 * nfixcol (+ sum q + nrand) + 3 doubles; a chain with held-out records (ngp_set_holdout, m > 0) appends sum_fit[N] | sum_fit2[N] |
 * n_fit[N], 3 N doubles more, so that ngp_allreduce_posterior over K fold-chains leaves every record's pooled sums on every handle. */
int32_t ngp_posterior_len(ngp_handle *h, int64_t *len);
int32_t ngp_export_posterior_device(ngp_handle *h, void *device_ptr, int64_t len);

/* Fine seam: one call of M[set].funct(mSet, M, beta, delta, ycorr, varE, varBeta) (src/samplers.jl:52).
 * In/out arrays are the caller's: ycorr N, beta ncol, delta ncol (out), varBeta nreg, piHat 2 (BayesB).
 * The call works in the handle's own chain arrays: the handle's residual, the set's effects, indicators, variances and pi, and varE
 * then hold the caller's values, so a chain that ngp_run has under way on the same handle does not go on as if the call had not been
 * made (put its state back with ngp_set_state, or keep one handle per seam).  What the call returns does not depend on the handle's
 * chain: the set's own call counter keys its draws, ngp_set_y restarts it. */
int32_t ngp_sweep_set(ngp_handle *h, int32_t set_id, double varE, double *ycorr, double *beta, int64_t *delta, double *varBeta,
                      double *piHat);
/* The same call with the caller's state in DEVICE memory of the handle's device (ycorr N, beta ncol, varBeta nreg doubles; delta
 * ncol int64, may be null; piHat 2 doubles, BayesB / BayesC): device-to-device copies on the handle's stream, no PCIe round trip per
 * set and iteration for a host that keeps its state on the GPU (ROCArrays).  Values are not validated on the host: a variance that
 * is not finite poisons the chain visibly, as in ngp_run.  Returns after the stream has drained. */
int32_t ngp_sweep_set_dev(ngp_handle *h, int32_t set_id, double varE, void *d_ycorr, void *d_beta, void *d_delta, void *d_varBeta,
                          void *d_piHat);

/* Device time of the iterations of ngp_run (HIP events on the handle's stream) and the number of sweep-kernel launches,
 * both accumulated since the last call. */
int32_t ngp_get_timing(ngp_handle *h, int64_t *sweep_launches, double *iter_ms, int64_t *iters);
/* Runs ONE extra iteration with a HIP event pair around every sweep-kernel launch and returns the
 * average launch duration of the dominant (panel-streaming) kernel, its launch count and the
 * algorithmic bytes one launch streams (bench.py roofline). */
int32_t ngp_profile_iteration(ngp_handle *h, double *avg_ms, int64_t *launches, double *bytes_per_launch);

/* Test probe of the device draw layer: n first draws of streams (seed,chain,iter,kind,index0+i);
 * what: 0 uniform, 1 normal, 2 chisq(p1), 3 beta(p1,p2), 4 gamma(p1). */
int32_t ngp_draws_indexed(ngp_handle *h, uint64_t iter, uint64_t kind, uint64_t index0, int32_t what, double p1, double p2,
                          int64_t n, double *out);
/* det_log / ppnd16 evaluated on the device (bit-parity probe), n inputs -> n outputs.  which: 0 det_log, 1 ppnd16, 2 sqrt,
 * 3 1 / x, 4 det_exp_any (exp for arguments of either sign: BayesLV's slice bounds). */
int32_t ngp_eval_math(ngp_handle *h, int32_t which, const double *in, int64_t n, double *out);

/* ---- streamer variants of the persistent sweep (before the panel is set) ----
 * 0 = automatic, 1 = phase streamer (every shard height), 2 = row-owning waves + loader wave (shards of at most 224 rows,
 * lags 3..6; the default for shards of 64 to 224 rows).  Both replace the loop of src/functions.jl:124-136; they differ in
 * the summation order of the shard partial of X_t'ycorr only: ngp_get_streamer reports the variant in force and the number of
 * GEMV chains per partial (8 or 7), which the blocked oracle needs like R, S, lag and near lags.
 * 4 / 6 = variant 2 with TWO / THREE shards per streamer workgroup (lag 3 / lag 2): what fp32 panels of more than 63,232 rows (one
 * resident wave of 256-row shards) run in automatically -- two up to 107,520 rows, three up to 156,576 on 256 CUs; the layout (R, S)
 * and every result are those of variant 2 with that layout and lag, only the grid is S / 2 or S / 3 streamers (ngp_get_streamer
 * reports 2).  Taller fp32 panels fall back to the per-block engine (mode 0) -- or take the compact storage, whose shards reach
 * 896 rows. */
int32_t ngp_set_streamer(ngp_handle *h, int32_t variant);
int32_t ngp_get_streamer(ngp_handle *h, int32_t *variant, int32_t *gemv_chains);

/* ---- panel storage (before the panel is set) ----
 * NGP_STORAGE_F32 (default): the centred panel as fp32 tiles (4 bytes per genotype).
 * NGP_STORAGE_U8 ("compact"): the genotype codes stay one byte each and the centring of src/prepMatVec.jl:129 is applied
 * analytically with the Float64 column means m_j = (sum_i g_ij) / N: x_j'ycorr = sum_i g_ij ycorr_i - m_j sum_i ycorr_i,
 * ycorr -= x_j dlt = ycorr_i - (g_ij dlt - m_j dlt), x_k'x_j = (exact integer dot product) - N m_k m_j.  A quarter of the
 * memory and of the bytes streamed per iteration, and no fp32 rounding of the panel: the chain agrees with the reference's
 * Float64 arithmetic to rounding error of the sums (the fp32 tiles deviate by ~1e-7 relative).  Persistent sweep only; shards
 * are multiples of 16 rows (up to 896 rows, N up to ~196k on one MI355X); look-ahead lags 3, 4, 6, 8, 12 (4 or 8 for shards
 * taller than 224 rows, 4 above 448 rows; a request is rounded down to the next of these); ngp_get_streamer reports variant 3, 7 GEMV chains.  Input: ngp_set_panel_u8,
 * ngp_load_panel_file, ngp_generate_panel (ngp_set_panel_f64 / _f32 are refused: they carry centred values, not codes).
 * ngp_get_storage: the storage in force and, optionally, the P column means the library subtracted (src/prepMatVec.jl:129; zeros where
 * the caller passed centre = 0): with them a host can rebuild any centred row of the panel from the genotype codes. */
/* ngp_set_max_shards: the persistent sweep normally splits the rows over every CU but the sampler's and the reducers' (one
 * streamer workgroup per CU, all co-resident).  A smaller number makes the shards taller and leaves CUs free -- for a second
 * chain on the same device (each chain's whole grid must be resident at once), or to exercise tall-shard layouts on small
 * panels.  0 = automatic.  Before the panel is set.  Chains of ONE process that share a device (one handle and one host thread
 * each) are kept apart by the library: a call that launches sweeps leases ceil(grid / 8) CUs of every XCD for its duration, and
 * a call whose grid does not fit beside the running ones waits for them to return (the chains then take turns); sweeps of other
 * processes cannot be seen -- against those the bounded waits of the kernel remain (NGP_ERR_HIP, chain to be set again). */
int32_t ngp_set_max_shards(ngp_handle *h, int32_t max_shards);
/* The largest max_shards with which `chains` chains of this handle's device are co-resident (256 CUs: 247 for one chain, 123
 * for two, 76 for three, 61 for four). */
int32_t ngp_shards_for_chains(ngp_handle *h, int32_t chains, int32_t *max_shards);
/* ---- K chains per pass over the panel ----
 * Independent chains (one handle each) that share ONE panel run their sweeps in ONE kernel launch per iteration: every streamer
 * workgroup forms X_t'[y_1 .. y_K] from each tile it reads, so the panel is streamed once for K iterations' worth of sampling;
 * every chain keeps its own sampler workgroup, reducers, hand-off rings and draws, and stays bit for bit the chain it is alone with
 * the same layout.  Set-up: the first handle sets the panel (after ngp_set_max_shards(ngp_shards_for_pass(K))), the others call
 * ngp_share_panel(h, first) in place of a panel upload -- no copy of the panel is made; then each handle gets its own marker sets,
 * y and seeds, and ngp_run_many(handles, K, niter) runs them fused (engines served: persistent sweep over fp32 tiles with shards of at
 * most 64 rows, lag 6 or 8, 2..8 chains -- e.g. 10k x 100k; shards of 64..224 rows, lag 4..6, two chains -- e.g. 50k x 600k; compact storage,
 * two or three chains; every method, Tuple, BayesR and BayesRCpi sets included, and the chains of a pass need not hold the same
 * methods; other layouts -- fp32 panels whose streamer workgroups own several shards among them -- run the handles side by side as before).  Independent chains are
 * the path's own parallelism (src/samplers.jl:23: one chain per Julia task). */
int32_t ngp_share_panel(ngp_handle *h, ngp_handle *owner);
int32_t ngp_shards_for_pass(ngp_handle *h, int32_t chains, int32_t *max_shards);
#define NGP_STORAGE_F32 0
#define NGP_STORAGE_U8 1
int32_t ngp_set_storage(ngp_handle *h, int32_t storage);
int32_t ngp_get_storage(ngp_handle *h, int32_t *storage, double *means, int64_t P);

/* Diagnostic timing modes of the persistent kernel (1..6: parts of the pipeline switched off, ngp_sweep.h).  They are an
 * explicit, per-handle setting -- never read from the environment -- and while one is active ngp_run / ngp_sweep_set do
 * their launches and then return NGP_ERR_DEBUG: the chain they leave behind is invalid.  0 = off.  A model with a BayesRCpi set
 * takes 0 only (NGP_ERR_ARG otherwise): its sweep kernel has no timing modes. */
int32_t ngp_debug_set_mode(ngp_handle *h, int32_t mode);
/* Tuning knob of the row-owning streamer: pacing of its loader wave, 0..4 = s_sleep units (64 clocks) after every four tile
 * requests (default 0), + 16 = count every partial before the block's barrier, + 1024 (before the panel is set) = build the Gram window
 * on the matrix cores (v_mfma_f64_16x16x4_f64) instead of the fp64 VALU kernel: the same sums in the same order, bit for bit;
 * + 2048 = the row-owning streamers over fp32 tiles on the sampler's XCD do not warm its L2 with the next block's Gram planes;
 * + 8192 = the warmer role (ngp_get_warmer) is withheld, + 16384 = it is offered below 160-row shards too;
 * + 32768 = the row waves of the row-owning streamer over fp32 tiles load none of their quads themselves (the loader wave requests every
 * quad, ngp_get_census), + 1 << 28 = they do so below 160-row shards too, wherever the loader keeps its early part;
 * bits 16-27 = shard + 1 whose barrier-arrival timeline the diagnostic kernel records (0: shard 1).  Changes timing only, never results. */
int32_t ngp_debug_set_knob(ngp_handle *h, int32_t knob);

/* Resume support, second half: overwrite the posterior sums (same shapes as ngp_get_posterior_sums).  With ngp_set_state a
 * resumed run then reproduces the posterior means of the uninterrupted one -- the role of the reference's append-only *Out
 * files (src/outFiles.jl:17-21, rows written at src/samplers.jl:56-104). */
int32_t ngp_set_posterior_sums(ngp_handle *h, const double *sum_beta, const double *sum_beta2, const double *sum_delta,
                               const double *sum_varBeta, const double *sum_pi, double sum_varE, double sum_b, int64_t nKept);
/* Binary snapshot of chain state + posterior sums + draw-stream identity (seed, chain) in one file (written to path.tmp, then
 * renamed).  ngp_load_snapshot needs the same model (panel, sets, y) built first and verifies N, P, variance components and
 * sets; afterwards ngp_run continues the interrupted chain bit for bit. */
int32_t ngp_save_snapshot(ngp_handle *h, const char *path);
int32_t ngp_load_snapshot(ngp_handle *h, const char *path);

/* Per-iteration traces beyond varE / b (ngp_get_trace): effects of up to 4096 chosen loci (0-based panel columns), the first
 * n_varBeta variance components and pi of every set, recorded for every iteration of the following ngp_run calls (what
 * the reference writes as rows of beta<set>Out / var<set>Out / pi<set>Out, src/samplers.jl:80-84, for these columns).
 * ngp_get_trace_ext copies the first n iterations of the last ngp_run: beta_tr[n][nloci], varBeta_tr[n][n_varBeta], pi_tr[n][nsets]. */
int32_t ngp_set_trace_loci(ngp_handle *h, const int64_t *loci, int64_t n, int64_t n_varBeta);
int32_t ngp_get_trace_ext(ngp_handle *h, double *beta_tr, double *varBeta_tr, double *pi_tr, int64_t n);

/* Posterior sums pooled over n chains (one handle per chain, src/samplers.jl:23 runs one chain per Julia task): afterwards
 * every handle holds the sums over all chains.  Handles on different devices: ONE RCCL all-reduce (fp64 sum) over xGMI, RCCL
 * loaded on first use; handles sharing a device are added on the device.  Errors are reported on hs[0]. */
int32_t ngp_allreduce_posterior(ngp_handle **hs, int32_t n);
/* niter iterations of n chains at once, one host thread per handle inside the library (what n Julia tasks calling ngp_run
 * would do).  Chains on different devices run in parallel; chains sharing a device run side by side when their grids fit it
 * together (ngp_set_max_shards: e.g. three chains of 10k x 100k on one MI355X, 801 instead of 346 iterations/s in all) and in
 * turns otherwise.  Every chain is bit for bit what it is alone.  Returns the first non-zero status (message on that handle). */
int32_t ngp_run_many(ngp_handle **hs, int32_t n, int64_t niter);

/* Kept samples to a binary file without stopping the chain -- the role of the reference's per-iteration text rows (src/samplers.jl:56-104,
 * src/outFiles.jl:17-21).  From the next ngp_run on, every kept iteration leaves one record (packed on the device, copied on a second
 * stream, written by a thread of the library); ngp_run returns when its last record is in the file.  NULL closes the file.  Layout:
 * "NGPSMP01" | int64 P, nvb, nsets, nfix, nclass, record bytes | per set int64 {method, K, col0, ncol, variance entries, tuple k} |
 * records: int64 iteration | varE | b | b_fixed[nfix] | beta[P] | varBeta[nvb] | piHat[2 nsets] | class probabilities[nclass] |
 * delta[P] (bytes, padded to 8).  A chain with random-effect sets writes "NGPSMP02": the header goes on with int64 nrand | q per set, and
 * every record holds u (set after set) and varU[nrand] between b_fixed and beta. */
int32_t ngp_set_sample_file(ngp_handle *h, const char *path);
/* Placement census of the last persistent-sweep launch: out[b] = (XCC id + 1) << 32 | HW_REG_HW_ID of workgroup b (0: never resident),
 * n >= *grid entries; bits 40-63 of a row-owning streamer's entry over fp32 tiles: quads of that launch which its wave 0 loaded itself
 * instead of taking them from the loader wave (0 where the loader brings every quad).  Every launch of the persistent kernel opens with a census of its own grid (all of its workgroups wait for
 * each other, so all must be resident at once); a launch whose grid is not complete within 20 ms ends before any role has touched
 * the chain, and the call runs it again with the whole device leased (the chains of one process then take turns) -- *retries counts
 * those, *exclusive says whether this handle now always leases the whole device.  Any pointer may be NULL. */
int32_t ngp_get_census(ngp_handle *h, uint64_t *out, int64_t n, int64_t *grid, int64_t *retries, int32_t *exclusive);
/* The warmer of the last persistent-sweep launch: where the last reducer workgroup has no far lag to correct and shares the sampler's
 * XCD, it pulls the next blocks' Gram planes into that XCD's L2 in place of the streamers' loader waves (speed only).  *active = 1
 * if it did, *blocks = blocks it warmed in that launch; both 0 where there is no such workgroup.  The role is offered beside the
 * row-owning streamer over fp32 tiles with shards of 160 rows or more, where it was measured to pay.  Either pointer may be NULL. */
int32_t ngp_get_warmer(ngp_handle *h, int32_t *active, int64_t *blocks);
/* Test hook of that fallback: the sweep of iteration `iteration` (counted as ngp_get_state's iter) closes its own census as timed
 * out, once; the call must resume it and end bit for bit where an undisturbed chain ends.  0 = off. */
int32_t ngp_debug_fail_census(ngp_handle *h, int64_t iteration);
/* Test hook of ngp_allreduce_posterior: group this handle under virtual device vdev (-1: its real device).  Handles of ONE GPU with
 * different virtual devices then take the multi-device branch (leaders, packing, unpacking); the collective itself is a sum on that
 * GPU instead of ncclAllReduce. */
int32_t ngp_debug_set_virtual_device(ngp_handle *h, int32_t vdev);
/* Test hook of the exception barrier: throws a C++ exception inside an entry point (kind 0 std::bad_alloc, 1 std::length_error,
 * 2 a non-standard one); what comes back is a negative status and a message -- never an unwind into the caller.  h may be NULL. */
int32_t ngp_debug_throw(ngp_handle *h, int32_t kind);
/* Test hook of the staged loaders: every loop that stages host columns or a panel file through a fixed-size buffer (256 MiB:
 * ngp_set_panel_f64 / _f32, ngp_panel_columns_*, ngp_grm_columns_*, ngp_prediction_columns_*; 64 MiB: ngp_set_panel_u8,
 * ngp_load_panel_file, ngp_load_prediction_file) takes `bytes` for that size, so that a small panel crosses many chunk boundaries.
 * The rounding of each loop stays (at least one column, one 64-column block, 64 columns of a relationship matrix and multiples of
 * 64 there); results never depend on the value.  0 = the defaults; negative: NGP_ERR_ARG. */
int32_t ngp_debug_set_staging_bytes(ngp_handle *h, int64_t bytes);

/* ---- BayesLV sets: a log-linear model of the SNP variances (src/runTime.jl:116-133, src/functions.jl:421-486) ----
 * Columns [col0, col0 + ncol) with one variance per locus (all varBeta0 at first).  The sweep is BayesPR's with one region per locus
 * (bit for bit, given the variances); behind it the variance step draws every locus' variance by a slice step around
 * exp(C c + zeta), then c ~ N(iCpC C'logVar, iCpC varZeta) and zeta = logVar - C c ("BayesLV sets").
 * C: ncol x ncov covariates, column-major with leading dimension ld (ncov in 1..NGP_LV_MAXCOV), the design matrix of the variance
 * formula (src/mme.jl:427).  The library forms C'C, adds min_i |(C'C)_ii / 10000| to its diagonal (src/mme.jl:433-436) and inverts
 * it in Float64 by a Cholesky factorisation.  varZeta0 > 0: the variance of zeta; est_mode 0 keeps it, 1 sets it to var(zeta) and
 * 2 to est_fraction var(logVar) after every step (estimateVarZeta false / true / a Float64).  zeta0: ncol starting values of zeta
 * (the reference: unseeded rand(ncol), src/mme.jl:430), or NULL for keyed uniforms (kind 16); ngp_set_y goes back to them.
 * lhs0 / rhs0 as for ngp_add_marker_set.  The set contributes ncol entries to varBeta and a [0.5, 0.5] placeholder to piHat.
 * NGP_ERR_ARG: ncov outside 1..16, a non-finite entry of C or zeta0, varBeta0 <= 0, varZeta0 <= 0, est_mode
 * outside 0..2, est_fraction <= 0 in mode 2, ncol < 2 with an estimated varZeta, a C'C whose Cholesky factorisation fails.
 * The fine seam (ngp_sweep_set, ngp_sweep_set_dev) on such a set does the sweep AND the variance step: varBeta (ncol) is in / out on
 * the caller's arrays; zeta, c and varZeta live in the handle. */
int32_t ngp_add_marker_set_lv(ngp_handle *h, int64_t col0, int64_t ncol, double varBeta0, const double *C, int64_t ld, int32_t ncov,
                              double varZeta0, int32_t est_mode, double est_fraction, const double *zeta0, const double *lhs0,
                              const double *rhs0, int32_t *set_id);
/* State of a BayesLV set: c[ncov], its posterior sums, varZeta and its sum, zeta[ncol], iCpC[ncov x ncov] (row-major, symmetric) and
 * the number of loci whose slice was empty ("trapped", their variance kept) in the last iteration.  Any pointer may be NULL. */
int32_t ngp_get_lv_state(ngp_handle *h, int32_t set_id, double *c, double *sum_c, double *varZeta, double *sum_varZeta, double *zeta,
                         double *iCpC, int64_t *trapped);
/* Resume: c / sum_c / zeta may be NULL (left as they are); varZeta > 0. */
int32_t ngp_set_lv_state(ngp_handle *h, int32_t set_id, const double *c, const double *sum_c, double varZeta, double sum_varZeta,
                         const double *zeta);

/* ---- GBLUP: a SNP term with a Random("G", v) prior (src/prepMatVec.jl:122-126) ----
 * The reference forms VanRaden's genomic relationship matrix G from the raw genotypes (makeG, src/misc.jl:145-160), inverts it and samples
 * one breeding value per individual over the dense N x N precision K = inv(G) (sampleZ!, src/functions.jl:57-72, 92-97, 498-501).  Here:
 * ngp_grm_begin / ngp_grm_columns_* / ngp_grm_end build G on the device, ngp_grm_invert turns it into K, ngp_add_random_set_dense makes a
 * random-effect set of it.  The builder is independent of the genotype panel, of ngp_set_storage and of the model: it may be used on
 * a fresh handle, and a handle has at most one matrix under construction.  All of it is fp64 (the inverse multiplies input rounding by the
 * condition number of G); the matrix product runs on the matrix cores.
 *
 * ngp_grm_begin: method 1 or 2 (src/misc.jl:149-156); allocates the accumulator (N rounded up to 64, squared, doubles).
 * ngp_grm_columns_*: ncol raw (uncentred) genotype columns, column-major with leading dimension ld >= N, host memory; staged in
 * chunks of 256 MiB.  Per column, on the device: mean, p = mean / 2, centring, for method 2 the division by sqrt(2 p (1 - p)); then
 * G += Xc Xc'.  _f32 and _u8 convert exactly to fp64 first: on equal values the three give the same bits.  The result does not depend on
 * how the columns are split into calls as long as every call but the last brings a multiple of 64 columns: every entry of G is one
 * chain of matrix-core accumulations over the columns in their order, and the sum of 2 p q (method 1) is added up in column order.
 * Refused with NGP_ERR_ARG (G unchanged by that call's failing chunk, the builder still open): a non-finite genotype; under method 2 a
 * column with 2 p (1 - p) = 0 (monomorphic), which the reference divides 0 by 0 and poisons G with -- the message names the column.
 * Method 1 takes monomorphic columns as the zero columns they become.
 * ngp_grm_end: divides by sum 2 p q (method 1) or by the number of columns (method 2), adds 0.001 to the diagonal (src/misc.jl:158) and
 * mirrors the computed triangle: G is exactly symmetric.  A sum of 2 p q that is not positive (method 1, every column monomorphic) is
 * NGP_ERR_ARG and drops the matrix.
 * ngp_grm_get: the N x N matrix to the host (G after ngp_grm_end, K after ngp_grm_invert).
 * ngp_grm_invert: Cholesky factorisation and inverse in place (rocSOLVER dpotrf / dpotri, loaded on first use: NGP_ERR_HIP with a clear
 * message if it is absent; no host fallback), then the computed triangle is mirrored: K is exactly symmetric.  A matrix that is not
 * positive definite is NGP_ERR_ARG with the failing pivot (the matrix is dropped); before ngp_grm_end: NGP_ERR_STATE. */
int32_t ngp_grm_begin(ngp_handle *h, int64_t N, int32_t method);
int32_t ngp_grm_columns_f64(ngp_handle *h, const double *M, int64_t ncol, int64_t ld);
int32_t ngp_grm_columns_f32(ngp_handle *h, const float *M, int64_t ncol, int64_t ld);
int32_t ngp_grm_columns_u8(ngp_handle *h, const uint8_t *M, int64_t ncol, int64_t ld);
int32_t ngp_grm_end(ngp_handle *h);
int32_t ngp_grm_get(ngp_handle *h, double *G_out);
int32_t ngp_grm_invert(ngp_handle *h);
/* A random-effect set whose K is a dense q x q matrix: GBLUP's inv(G), or Random(Sigma, v) with a large dense Sigma.  Everything
 * ngp_add_random_set says about levels, df, scale, varU0, the sampling order, the draw keys, weighted residuals, ngp_get_random /
 * ngp_set_random / ngp_sample_random_set, the packed posterior, sample files and snapshots holds here too (a dense set and a CSR set with
 * the same id consume the same random numbers); what differs is the engine of the Gauss-Seidel: blocks of 64 levels, one launch per
 * block over all compute units, K read once per iteration (8 q^2 bytes), u'Ku formed without a second pass ("Dense
 * random-effect sets and the GRM": the normative summation orders).  A dense array given to ngp_add_random_set keeps going to the CSR
 * engine.  level == NULL: the identity incidence of GBLUP (record i is level i; q must equal N).  K comes from ONE of
 *   K != NULL                   a host array of q x q doubles, exactly symmetric and finite (else NGP_ERR_ARG), copied to the device;
 *   K == NULL, k_src != NULL    the dense K of set k_src_set of ANOTHER handle on the same device, by reference: no copy is made, the
 *                               matrix is read-only and lives as long as any set refers to it (chains = 8 is one matrix, not eight);
 *   K == NULL, k_src == NULL    this handle's own inverted relationship matrix (ngp_grm_invert), without a copy: the set takes it
 *                               over, the builder is empty afterwards.
 * k_src must be a complete handle (panel or records set) that no other thread is setting up during this call.
 * A diagonal entry of K that is not > 0 is NGP_ERR_ARG.  The model signature of snapshots digests the level coding and every entry
 * of K, as for a CSR set; the matrix is hashed on the device (it may never have been in host memory), once, and sets that share it
 * share the word. */
int32_t ngp_add_random_set_dense(ngp_handle *h, const int32_t *level, int64_t q, const double *K, ngp_handle *k_src, int32_t k_src_set,
                                 double df, double scale, double varU0, int32_t *set_id);

/* ---- single-step GBLUP (Aguilar et al. 2010; Christensen & Lund 2010): one breeding value per animal of the pedigree, precision
 *        H^-1 = A^-1 + [ 0 0 ; 0  G_w^-1 - A22^-1 ],   G_w = (1 - w) G + w A22,   A22 = A over the genotyped animals ----
 * H^-1 is sparse except for one n_g x n_g corner, so neither engine above fits: ngp_add_random_set_hybrid walks ONE Gauss-Seidel sweep
 * over a CSR S plus a dense block D on the LAST nd levels, K = S + embed(D) (the caller numbers the genotyped animals last).
 *
 * ngp_grm_single_step: after ngp_grm_end (G with the reference's + 0.001 ridge), in place of ngp_grm_invert; before ngp_grm_end or after
 * ngp_grm_invert: NGP_ERR_STATE.  A22 is N x N (ld >= N), host memory.  Forms G_w entry by entry in fp64, inverts G_w and A22 by the
 * rocSOLVER path of ngp_grm_invert (A22 in a second N^2 buffer, released on return) and leaves D = G_w^-1 - A22^-1 as the handle's matrix,
 * mirrored from the computed triangle: exactly symmetric; ngp_grm_get returns it.  NGP_ERR_ARG, with the matrix dropped and the handle
 * usable: w outside [0, 1), an A22 that is not finite or not exactly symmetric, G_w or A22 not positive definite.  G is not tuned to the
 * scale of A22 and there is no tau / omega scaling.
 *
 * ngp_add_random_set_hybrid: S is q x q CSR (columns ascending, symmetric, finite; k_col / k_val may be NULL when k_ptr[q] == 0); D is
 * nd x nd over the levels q - nd .. q - 1, 1 <= nd <= q, from ONE of
 *   D != NULL                   a host array of nd x nd doubles, exactly symmetric and finite (else NGP_ERR_ARG), copied;
 *   D == NULL, k_src != NULL    the block of HYBRID set k_src_set of another handle on the same device, by reference (that set's T,
 *                               below: chains = K hold one matrix; the caller gives the same S);
 *   D == NULL, k_src == NULL    this handle's own corner block (ngp_grm_single_step), taken over: the builder is empty afterwards.
 * Set-up: the entries of S with row and column both among the last nd levels are added into the block, T = D + S_tt (one sum per stored
 * entry), and leave the CSR; K_ll of a trailing level is T_ll; a K_ll that is not > 0 is NGP_ERR_ARG.  The head rows 0 .. q - nd - 1 get
 * the depths ngp_add_random_set gives them; ngp_set_random_schedule / ngp_get_random_schedule apply to the head (refused when nd == q).
 * One step: k_rand_levels for all q levels; the head rows through the serial or level-scheduled CSR engine (same bits under both); per
 * trailing row the seed sum_{c < hd} S_lc u_c with this sweep's head values; the blocked chain of the dense engine over T started from the
 * seed; u'Ku with the cross block counted exactly twice ("Hybrid random-effect sets": the normative orders).
 * nd == q with an empty S gives the bits of ngp_add_random_set_dense on D.  Everything ngp_add_random_set says about levels, df, scale,
 * varU0, draw keys, weighted residuals, ngp_get_random / ngp_set_random / ngp_sample_random_set, posterior sums, sample files and
 * snapshots holds; the model signature digests S as a CSR set does and T as a dense set does. */
int32_t ngp_grm_single_step(ngp_handle *h, const double *A22, int64_t ld, double w);
int32_t ngp_add_random_set_hybrid(ngp_handle *h, const int32_t *level, int64_t q, const int64_t *k_ptr, const int32_t *k_col, const double *k_val,
                                  int64_t nd, const double *D, ngp_handle *k_src, int32_t k_src_set, double df, double scale, double varU0,
                                  int32_t *set_id);
/* A handle with N records and NO genotype panel -- the canonical GBLUP model y ~ 1 + SNP(M1) with VCV M1 = Random("G", v) has no
 * marker set.  Takes the place of the panel call in the call sequence (a new model, like every ngp_set_panel_*; residual weights
 * before it).  On such a handle ngp_set_y, the residual prior, fixed-effect sets, random-effect sets of both engines, ngp_run,
 * ngp_run_many (side by side), sample files, snapshots, ngp_share_panel and the packed posterior work; ngp_add_marker_set*, ngp_sweep_set*
 * and ngp_profile_iteration are refused (NGP_ERR_STATE), and ngp_run requires a random-effect set.  Internally the handle carries ONE
 * inert block of 64 zero columns in place of the panel: state and file formats are those of a model with P = 64 and no marker set
 * (beta and its sums 64 zeros, delta 64 ones, no variance component), nothing is ever swept. */
int32_t ngp_set_records(ngp_handle *h, int64_t N);

/* BayesRCpi marker set -- annotation-informed BayesR, BayesRCπ(pi, class, v, annot) of the reference (set-up src/mme.jl:384-403, :493-516;
 * sampler src/functions.jl:291-360, :518-520, :536-544; output src/mme.jl:573-576, src/samplers.jl:85-87).  A annotations (annot:
 * ncol x A int32 entries 0 / 1, column-major with leading dimension ld), K variance classes vClass with probabilities pi (sum 1), ONE
 * variance per annotation (nVarCov = A, all starting at varBeta0), piHat[a] = pi for every annotation, annotProb[l, a] = annot[l, a] /
 * sum_a annot[l, a].  Limits: K >= 2, 1 <= A <= 8, A K <= 16.  NGP_ERR_ARG for a locus without an annotation (the reference divides
 * 0 / 0 there and throws in Categorical; its own comment says such loci belong in another set) and for entries other than 0 / 1.
 * Per sweep and locus: the annotation by one inverse-CDF uniform on the annotations' total weights, then the class inside it by the
 * search of BayesR (a fresh uniform per comparison), from log-weights log pi[a][v] - log(varc lhs) / 2 + log annotProb[l, a] taken
 * relative to their maximum ("BayesRCpi sets": the normative arithmetic, the draw keys and the departures from
 * the literal lines).  Behind the sweep: varBeta[a] = (scale df + sumS[a]) / chi2(df + nNonZero[a]); estPi: pi[a] ~ Dirichlet(nLoci[a, :]
 * + 1); and always annotProb[l, present] ~ Dirichlet(1 + [a == annotCat[l]]).  delta holds the class, annotCat the annotation of a
 * locus, both from 1.  In ngp_get_state / ngp_set_state / ngp_sweep_set the set has A variances; piHat is a [0.5, 0.5] placeholder
 * there (ngp_sweep_set takes piHat == NULL).  ngp_get_rc_state / ngp_set_rc_state carry the rest: piHat[A K] and sum_pi[A K]
 * (annotation-major; ngp_get_class_state sees the same A K words), annotProb[ncol A] and sum_annot[ncol A] (column-major, leading
 * dimension ncol), annotCat[ncol]; any pointer may be NULL.  sum_annot[l, a] counts the kept iterations with annotCat[l] = a + 1.  All
 * of it travels in the packed posterior (sums), sample records and snapshots (csrc/ngp_state.h).  Served by the persistent sweep
 * (fp32 and compact tiles, fp32 panels whose streamer workgroups own several shards included; kernels of its own) and the per-block
 * engine, also beside other methods in one 64-column block.  ngp_run_many fuses chains of such a model wherever it fuses chains of
 * any other (K chains per pass, above).  Time stamps and timing modes stay refused.  BayesRCplus is not on the device (one step per annotation on the same column,
 * src/functions.jl:362-419: a different block chain). */
int32_t ngp_add_marker_set_rc(ngp_handle *h, int64_t col0, int64_t ncol, double df, double scale, double varBeta0, const double *vClass,
                              const double *pi, int32_t K, const int32_t *annot, int64_t ld, int32_t A, int32_t estPi, const double *lhs0,
                              const double *rhs0, int32_t *set_id);
int32_t ngp_get_rc_state(ngp_handle *h, int32_t set_id, double *piHat, double *sum_pi, double *annotProb, int32_t *annotCat, double *sum_annot);
int32_t ngp_set_rc_state(ngp_handle *h, int32_t set_id, const double *piHat, const double *sum_pi, const double *annotProb, const int32_t *annotCat,
                         const double *sum_annot);

/* ---- prediction of new individuals: mean and SD of X_new beta over the kept draws ----
 * A prediction panel holds Np individuals x the training panel's P columns in the same column order, in the handle's storage (fp32
 * tiles filled from f64 / f32 / u8 input; under NGP_STORAGE_U8 the byte codes, from u8 input only).  It belongs to the shared panel
 * object: every handle that shares the training panel (ngp_share_panel, before or after) sees it, no second copy is made, and a new
 * training panel drops it together with every chain's prediction sums.  Upload as for the training panel: ngp_begin_prediction_panel,
 * then ngp_prediction_columns_* (any order, any boundaries; columns never written are zero columns), then ngp_end_prediction_panel;
 * between begin and end every other call on the handle is NGP_ERR_STATE.  centre != 0 subtracts the TRAINING panel's column means
 * (ngp_get_storage), never means of the prediction rows: fp32 tiles store (float)((double)v - mu_j) as the training tiles do, byte
 * tiles are centred analytically with the same mu_j.  Residual weights never scale prediction rows.  ngp_load_prediction_file reads
 * an NGPPNL01 file (8 or 2 bits) of P columns.
 * NGP_ERR_STATE: no finished training panel, a records-only (GBLUP) handle; NGP_ERR_ARG: columns outside [0, P), Np < 1, compact
 * storage given f64 / f32 input.  A refused call leaves a handle that still runs.
 *
 * From then on every KEPT iteration (the ones that accumulate the posterior sums, no others) is followed by one pass over the
 * prediction panel: for every marker set s over its own columns g_s(i) = sum_j x_ij beta_j, g(i) = sum_s g_s(i) in set order
 * (columns no set owns contribute nothing), accumulated in fp64 into sum[s][i] += g_s(i), sum2[s][i] += g_s(i)^2, s = 0 .. nsets with
 * row nsets the total.  The summation order is normative and fixed ("Prediction"): the result does not depend on
 * the grid, the device or the number of chains served by a launch.  In a fused ngp_run_many ONE launch per kept iteration serves
 * every chain whose marker sets lie on the same columns as the leader's, each chain bit for bit what it computes alone;
 * ngp_get_prediction_stats counts the launches a handle made and the chains they served (fused: the leader counts, the others 0).
 * The sums are zeroed by ngp_set_y.  A prediction panel loaded or replaced while a chain is under way starts the prediction sums of
 * that chain at zero (its next ngp_run sizes them for the new panel) while nKept goes on counting the chain's kept draws: the sums
 * then hold the kept draws since the panel came, fewer than nKept.  They are not part of snapshots, of the packed posterior or of
 * ngp_allreduce_posterior (formats unchanged): a host carries them beside a snapshot with ngp_get_prediction / ngp_set_prediction, and
 * pools chains itself.
 * Arrays are [nsets + 1][Np], row-major (row s contiguous).  nKept is the count ngp_get_posterior_sums reports.
 * ngp_get_prediction_last: g_s and g of the last kept draw.  ngp_get_prediction_layout: rows per shard R, shards S of the prediction
 * tiles, the chunk length in columns of the normative sum, and the rows of this handle's prediction arrays (nsets + 1; 0 while it
 * has no marker set); any pointer may be NULL. */
int32_t ngp_begin_prediction_panel(ngp_handle *h, int64_t Np);
int32_t ngp_prediction_columns_f64(ngp_handle *h, int64_t col0, const double *M, int64_t ncol, int64_t ld, int32_t centre);
int32_t ngp_prediction_columns_f32(ngp_handle *h, int64_t col0, const float *M, int64_t ncol, int64_t ld, int32_t centre);
int32_t ngp_prediction_columns_u8(ngp_handle *h, int64_t col0, const uint8_t *G, int64_t ncol, int64_t ld, int32_t centre);
/* Packed .bed columns of the candidates (arguments as ngp_panel_columns_bed, rows: NULL or Np indices).  What is subtracted is the
 * training mean, as above.  A missing call takes the training mean (MEAN: the tile value is exactly 0; needs centre != 0) or the
 * training mean rounded to a code, floor(mean + 0.5) in 0..2 (ROUND).  counts are over the prediction rows. */
int32_t ngp_prediction_columns_bed(ngp_handle *h, int64_t col0, const uint8_t *packed, int64_t ncol, int64_t stride, int64_t n_file,
                                   const int64_t *rows, int32_t allele, int32_t missing, int32_t centre, int64_t *counts);
int32_t ngp_end_prediction_panel(ngp_handle *h);
int32_t ngp_load_prediction_file(ngp_handle *h, const char *path, int32_t centre);
int32_t ngp_get_prediction_layout(ngp_handle *h, int64_t *Np, int64_t *R, int64_t *S, int64_t *chunk_cols, int64_t *rows);
int32_t ngp_get_prediction(ngp_handle *h, double *sum, double *sum2, int64_t rows, int64_t Np, int64_t *nKept);
int32_t ngp_set_prediction(ngp_handle *h, const double *sum, const double *sum2, int64_t rows, int64_t Np);
int32_t ngp_get_prediction_last(ngp_handle *h, double *out, int64_t rows, int64_t Np);
int32_t ngp_get_prediction_stats(ngp_handle *h, int64_t *launches, int64_t *chains_served);

/* ---- genomic variance of every kept draw: windows, marker sets, total, and the window posterior probability of association ----
 * Behind every KEPT iteration (and in no other) one pass over the training panel forms, over the N training individuals,
 * V_w = var_i sum_{j in w} x_ij beta_j for every window w, V_s for every marker set and V_g for all sets together (sample variance,
 * N - 1, clamped at 0), q = V / V_g (0 when V_g == 0), r = V_g / (V_g + varE) and the indicator [q > threshold].  The arithmetic is
 * normative ("Genomic variance"; tests/ref_genvar.py): the results do not depend on the layout of the tiles,
 * the engine, the chains of a fused launch or the device.
 * ngp_set_variance_windows: the windows of marker set set_id as half-open column ranges [start, stop) relative to the set's first
 * column (a Tuple set: relative to its span): ascending, disjoint, non-empty, inside the set; they need not cover it.  nwin = 0
 * drops the set's windows.  Legal any time after the set exists; zeroes this chain's variance sums.
 * ngp_enable_genomic_variance: on / off, the threshold in [0, 1], and the rows of the per-draw trace (0: none; draws beyond it are
 * counted, not stored).  Needs a finished panel; refused (NGP_ERR_STATE) on a records-only handle, with residual weights (the tiles
 * then hold row-scaled values whose variance is not var(X beta)), with N < 2 and with N > 2^18 (the head-room of the 64-bit
 * fixed-point sums is argued for 2^18 terms).  Enabling zeroes the sums.
 * Slots, in order: the windows of set 0, of set 1, ..., then one per set in set order, then the total: nslots = nwin_total + nsets + 1.
 * ngp_get_genomic_variance: sums over the kept draws per slot -- V, V^2, q, q^2, the count of q > threshold -- the last draw's V,
 * ratio[2] = sum r, sum r^2, and the number of draws in them (any pointer may be NULL); ngp_set_genomic_variance puts them back
 * (resume).  ngp_get_genomic_variance_trace: V [rows][nslots] and r [rows] of the first `traced` draws.
 * ngp_get_genomic_variance_stats: passes this handle launched and the chains they served; in a fused ngp_run_many ONE pass per kept
 * iteration serves every chain whose sets and windows equal the leader's (the leader counts, the others report 0).
 * The sums are zeroed wherever sum_beta is (ngp_set_y), dropped with a new panel or a change of the sets, and are not part of
 * snapshots, the packed posterior, sample records or ngp_allreduce_posterior: a host pools chains by adding their sums. */
int32_t ngp_set_variance_windows(ngp_handle *h, int32_t set_id, const int64_t *start, const int64_t *stop, int64_t nwin);
int32_t ngp_enable_genomic_variance(ngp_handle *h, int32_t on, double threshold, int64_t trace_rows);
int32_t ngp_get_genomic_variance_layout(ngp_handle *h, int64_t *nslots, int64_t *nwin_total, int64_t *nsets, int64_t *traced, int64_t *trace_dropped);
int32_t ngp_get_genomic_variance(ngp_handle *h, double *sumV, double *sumV2, double *sumQ, double *sumQ2, double *count, double *last, int64_t nslots,
                                 double *ratio, int64_t *nKept);
int32_t ngp_set_genomic_variance(ngp_handle *h, const double *sumV, const double *sumV2, const double *sumQ, const double *sumQ2, const double *count,
                                 const double *last, int64_t nslots, const double *ratio, int64_t nKept);
int32_t ngp_get_genomic_variance_trace(ngp_handle *h, double *V, double *ratio, int64_t rows, int64_t nslots);
int32_t ngp_get_genomic_variance_stats(ngp_handle *h, int64_t *launches, int64_t *chains_served);

/* ---- convergence diagnostics of every kept draw: mean, SD, effective sample size and Monte-Carlo standard error per parameter ----
 * Behind every KEPT iteration (and in no other) one element-wise pass updates a streaming lag-window autocovariance of every
 * monitored scalar; nothing is launched while the diagnostics are off.  The monitored vector theta[D] is the doubles of the sample
 * record in record order (csrc/ngp_state.h, diag_layout): varE | b | b_fixed | u, then varU of the random-effect sets | beta[P] |
 * varBeta | piHat[2] per marker set | class probabilities | per BayesLV set c[16], varZeta | the drawn thresholds t_2 .. t_{C-1}.
 * The arithmetic is normative ("Convergence diagnostics"; tests/ref_diag.py) and bit for bit the same alone
 * and in a fused ngp_run_many.  The ESS is Geyer's initial positive sequence estimator over the lags 0 .. lags-1.
 * ngp_enable_diagnostics: on / off, the window (lags even, 2 .. 256; 64 is the usual choice) and split: draws with index < split feed
 * half 0, the others half 1 (the halves are the sequences of a split-R-hat; a host pools chains).  Needs a model (a finished panel or
 * ngp_set_records); zeroes the state.  NGP_ERR_ARG for an odd lags or one out of range and for split < 0; NGP_ERR_NOMEM when the
 * (3 lags + 5) D doubles do not fit -- the diagnostics are then off and the handle runs on.  D follows the model until the first kept
 * draw; a model that changes afterwards makes ngp_run fail with NGP_ERR_STATE (enable again).
 * ngp_get_diagnostics_layout: D, lags, split, the draws taken and the words of the state image.
 * ngp_get_diagnostics: per parameter mean, sample variance, ESS, MCSE = sqrt(var / ESS), truncated (1: the positive sequence had not
 * ended inside the window -- the ESS is an upper bound; raise lags or thin more), and per half the number of draws half_n[2], the
 * means half_mean[2][D] and the variances half_var[2][D] (NaN below two draws).  Any pointer may be NULL; with no draw taken the call
 * returns NGP_OK, sets *n = 0 and leaves the arrays untouched.
 * ngp_get_diagnostics_state / ngp_set_diagnostics_state: the state as x1[D] | S1[2][D] | S2[2][D] | C[lags][D] | head[lags][D] |
 * ring[lags][D] with the draws taken, for resume beside a snapshot.  ngp_get_diagnostics_stats: updates this handle launched.
 * The state is zeroed wherever sum_beta is (ngp_set_y), dropped with a new panel, and is not part of snapshots, the packed
 * posterior, sample records or ngp_allreduce_posterior. */
int32_t ngp_enable_diagnostics(ngp_handle *h, int32_t on, int32_t lags, int64_t split);
int32_t ngp_get_diagnostics_layout(ngp_handle *h, int64_t *D, int32_t *lags, int64_t *split, int64_t *n, int64_t *state_words);
int32_t ngp_get_diagnostics(ngp_handle *h, double *mean, double *var, double *ess, double *mcse, double *truncated, double *half_n, double *half_mean,
                            double *half_var, int64_t D, int64_t *n);
int32_t ngp_get_diagnostics_state(ngp_handle *h, double *state, int64_t words, int64_t *n);
int32_t ngp_set_diagnostics_state(ngp_handle *h, const double *state, int64_t words, int64_t n);
int32_t ngp_get_diagnostics_stats(ngp_handle *h, int64_t *launches);
/* Timing hook of the diagnostics: device events around reps full-window updates (gather + update at draw indices >= lags, on a scratch
 * copy of the state: the chain's state and draw count stay what they are) and around reps finalise kernels over the chain's state;
 * milliseconds per launch (finalise: 0 while no draw is taken).  Allocates a second state for the call. */
int32_t ngp_debug_time_diagnostics(ngp_handle *h, int32_t reps, double *update_ms, double *finalise_ms);

/* ---- held-out records: missing phenotypes and cross-validation folds by data augmentation ----
 * A handle may carry a hold-out set H: m strictly increasing 0-based rows, 0 <= i < N, m < N.  A held-out record stays in the panel;
 * its phenotype is never read (ngp_set_y accepts NaN there and starts the record at the mean of the observed phenotypes) and is
 * redrawn at the head of every iteration of ngp_run / ngp_run_many from y_i | rest ~ N(fitted_i, varE / w_i): in the residual,
 * ycorr_i <- e_i ("Held-out records": the arithmetic and the draw keys are normative).  Every engine runs
 * unchanged, and K folds are K chains over one shared panel, each with its own mask (a sharer does not inherit the owner's).
 * In every KEPT iteration fit_i = yaug_i - ycorr_i, the whole linear predictor of the record (intercept, fixed, random and marker
 * terms), is accumulated: sum_fit[i] += fit, sum_fit2[i] += fit^2, n_fit[i] += 1; rows off H stay 0.
 * ngp_set_holdout: after the panel (or ngp_set_records / ngp_share_panel) and before ngp_set_y, NGP_ERR_STATE once y is set (a new
 * panel starts without a mask); NULL, 0 removes the mask; NGP_ERR_ARG for rows that are unsorted, repeated or out of range and for
 * m >= N.  ngp_get_holdout: rows[m], yaug[m], and the sums [N] each, n_fit as doubles (any pointer may be NULL);
 * ngp_set_holdout_state puts them back (resume).  ngp_get_holdout_layout: m (0 without a mask).
 * With a mask the packed posterior and snapshots carry the hold-out state (see ngp_posterior_len, ngp_save_snapshot; a snapshot is
 * refused by a handle with another mask or none); without one every format is byte for byte unchanged and nothing is launched.
 * The fine seam is not concerned: the caller owns ycorr there. */
int32_t ngp_set_holdout(ngp_handle *h, const int64_t *rows, int64_t m);
int32_t ngp_get_holdout(ngp_handle *h, int64_t *rows, double *yaug, double *sum_fit, double *sum_fit2, double *n_fit, int64_t m, int64_t N);
int32_t ngp_set_holdout_state(ngp_handle *h, const double *yaug, const double *sum_fit, const double *sum_fit2, const double *n_fit, int64_t m,
                              int64_t N);
int32_t ngp_get_holdout_layout(ngp_handle *h, int64_t *m);

/* ---- liability traits: binary and ordered classes (threshold / probit model), censored records (Tobit) ----
 * A record with a liability stays in the panel.  Its latent liability l_i is redrawn at the head of every iteration of ngp_run /
 * ngp_run_many from N(fitted_i, varE / w_i) truncated to the record's interval; in the residual, ycorr_i <- e_i, as for a held-out
 * record ("Liability traits": the truncated-normal sampler, the threshold draw, the start values and the draw
 * keys are normative).  Every engine runs unchanged.
 * ngp_set_liability_classes: cls[N] in 1..C, 2 <= C <= 8; class c means t_{c-1} < l <= t_c with t_0 = -inf, t_1 = 0, t_C = +inf, the
 *   thresholds between them drawn every iteration (C >= 3).  Entries of held-out rows are not read; every class needs a record that
 *   is not held out (NGP_ERR_ARG).  The residual variance is then held at 1 (the probit scale) and ngp_set_y reads y at no row.
 * ngp_set_liability_bounds: m strictly increasing rows, none held out, with lo < hi and at least one of them finite; ngp_set_y reads
 *   y off these rows only; varE is sampled as usual.
 * Both come after the panel (or ngp_set_records / ngp_share_panel) and the hold-out mask and before ngp_set_y (NGP_ERR_STATE once y
 * is set); they exclude one another (NGP_ERR_STATE); NULL, 0 removes either.  A failed call leaves the handle as it was.
 * ngp_get_liability_layout: m (0 without liabilities) and C (0 for bounds).  ngp_get_liability: rows[m], liab[m], and with classes
 *   thr, sum_thr, sum_thr2 of C - 1 entries each: the thresholds t_1 .. t_{C-1} and the sums of them and of their squares over kept
 *   iterations (any pointer may be NULL); ngp_set_liability_state puts them back (resume).
 * ngp_get_liability_stats: draws whose rejection loop ran out of its 256 rounds (they return the midpoint or the finite bound);
 *   0 in any sane chain.
 * ngp_fix_residual_variance: v > 0 holds varE = v from ngp_set_y on (no draw, the trace reports v), v = 0 returns to sampling; with
 *   classes only v = 1 is accepted.
 * With liabilities the packed posterior appends sum_thr | sum_thr2 (classes) and snapshots carry the liabilities and thresholds
 * (a snapshot is refused by a handle with other classes, other bounds or none); without them every format is byte for byte
 * unchanged and nothing is launched.  The fine seam is not concerned: the caller owns ycorr there. */
int32_t ngp_set_liability_classes(ngp_handle *h, const int32_t *cls, int32_t C);
int32_t ngp_set_liability_bounds(ngp_handle *h, const int64_t *rows, const double *lo, const double *hi, int64_t m);
int32_t ngp_get_liability_layout(ngp_handle *h, int64_t *m, int32_t *C);
int32_t ngp_get_liability(ngp_handle *h, int64_t *rows, double *liab, double *thr, double *sum_thr, double *sum_thr2, int64_t m, int32_t C);
int32_t ngp_set_liability_state(ngp_handle *h, const double *liab, const double *thr, const double *sum_thr, const double *sum_thr2, int64_t m,
                                int32_t C);
int32_t ngp_get_liability_stats(ngp_handle *h, int64_t *fallthrough);
int32_t ngp_fix_residual_variance(ngp_handle *h, double v);
/* Test probe of the truncated standard normal, beside ngp_draws_indexed: out[i] is the draw on the interval a[i] < z < b[i] (either
 * bound may be infinite) of stream (seed,chain,iter,kind,index0+i). */
int32_t ngp_tnormal_indexed(ngp_handle *h, uint64_t iter, uint64_t kind, uint64_t index0, const double *a, const double *b, int64_t n,
                            double *out);

/* ---- ordered traits on the scale of the trait: Cowles' threshold step, class probabilities of held-out records ----
 * Both are options of a handle with liability classes; without them nothing is launched and every format is byte for byte what it
 * was ("Normal distribution function", "Cowles' threshold step", "Class probabilities": normative).
 * ngp_set_threshold_step: mode 0 = Albert-Chib (the default: each threshold uniform between the liabilities of its two classes),
 *   mode 1 = Cowles (1996): one joint Metropolis-Hastings move of t_2 .. t_{C-1} per iteration, proposed from truncated normals of SD
 *   sigma around the current values and decided on the records' fitted values alone; the liabilities are redrawn behind it as before.
 *   sigma > 0 is a fixed proposal SD; sigma = 0 starts at 1 / sqrt(m) and follows the acceptance rate (target 0.44) in the iterations
 *   <= burnIn, fixed from then on.  After ngp_set_liability_classes (which puts the step back to mode 0) and before ngp_set_y:
 *   NGP_ERR_STATE without classes or once y is set, NGP_ERR_ARG for mode 1 with C < 3, a mode other than 0 / 1 or sigma < 0; a failed
 *   call changes nothing.
 * ngp_get_threshold_step: the mode, the SD in force (0 in mode 0) and the proposals made / taken since ngp_set_y (any pointer may be
 *   NULL); ngp_set_threshold_step_state puts the last three back (resume).
 * In mode 1 a snapshot appends sigma | tries | accepted and its signature names the mode: a handle in the other mode refuses it.
 * ngp_enable_class_probabilities: needs classes AND a hold-out mask, before ngp_set_y (NGP_ERR_STATE otherwise).  In every kept
 *   iteration p_c = Phi((t_c - fit) / sd) - Phi((t_{c-1} - fit) / sd) of every held-out record is added to sum_prob[c-1][k]; the
 *   number of draws is n_fit of ngp_get_holdout.  ngp_get_class_probabilities: sum_prob[C][m], class-major, rows in the order of the
 *   hold-out set; ngp_set_class_probabilities puts it back (resume).  The packed posterior and the snapshot body then end with
 *   sum_prob[C m]; ngp_allreduce_posterior pools it over chains that hold out the SAME records and refuses (NGP_ERR_ARG) chains whose
 *   masks differ, since the sums are laid out by position in the hold-out set (pool fold-chains on the host).  A snapshot is refused by a
 *   handle without the option, and the other way round.
 * ngp_debug_pnorm: test probe; which 0: out[i] = Phi(a[i]) (b may be NULL), 1: out[i] = log(Phi(b[i]) - Phi(a[i])), -inf unless
 *   a[i] < b[i]. */
int32_t ngp_set_threshold_step(ngp_handle *h, int32_t mode, double sigma);
int32_t ngp_get_threshold_step(ngp_handle *h, int32_t *mode, double *sigma, int64_t *tries, int64_t *accepted);
int32_t ngp_set_threshold_step_state(ngp_handle *h, double sigma, int64_t tries, int64_t accepted);
int32_t ngp_enable_class_probabilities(ngp_handle *h, int32_t on);
int32_t ngp_get_class_probabilities(ngp_handle *h, double *sum_prob, int64_t m, int32_t C);
int32_t ngp_set_class_probabilities(ngp_handle *h, const double *sum_prob, int64_t m, int32_t C);
int32_t ngp_debug_pnorm(ngp_handle *h, int32_t which, const double *a, const double *b, int64_t n, double *out);

#ifdef __cplusplus
}
#endif
#endif
