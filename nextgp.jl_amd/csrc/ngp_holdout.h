// Held-out records by data augmentation ("Held-out records").  A held-out record stays in the panel; at the head
// of every iteration its phenotype is redrawn from its conditional, y_i | rest ~ N(fitted_i, varE / w_i), which in the residual is one
// line: ycorr_i <- e_i.  Two kernels outside the sweep's translation units, one held-out row per lane: plain loads and stores only.
//
//   rows[m]   the held-out rows, strictly increasing;  yaug[m]  the augmented phenotype of each
//   ycorr     the residual as it lies on the device (with residual weights the scaled residual s_i ycorr_i; rs = the row scales, else null)
//   r_i       the residual of row i as ngp_get_state gives it: ycorr_i, with weights ycorr_i / s_i (the operation of k_row_descale)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ngp_common.h"
#include "ngp_rng.h"

#pragma clang fp contract(off)

namespace ngp {

// head of an iteration, in front of k_head: e = sqrt(varE) z with z the normal of stream (seed, chain, iter, NGP_KIND_AUGMENT, row);
// yaug = (yaug - r) + e', the device word of the row becomes e.  varE == 0 (the first iteration of a fresh chain): nothing is touched.
__global__ __launch_bounds__(256) void k_holdout_augment(const long long *__restrict__ rows, long long m, double *__restrict__ ycorr,
                                                         double *__restrict__ yaug, const double *__restrict__ rs, const DScal *__restrict__ sc,
                                                         uint64_t seed, uint64_t chain, uint64_t iter, const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;  // an earlier sweep of this call gave up (ngp_sweep_args.h, abort_w)
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= m) return;
    const double varE = sc->varE;
    if (varE == 0.0) return;
    const long long i = rows[k];
    Rng r = rng_seed(seed, chain, iter, NGP_KIND_AUGMENT, (uint64_t)i);
    const double z = rng_normal(r);
    const double e = det_sqrt(varE) * z;
    const double yt = ycorr[i];
    const double ri = rs ? yt / rs[i] : yt;
    const double ep = rs ? e / rs[i] : e;
    const double fit = yaug[k] - ri;
    yaug[k] = fit + ep;
    ycorr[i] = e;
}

// kept iteration, beside k_post: the whole linear predictor of every held-out record (intercept, fixed, random and marker terms)
__global__ __launch_bounds__(256) void k_holdout_accum(const long long *__restrict__ rows, long long m, const double *__restrict__ ycorr,
                                                       const double *__restrict__ yaug, const double *__restrict__ rs, double *__restrict__ sum_fit,
                                                       double *__restrict__ sum_fit2, double *__restrict__ n_fit, const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= m) return;
    const long long i = rows[k];
    const double yt = ycorr[i];
    const double ri = rs ? yt / rs[i] : yt;
    const double fit = yaug[k] - ri;
    sum_fit[i] = sum_fit[i] + fit;
    sum_fit2[i] = sum_fit2[i] + fit * fit;
    n_fit[i] = n_fit[i] + 1.0;
}

}  // namespace ngp
