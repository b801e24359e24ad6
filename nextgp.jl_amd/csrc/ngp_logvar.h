// ngp_logvar.h -- gfx950 kernels of the variance model of one BayesLV marker set per iteration: the second half of sampleBayesLV!
// of the reference (src/functions.jl:442-485; set-up src/mme.jl:418-439).  The sweep of such a set is the BayesPR sweep with one
// variance per locus and runs in k_sweep unchanged; what is here replaces the region draw of BayesPR (k_regssq / k_regdraw).
// DESIGN.md "BayesLV sets" is the normative description of every summation order and draw key used here; tests/ref_logvar.py restates
// it operation by operation.  No FMA in the step itself (fp contract off, no __builtin_fma): every product and sum is rounded on its
// own; det_exp_any and det_log are the fixed sequences of ngp_rng.h.
//
// Per set and iteration, on the chain's stream, behind the sweep (launch_variance):
//   k_lv_slice    one 64-lane wave per 256 loci: the slice draw of every locus' variance (:448-468), logv = det_log(variance), the
//                 segment's trapped count and its partials of C'logv, one per covariate
//   k_lv_coef     ONE wave: rhsC = C'logv from the partials (segments ascending), meanC = iCpC rhsC, L = chol(iCpC varZeta),
//                 c = meanC + L z (:475-477), the trapped count of the iteration
//   k_lv_resid    zeta_l = logv_l - (C c)_l (:478) and, where varZeta is estimated, the segment partials of sum(x),
//                 x = zeta (mode 1) or logv (mode 2)
//   k_lv_reduce   stage 0 (ONE wave): mean = sum(x) / n from the partials      } only where varZeta is estimated (:481-485):
//   k_lv_ssq      segment partials of sum((x - mean)^2)                        } Julia's var, the two-pass form
//   k_lv_reduce   stage 1: varZeta = ss / (n - 1)  (mode 2: f * that)          }
#pragma once
#include "ngp_common.h"

#pragma clang fp contract(off)

#ifndef NGP_LV_MAXCOV
#define NGP_LV_MAXCOV 16  // (include/nextgp_hip.h)
#endif
// the small state of a set (doubles): c | varZeta | sum_c | sum_varZeta (posterior sums: entries 0..16 added to 17..33 on every kept
// iteration) | trapped count of the last iteration | mean (scratch between the two passes of var)
#define NGP_LV_C 0
#define NGP_LV_VZ 16
#define NGP_LV_SUM 17
#define NGP_LV_TRAP 34
#define NGP_LV_MEAN 35
#define NGP_LV_WORDS 40

namespace ngp {

// ------------------------------------------------------------------------------------------
// slice draw (src/functions.jl:448-468, taken literally, every operation rounded on its own, left to right as Julia parses it).
// 256 threads = 4 waves = 4 segments of 256 loci per workgroup; lane j of a segment's wave takes the loci j, j + 64, j + 128, j + 192
// of the segment (in that order), then the xor butterfly 32 .. 1 -- the pattern of k_regssq.  u1..u4 are four consecutive uniforms of
// ONE keyed stream (NGP_KIND_LV_UNIFORM, (set << 40) | locus).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_lv_slice(long long n, int ncov, const double *__restrict__ beta, double *__restrict__ vb,
                                                  const double *__restrict__ zeta, const double *__restrict__ Cm,
                                                  const double *__restrict__ st, double *__restrict__ logv, double *__restrict__ part,
                                                  int *__restrict__ trapseg, int set, uint64_t seed, uint64_t chain, uint64_t it,
                                                  const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;  // an earlier sweep of this call gave up (ngp_sweep_args.h, abort_w)
    const long long nseg = (n + 255) / 256;
    const long long sg = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (sg >= nseg) return;  // (uniform over the wave)
    const int lane = threadIdx.x & 63;
    const double varZeta = st[NGP_LV_VZ];
    const double m23 = -2.0 / 3.0;
    double lg[4];
    int trapped = 0;
#pragma unroll
    for (int m = 0; m < 4; m++) {
        const long long l = sg * 256 + lane + 64 * m;
        lg[m] = 0.0;
        if (l >= n) continue;
        double vari = vb[l];
        const double bi = beta[l], z = zeta[l];
        const double lv0 = det_log(vari);
        const double var_mui = lv0 - z;
        Rng r = rng_seed(seed, chain, it, NGP_KIND_LV_UNIFORM, ((uint64_t)set << 40) | (uint64_t)l);
        const double u1 = rng_uniform(r);
        const double u2 = rng_uniform(r);
        const double u3 = rng_uniform(r);
        const double u4 = rng_uniform(r);
        const double sv = det_sqrt(vari);
        const double v15 = vari * sv;
        const double p15 = 1.0 / v15;                 // vari^-1.5
        const double c1 = p15 * u1;
        const double hb = -0.5 * bi;
        const double hbb = hb * bi;                   // -0.5 bi bi
        const double a2 = hbb / vari;
        const double c2 = det_exp_any(a2) * u2;
        const double hz = -0.5 * z;
        const double hzz = hz * z;
        const double a3 = hzz / varZeta;
        const double c3 = det_exp_any(a3) * u3;
        const double m2v = -2.0 * varZeta;
        const double t3 = m2v * det_log(c3);
        const double temp = det_sqrt(t3);
        double lbound = det_exp_any(var_mui - temp);
        double rbound = det_exp_any(var_mui + temp);
        const double r2 = det_exp_any(m23 * det_log(c1));
        if (r2 < rbound) rbound = r2;
        const double l2 = hbb / det_log(c2);
        if (l2 > lbound) lbound = l2;
        if (lbound >= rbound) {
            trapped += 1;
        } else {
            const double d = rbound - lbound;
            const double t = u4 * d;
            vari = lbound + t;
            vb[l] = vari;
        }
        const double lgv = det_log(vari);             // logVar == det_log(varBeta) at all times
        logv[l] = lgv;
        lg[m] = lgv;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) trapped = trapped + __shfl_xor(trapped, off);
    if (lane == 0) trapseg[sg] = trapped;
    for (int k = 0; k < ncov; k++) {
        const double *Ck = Cm + (size_t)k * (size_t)n;
        double a = 0.0;
#pragma unroll
        for (int m = 0; m < 4; m++) {
            const long long l = sg * 256 + lane + 64 * m;
            if (l < n) {
                const double t = Ck[l] * lg[m];
                a = a + t;
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) a = a + __shfl_xor(a, off);
        if (lane == 0) part[(size_t)k * (size_t)nseg + (size_t)sg] = a;
    }
}

// the partials p[0 .. nseg) added in ascending order from p[0]; the loads of 32 go out together (k_regdraw)
__device__ inline double lv_sum_partials(const double *__restrict__ p, long long nseg) {
    double tot = p[0];
    long long sg = 1;
    for (; sg + 32 <= nseg; sg += 32) {
        double v[32];
#pragma unroll
        for (int i = 0; i < 32; i++) v[i] = p[sg + i];
#pragma unroll
        for (int i = 0; i < 32; i++) tot = tot + v[i];
    }
    for (; sg < nseg; sg++) tot = tot + p[sg];
    return tot;
}

// ------------------------------------------------------------------------------------------
// regression coefficients of the log-variances, ONE workgroup of one wave.  Lane k < ncov sums column k's partials and draws z_k
// (NGP_KIND_LV_NORMAL, (set << 40) | k); lane 0 then does, every product and sum rounded, sums from 0.0 with ascending index:
//   meanC_i = sum_j iCpC[i][j] rhsC_j;   S[i][j] = iCpC[i][j] varZeta;   L = lower Cholesky of S, row by row:
//   s = S[i][j] - sum_{k < j} L[i][k] L[j][k] (one subtraction per k);  L[i][i] = sqrt(s), L[i][j] = s / L[j][j]
//   c_i = meanC_i + sum_{j <= i} L[i][j] z_j
// A pivot that is not positive makes every c a NaN (the chain is poisoned visibly); nothing here can loop.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_lv_coef(long long n, int ncov, const double *__restrict__ iCpC, const double *__restrict__ part,
                                                const int *__restrict__ trapseg, double *__restrict__ st, int set, uint64_t seed,
                                                uint64_t chain, uint64_t it, const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    __shared__ double rhsC[NGP_LV_MAXCOV], zz[NGP_LV_MAXCOV], L[NGP_LV_MAXCOV * NGP_LV_MAXCOV];
    const long long nseg = (n + 255) / 256;
    const int tid = threadIdx.x;
    if (tid < ncov) {
        rhsC[tid] = lv_sum_partials(part + (size_t)tid * (size_t)nseg, nseg);
        Rng r = rng_seed(seed, chain, it, NGP_KIND_LV_NORMAL, ((uint64_t)set << 40) | (uint64_t)tid);
        zz[tid] = rng_normal(r);
    }
    if (tid == 63) {  // trapped loci of this iteration
        long long tr = 0;
        for (long long sg = 0; sg < nseg; sg++) tr += trapseg[sg];
        st[NGP_LV_TRAP] = (double)tr;
    }
    __syncthreads();
    if (tid != 0) return;
    const double varZeta = st[NGP_LV_VZ];
    bool bad = false;
    for (int i = 0; i < ncov; i++)
        for (int j = 0; j <= i; j++) {
            double s = iCpC[i * ncov + j] * varZeta;
            for (int k = 0; k < j; k++) {
                const double t = L[i * ncov + k] * L[j * ncov + k];
                s = s - t;
            }
            if (i == j) {
                if (!(s > 0.0)) bad = true;
                L[i * ncov + i] = det_sqrt(s);
            } else {
                L[i * ncov + j] = s / L[j * ncov + j];
            }
        }
    for (int i = 0; i < ncov; i++) {
        double mean = 0.0;
        for (int j = 0; j < ncov; j++) {
            const double t = iCpC[i * ncov + j] * rhsC[j];
            mean = mean + t;
        }
        double acc = 0.0;
        for (int j = 0; j <= i; j++) {
            const double t = L[i * ncov + j] * zz[j];
            acc = acc + t;
        }
        st[NGP_LV_C + i] = bad ? __builtin_nan("") : mean + acc;
    }
}

// ------------------------------------------------------------------------------------------
// zeta_l = logv_l - fit_l, fit_l = sum_k C[l][k] c_k (from 0.0, ascending k, every product and sum rounded); est_mode 1 / 2: the
// segment partials of sum(x), x = zeta / logv, in the segment pattern of k_lv_slice
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_lv_resid(long long n, int ncov, const double *__restrict__ Cm, const double *__restrict__ st,
                                                  const double *__restrict__ logv, double *__restrict__ zeta, int est_mode,
                                                  double *__restrict__ vpart, const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    const long long nseg = (n + 255) / 256;
    const long long sg = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (sg >= nseg) return;
    const int lane = threadIdx.x & 63;
    double a = 0.0;
#pragma unroll
    for (int m = 0; m < 4; m++) {
        const long long l = sg * 256 + lane + 64 * m;
        if (l >= n) continue;
        double fit = 0.0;
        for (int k = 0; k < ncov; k++) {
            const double t = Cm[(size_t)k * (size_t)n + (size_t)l] * st[NGP_LV_C + k];
            fit = fit + t;
        }
        const double lgv = logv[l];
        const double z = lgv - fit;
        zeta[l] = z;
        a = a + (est_mode == 1 ? z : lgv);
    }
    if (est_mode == 0) return;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) a = a + __shfl_xor(a, off);
    if (lane == 0) vpart[sg] = a;
}

// segment partials of sum((x - mean)^2): d = x - mean; q = d d; a = a + q (lane order, then the butterfly)
__global__ __launch_bounds__(256) void k_lv_ssq(long long n, const double *__restrict__ x, const double *__restrict__ st,
                                                double *__restrict__ vpart, const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    const long long nseg = (n + 255) / 256;
    const long long sg = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (sg >= nseg) return;
    const int lane = threadIdx.x & 63;
    const double mean = st[NGP_LV_MEAN];
    double a = 0.0;
#pragma unroll
    for (int m = 0; m < 4; m++) {
        const long long l = sg * 256 + lane + 64 * m;
        if (l < n) {
            const double d = x[l] - mean;
            const double q = d * d;
            a = a + q;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) a = a + __shfl_xor(a, off);
    if (lane == 0) vpart[sg] = a;
}

// ONE wave, lane 0: the partials in ascending order; stage 0: mean = sum / n; stage 1: v = ss / (n - 1), varZeta = v (est_mode 1) or
// frac * v (est_mode 2)
__global__ __launch_bounds__(64) void k_lv_reduce(long long n, int stage, int est_mode, double frac, const double *__restrict__ vpart,
                                                  double *__restrict__ st, const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    if (threadIdx.x != 0) return;
    const double tot = lv_sum_partials(vpart, (n + 255) / 256);
    if (stage == 0) {
        st[NGP_LV_MEAN] = tot / (double)n;
    } else {
        const double v = tot / (double)(n - 1);
        st[NGP_LV_VZ] = (est_mode == 2) ? frac * v : v;
    }
}

// keyed start of zeta (zeta0 == NULL): uniforms of NGP_KIND_LV_START, iteration 0, (set << 40) | locus
__global__ __launch_bounds__(256) void k_lv_start(long long n, double *__restrict__ zeta, int set, uint64_t seed, uint64_t chain) {
    const long long l = (long long)blockIdx.x * 256 + threadIdx.x;
    if (l >= n) return;
    Rng r = rng_seed(seed, chain, 0, NGP_KIND_LV_START, ((uint64_t)set << 40) | (uint64_t)l);
    zeta[l] = rng_uniform(r);
}

}  // namespace ngp
