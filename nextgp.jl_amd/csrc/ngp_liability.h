// Liability traits by data augmentation ("Liability traits"): binary and ordered classes (threshold / probit
// model) and censored records (Tobit).  An augmented record stays in the panel; at the head of every iteration its latent liability
// is redrawn from its conditional, a normal N(fitted_i, varE / w_i) truncated to the record's interval, which in the residual is the
// one line of ngp_holdout.h: ycorr_i <- e_i.  Kernels outside the sweep's translation units, plain loads and stores only.
//
//   A[m]      the augmented rows, strictly increasing;  liab[m]  the current liability of each
//   lo, hi    the interval of each row (censored records), or cls[m] in 1..C with thr[0..C]: thr[0] = -inf, thr[1] = 0, thr[C] = +inf,
//             class c means thr[c-1] < l <= thr[c]
//   ycorr, rs, r_i   as in ngp_holdout.h
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ngp_common.h"
#include "ngp_rng.h"

#pragma clang fp contract(off)

#define NGP_TN_ROUNDS 256   // bound of every rejection loop of rng_tnormal
#define NGP_LIAB_MAXC 8     // classes of a threshold trait

namespace ngp {

// ---- truncated standard normal (Robert 1995), a fixed sequence of IEEE operations; every round takes its uniforms in the order written ----

// z > a by rejection from the normal (a < 0: at least every second draw is taken)
__device__ inline bool tn_normal_above(Rng &r, double a, double &z) {
    for (int k = 0; k < NGP_TN_ROUNDS; k++) {
        const double x = ppnd16(rng_uniform(r));
        if (x > a) { z = x; return true; }
    }
    return false;
}

// a >= 0: translated exponential proposal x = a - log(u1) / alpha, alpha = (a + sqrt(a^2 + 4)) / 2, taken when
// u2 <= exp(-(x - alpha)^2 / 2) and x <= b (b = +inf: the one-sided tail)
__device__ inline bool tn_tail(Rng &r, double a, double b, double &z) {
    const double aa = a * a;
    const double s = det_sqrt(aa + 4.0);
    const double alpha = (a + s) / 2.0;
    for (int k = 0; k < NGP_TN_ROUNDS; k++) {
        const double u1 = rng_uniform(r);
        const double u2 = rng_uniform(r);
        const double lg = det_log(u1);
        const double x = a - lg / alpha;
        const double d = x - alpha;
        const double q = -(d * d) / 2.0;
        const double rho = det_exp(q);
        if (x <= b && u2 <= rho) { z = x; return true; }
    }
    return false;
}

// (a, +inf), a of either sign
__device__ inline bool tn_above(Rng &r, double a, double &z) {
    if (a < 0.0) return tn_normal_above(r, a, z);
    return tn_tail(r, a, __builtin_huge_val(), z);
}

// uniform proposal x = a + (b - a) u1, taken when u2 <= exp((m2 - x^2) / 2): m2 = a^2 for 0 <= a, 0 for a < 0 < b
__device__ inline bool tn_uniform(Rng &r, double a, double b, double m2, double &z) {
    const double w = b - a;
    for (int k = 0; k < NGP_TN_ROUNDS; k++) {
        const double u1 = rng_uniform(r);
        const double u2 = rng_uniform(r);
        const double x = a + w * u1;
        const double q = (m2 - x * x) / 2.0;
        const double rho = det_exp(q);
        if (u2 <= rho) { z = x; return true; }
    }
    return false;
}

// 0 <= a < b < +inf.  The switch between the two proposals: b <= a + 2 sqrt(e) / (a + sqrt(a^2 + 4)) exp((a^2 - a sqrt(a^2 + 4)) / 4)
__device__ inline bool tn_between_pos(Rng &r, double a, double b, double &z) {
    const double aa = a * a;
    const double s = det_sqrt(aa + 4.0);
    const double t = a * s;
    const double d = aa - t;
    const double q = d / 4.0;
    const double ex = det_exp(q);
    const double den = a + s;
    const double c = 3.2974425414002564 / den;  // 2 sqrt(e)
    const double w = c * ex;
    const double lim = a + w;
    if (b <= lim) return tn_uniform(r, a, b, aa, z);
    return tn_tail(r, a, b, z);
}

// z from N(0, 1) restricted to (a, b), a < b, either bound possibly infinite.  A lane whose loop runs out (or whose bounds are not
// a < b: a NaN from a poisoned chain compares false everywhere) returns the midpoint, the finite bound or 0 and counts one in *fall.
__device__ inline double rng_tnormal(Rng &r, double a, double b, unsigned long long *fall) {
    const double inf = __builtin_huge_val();
    double z = 0.0;
    bool ok = false;
    if (a < b) {
        if (b == inf) ok = tn_above(r, a, z);
        else if (a == -inf) { ok = tn_above(r, -b, z); z = -z; }
        else if (a >= 0.0) ok = tn_between_pos(r, a, b, z);
        else if (b <= 0.0) { ok = tn_between_pos(r, -b, -a, z); z = -z; }
        else if (b - a <= 2.5066282746310002) ok = tn_uniform(r, a, b, 0.0, z);  // sqrt(2 pi)
        else {
            for (int k = 0; k < NGP_TN_ROUNDS && !ok; k++) {
                const double x = ppnd16(rng_uniform(r));
                if (x > a && x < b) { z = x; ok = true; }
            }
        }
    }
    if (ok) return z;
    if (fall) atomicAdd(fall, 1ull);
    const bool fa = a > -inf && a < inf, fb = b > -inf && b < inf;
    if (fa && fb) return a + (b - a) / 2.0;
    return fa ? a : (fb ? b : 0.0);
}

// probe (ngp_tnormal_indexed): draw i from stream (seed, chain, iter, kind, index0 + i) with the bounds (a[i], b[i])
__global__ __launch_bounds__(256) void k_tnormal_indexed(uint64_t seed, uint64_t chain, uint64_t it, uint64_t kind, uint64_t index0,
                                                         const double *__restrict__ a, const double *__restrict__ b, long long n,
                                                         double *__restrict__ out, unsigned long long *__restrict__ fall) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    Rng r = rng_seed(seed, chain, it, kind, index0 + (uint64_t)i);
    out[i] = rng_tnormal(r, a[i], b[i], fall);
}

// Thresholds of C >= 3 classes (Albert & Chib 1993), first in the iteration: ONE workgroup of 1024 threads.  Per class the minimum
// and maximum liability (order-free: any reduction tree gives the same bits), then thread 0 draws for c = 2 .. C-1 in order
// thr[c] = lower + u (upper - lower), lower = max(thr[c-1] (new), max liab of class c), upper = min(thr[c+1] (old), min liab of class
// c+1), u the uniform of stream (seed, chain, iter, NGP_KIND_THRESHOLD, c).  kept: sum_thr[c] += thr[c], sum_thr2[c] += thr[c]^2
// (both of C+1 entries, used at 2 .. C-1).
__global__ __launch_bounds__(1024) void k_thresholds(const int *__restrict__ cls, const double *__restrict__ liab, long long m, int C,
                                                     double *__restrict__ thr, double *__restrict__ sum_thr, double *__restrict__ sum_thr2,
                                                     int kept, uint64_t seed, uint64_t chain, uint64_t iter,
                                                     const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    __shared__ double wmn[16][NGP_LIAB_MAXC], wmx[16][NGP_LIAB_MAXC];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const double inf = __builtin_huge_val();
    double mn[NGP_LIAB_MAXC], mx[NGP_LIAB_MAXC];
#pragma unroll
    for (int c = 0; c < NGP_LIAB_MAXC; c++) { mn[c] = inf; mx[c] = -inf; }
    for (long long k = tid; k < m; k += 1024) {
        const int cc = cls[k] - 1;
        const double l = liab[k];
#pragma unroll
        for (int c = 0; c < NGP_LIAB_MAXC; c++) {
            mn[c] = (cc == c && l < mn[c]) ? l : mn[c];
            mx[c] = (cc == c && l > mx[c]) ? l : mx[c];
        }
    }
#pragma unroll
    for (int c = 0; c < NGP_LIAB_MAXC; c++) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double on = __shfl_xor(mn[c], off), ox = __shfl_xor(mx[c], off);
            mn[c] = on < mn[c] ? on : mn[c];
            mx[c] = ox > mx[c] ? ox : mx[c];
        }
        if (lane == 0) { wmn[wv][c] = mn[c]; wmx[wv][c] = mx[c]; }
    }
    __syncthreads();
    if (tid != 0) return;
    for (int c = 2; c <= C - 1; c++) {
        double cmx = wmx[0][c - 1], cmn = wmn[0][c];  // max of class c, min of class c+1
        for (int w = 1; w < 16; w++) {
            cmx = wmx[w][c - 1] > cmx ? wmx[w][c - 1] : cmx;
            cmn = wmn[w][c] < cmn ? wmn[w][c] : cmn;
        }
        const double tl = thr[c - 1], tu = thr[c + 1];
        const double lower = cmx > tl ? cmx : tl;
        const double upper = cmn < tu ? cmn : tu;
        Rng r = rng_seed(seed, chain, iter, NGP_KIND_THRESHOLD, (uint64_t)c);
        const double u = rng_uniform(r);
        const double wd = upper - lower;
        const double t = lower + u * wd;
        thr[c] = t;
        if (kept) {
            sum_thr[c] = sum_thr[c] + t;
            sum_thr2[c] = sum_thr2[c] + t * t;
        }
    }
}

// head of an iteration, in front of k_head, one augmented row per lane: fit = liab - r, sd = sqrt(varE) (/ s_i), a = (lo - fit) / sd,
// b = (hi - fit) / sd, z the truncated normal of stream (seed, chain, iter, NGP_KIND_LIABILITY, row), e = sqrt(varE) z;
// liab = fit + e', the device word of the row becomes e.  varE == 0 (the first iteration of a fresh censored chain): nothing is touched.
// The result is not clamped: a liability that rounds onto its bound is a draw of the closed interval.
__global__ __launch_bounds__(256) void k_liability_augment(const long long *__restrict__ rows, long long m, double *__restrict__ ycorr,
                                                           double *__restrict__ liab, const double *__restrict__ lo,
                                                           const double *__restrict__ hi, const int *__restrict__ cls,
                                                           const double *__restrict__ thr, const double *__restrict__ rs,
                                                           const DScal *__restrict__ sc, uint64_t seed, uint64_t chain, uint64_t iter,
                                                           unsigned long long *__restrict__ fall, const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;  // an earlier sweep of this call gave up (ngp_sweep_args.h, abort_w)
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= m) return;
    const double varE = sc->varE;
    if (varE == 0.0) return;
    const long long i = rows[k];
    const double yt = ycorr[i];
    const double ri = rs ? yt / rs[i] : yt;
    const double fit = liab[k] - ri;
    const double sde = det_sqrt(varE);
    const double sd = rs ? sde / rs[i] : sde;
    double l0, l1;
    if (cls) {
        const int c = cls[k];
        l0 = thr[c - 1];
        l1 = thr[c];
    } else {
        l0 = lo[k];
        l1 = hi[k];
    }
    const double a = (l0 - fit) / sd;
    const double b = (l1 - fit) / sd;
    Rng r = rng_seed(seed, chain, iter, NGP_KIND_LIABILITY, (uint64_t)i);
    const double z = rng_tnormal(r, a, b, fall);
    const double e = sde * z;
    const double ep = rs ? e / rs[i] : e;
    liab[k] = fit + ep;
    ycorr[i] = e;
}

}  // namespace ngp
