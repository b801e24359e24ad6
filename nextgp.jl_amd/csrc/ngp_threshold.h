// Ordered traits on the scale of the trait ("Cowles' threshold step" and "Class probabilities"): the joint
// Metropolis-Hastings move of the thresholds of C >= 3 classes (Cowles 1996), which takes the place of k_thresholds where
// ngp_set_threshold_step asks for it, and the class probabilities of the held-out records per kept draw.  Kernels outside the sweep's
// translation units: plain loads and stores, no floating-point atomics, every reduction a fixed tree.
//
//   thr[0..C]   thr[0] = -inf, thr[1] = 0, thr[C] = +inf, followed by sum_thr[C+1] and sum_thr2[C+1] (ngp_liability.h)
//   g[0..C]     the proposal in the same form, g[C+1] = 1.0 where it is strictly ordered, else 0.0
//   A[m], cls, liab, ycorr, rs, r_i   as in ngp_liability.h
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ngp_common.h"
#include "ngp_liability.h"
#include "ngp_pnorm.h"
#include "ngp_rng.h"

#pragma clang fp contract(off)

#define NGP_KIND_THRESHOLD_MH 24  // Cowles' step: the truncated normal of threshold c (index c = 2 .. C-1), the uniform of the decision (index 1)
#define NGP_THR_WG 1024           // rows of one workgroup of k_threshold_terms
#define NGP_THR_TARGET 0.44       // acceptance rate the adaptation aims at
#define NGP_THR_LS_MIN (-20.0)    // bounds of log sigma under adaptation
#define NGP_THR_LS_MAX 0.0

namespace ngp {

// the step's words on the device: the proposal SD, and the proposals made and taken since the chain began
struct ThrStep {
    double sigma;
    long long tries, accepted;
};

// Proposal and likelihood terms.  Workgroup w owns rows 1024 w .. 1024 w + 1023 of A.  Thread 0 of EVERY workgroup forms the same
// proposal (the draws are keyed, not shared): for c = 2 .. C-1 in order g_c = t_c + sigma z, z the truncated normal on
// ((g_{c-1} - t_c) / sigma, (t_{c+1} - t_c) / sigma) of stream (seed, chain, iter, NGP_KIND_THRESHOLD_MH, c); it is in order when
// g_{c-1} < g_c < t_{c+1} for every c.  Workgroup 0 writes g (and counts a draw that ran out of rounds).  A proposal out of order ends
// the kernel there.  Else per row, with fit and sd as k_liability_augment forms them and c the row's class,
//   term = det_lpdiff((g_{c-1} - fit) / sd, (g_c - fit) / sd) - det_lpdiff((t_{c-1} - fit) / sd, (t_c - fit) / sd),
// exactly 0.0 where both thresholds of the class are unchanged (and on the rows past m); per wave the butterfly 32 .. 1, then thread 0
// adds the 16 wave sums in index order into part[w].
__global__ __launch_bounds__(NGP_THR_WG) void k_threshold_terms(const long long *__restrict__ rows, const int *__restrict__ cls,
                                                                const double *__restrict__ liab, long long m, int C,
                                                                const double *__restrict__ ycorr, const double *__restrict__ rs,
                                                                const DScal *__restrict__ sc, const double *__restrict__ thr,
                                                                const ThrStep *__restrict__ ts, double *__restrict__ g_out,
                                                                double *__restrict__ part, uint64_t seed, uint64_t chain, uint64_t iter,
                                                                unsigned long long *__restrict__ fall, const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    __shared__ double st[NGP_LIAB_MAXC + 1], sg[NGP_LIAB_MAXC + 1], wsum[NGP_THR_WG / 64];
    __shared__ int s_ok;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    if (tid == 0) {
        const double sigma = ts->sigma;
        for (int c = 0; c <= C; c++) { st[c] = thr[c]; sg[c] = thr[c]; }
        bool ok = true;
        for (int c = 2; c <= C - 1; c++) {
            const double a = (sg[c - 1] - st[c]) / sigma;
            const double b = (st[c + 1] - st[c]) / sigma;
            Rng r = rng_seed(seed, chain, iter, NGP_KIND_THRESHOLD_MH, (uint64_t)c);
            const double z = rng_tnormal(r, a, b, blockIdx.x == 0 ? fall : nullptr);
            const double gc = st[c] + sigma * z;
            sg[c] = gc;
            ok = ok && (sg[c - 1] < gc) && (gc < st[c + 1]);
        }
        s_ok = ok ? 1 : 0;
        if (blockIdx.x == 0) {
            for (int c = 0; c <= C; c++) g_out[c] = sg[c];
            g_out[C + 1] = ok ? 1.0 : 0.0;
        }
    }
    __syncthreads();
    if (!s_ok) return;
    const long long k = (long long)blockIdx.x * NGP_THR_WG + tid;
    double term = 0.0;
    if (k < m) {
        const int c = cls[k];
        const double t0 = st[c - 1], t1 = st[c], g0 = sg[c - 1], g1 = sg[c];
        if (!(g0 == t0 && g1 == t1)) {
            const long long i = rows[k];
            const double yt = ycorr[i];
            const double ri = rs ? yt / rs[i] : yt;
            const double fit = liab[k] - ri;
            const double sde = det_sqrt(sc->varE);
            const double sd = rs ? sde / rs[i] : sde;
            const double ln = det_lpdiff((g0 - fit) / sd, (g1 - fit) / sd);
            const double lo = det_lpdiff((t0 - fit) / sd, (t1 - fit) / sd);
            term = ln - lo;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) term = term + __shfl_xor(term, off);
    if (lane == 0) wsum[wv] = term;
    __syncthreads();
    if (tid != 0) return;
    double s = wsum[0];
    for (int w = 1; w < NGP_THR_WG / 64; w++) s = s + wsum[w];
    part[blockIdx.x] = s;
}

// Decision, one workgroup, thread 0: S = sum of part[0 .. nwg) in index order, plus the proposal's correction
//   sum_{c=2}^{C-1} [ det_lpdiff((g_{c-1} - t_c) / sigma, (t_{c+1} - t_c) / sigma) - det_lpdiff((t_{c-1} - g_c) / sigma, (g_{c+1} - g_c) / sigma) ];
// taken iff det_log(u) < S + correction, u the first uniform of stream (seed, chain, iter, NGP_KIND_THRESHOLD_MH, 1) -- a NaN on
// either side compares false and rejects.  tries += 1, accepted += 1 when taken; kept: sum_thr[c] += t_c, sum_thr2[c] += t_c^2 as
// k_thresholds adds them; adapt: log sigma += (taken - NGP_THR_TARGET) / sqrt(tries), held inside [NGP_THR_LS_MIN, NGP_THR_LS_MAX].
__global__ __launch_bounds__(64) void k_threshold_decide(int C, double *__restrict__ thr, double *__restrict__ sum_thr,
                                                         double *__restrict__ sum_thr2, const double *__restrict__ g,
                                                         const double *__restrict__ part, int nwg, ThrStep *__restrict__ ts, int kept,
                                                         int adapt, uint64_t seed, uint64_t chain, uint64_t iter,
                                                         const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    if (threadIdx.x != 0) return;
    const double sigma = ts->sigma;
    bool take = false;
    if (g[C + 1] != 0.0) {
        double s = part[0];
        for (int w = 1; w < nwg; w++) s = s + part[w];
        double corr = 0.0;
        for (int c = 2; c <= C - 1; c++) {
            const double fwd = det_lpdiff((g[c - 1] - thr[c]) / sigma, (thr[c + 1] - thr[c]) / sigma);
            const double rev = det_lpdiff((thr[c - 1] - g[c]) / sigma, (g[c + 1] - g[c]) / sigma);
            corr = corr + (fwd - rev);
        }
        const double L = s + corr;
        Rng r = rng_seed(seed, chain, iter, NGP_KIND_THRESHOLD_MH, 1);
        const double lu = det_log(rng_uniform(r));
        take = lu < L;
    }
    if (take)
        for (int c = 2; c <= C - 1; c++) thr[c] = g[c];
    const long long n = ts->tries + 1;
    ts->tries = n;
    if (take) ts->accepted = ts->accepted + 1;
    if (kept)
        for (int c = 2; c <= C - 1; c++) {
            const double t = thr[c];
            sum_thr[c] = sum_thr[c] + t;
            sum_thr2[c] = sum_thr2[c] + t * t;
        }
    if (adapt) {
        double ls = det_log(sigma);
        const double gain = 1.0 / det_sqrt((double)n);
        const double d = (take ? 1.0 : 0.0) - NGP_THR_TARGET;
        ls = ls + gain * d;
        ls = ls < NGP_THR_LS_MIN ? NGP_THR_LS_MIN : ls;
        ls = ls > NGP_THR_LS_MAX ? NGP_THR_LS_MAX : ls;
        ts->sigma = det_exp(ls);
    }
}

// kept iteration, beside k_holdout_accum, one held-out row per lane: fit and sd as that kernel and k_holdout_augment form them,
// p_c = exp(det_lpdiff((t_{c-1} - fit) / sd, (t_c - fit) / sd)) for c = 1 .. C (an interval without mass: 0), sum_prob[c-1][k] += p_c
// (class-major, m entries per class, in the order of the hold-out set).
__global__ __launch_bounds__(256) void k_holdout_prob(const long long *__restrict__ rows, long long m, int C, const double *__restrict__ ycorr,
                                                      const double *__restrict__ yaug, const double *__restrict__ rs,
                                                      const DScal *__restrict__ sc, const double *__restrict__ thr,
                                                      double *__restrict__ sum_prob, const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k >= m) return;
    const long long i = rows[k];
    const double yt = ycorr[i];
    const double ri = rs ? yt / rs[i] : yt;
    const double fit = yaug[k] - ri;
    const double sde = det_sqrt(sc->varE);
    const double sd = rs ? sde / rs[i] : sde;
    for (int c = 1; c <= C; c++) {
        const double lp = det_lpdiff((thr[c - 1] - fit) / sd, (thr[c] - fit) / sd);
        const double p = det_exp(lp);  // (lp <= 0; -inf gives 0)
        sum_prob[(long long)(c - 1) * m + k] = sum_prob[(long long)(c - 1) * m + k] + p;
    }
}

}  // namespace ngp
