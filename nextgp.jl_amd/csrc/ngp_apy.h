// ngp_apy.h -- GBLUP at scale: the APY (algorithm for proven and young) form of inv(G) and the Gauss-Seidel of a random-effect set over
// it.  DESIGN.md section 2, "APY random-effect sets", is the normative description of every summation order here; tests/ref_apy.py
// restates the model in plain fp64.  Kernels of a translation unit of their own (ngp_apy_inst.hip).  Everything is fp64; no FMA in
// the sampler's kernels (fp contract off, no __builtin_fma): every product and sum is rounded on its own.  The matrix core's own
// accumulation (four products added to the accumulator one after the other) is the only fused arithmetic, and only set-up uses it.
//
// Levels: the nc core animals first, then the nn = N - nc non-core ones.  With Kc0 = inv(Gcc), P = Gnc Kc0 (nn x nc), m_i = g_ii - P_i. Gnc_i.,
// d_i = 1 / m_i and Kcc = Kc0 + P' diag(d) P the precision is [Kcc, -P'D; -DP, D]: a dense block over the core, and every non-core level
// conditionally independent of the others given the core.
//
// Per iteration, between k_rand_levels (all N levels; kdiag = diag(Kcc) | d) and k_rand_update (ngp_random.h), on the chain's stream:
//   k_apy_check     is u_n still the vector the seed s was formed from?  (bit patterns; u set from outside or restored: no)
//   k_apy_tail      draws off, only where k_apy_check said no: s = -P' D u_n again, by the operations of the fused pass
//   k_apy_reduce    (the same condition)
//   k_apy_seed      the below-block accumulator of core level l starts from s_l (k_dense_dhi would have written 0.0)
//   k_hyb_dhi, k_hyb_block (ngp_hybrid.h)  the blocked chain over Kcc, nc levels, from the seeded accumulator
//   k_apy_tail      THE PASS OVER P, once: per non-core row i  v_i = P_i. u_c (this sweep's core values), the draw of u_i, du_i, the
//                   term d_i (u_i - v_i)^2, and s -= P_i. d_i u_i for the next sweep
//   k_apy_reduce    the workgroups' partials of s and of the quadratic term, in workgroup order
//   k_apy_quad0     per core row the part of Kc0 u_c left of the diagonal, in the order the dense chain forms its dlo
//   k_apy_var       u'Ku = u_c' Kc0 u_c + sum_i d_i (u_i - v_i)^2 (both terms non-negative), then varU as k_dense_var draws it
//
// k_apy_tail<CPT, R>: 512 threads = 8 waves; thread tid owns the columns tid + 512 m, m < CPT, of every row its workgroup sees.  Its
// slice of u_c and its slice of the workgroup's partial of s stay in registers for the whole launch.  A workgroup owns the
// NGP_APY_WG_ROWS rows from NGP_APY_WG_ROWS * blockIdx.x on -- a function of nn and that constant only, never of the device -- and
// steps over them R at a time: the R x CPT entries of P a thread owns are loaded (coalesced: the threads of a wave read 64 adjacent
// doubles of a row) and stay in registers for the step; the R dot products are reduced across the workgroup by the butterfly inside
// each wave and the 8 wave sums added in wave order through LDS; thread r draws row r and leaves w_r = d_r u_r in LDS; every thread
// then takes w_r P_rc from its slice of s with the P entries it still holds.  LDS carries the reduction and the broadcast only; P
// is read once from HBM.
// The limit on the core: 512 threads x CPT = 16 columns = 8,192.  Registers at CPT = 16, R = 4: u_c 32 + s 32 + P 128 = 192 VGPRs
// of live data; a workgroup of 8 waves puts two waves on each SIMD, which leaves 512 / 2 = 256 VGPRs per lane -- one more row per step
// or one more wave per SIMD would spill.  Cores of at most 2,048 take CPT = 4, R = 8 (96 VGPRs of live data).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#ifdef NGP_APY_KERNELS
#include "ngp_common.h"
#endif

namespace ngp {

#define NGP_APY_MAX_CORE 8192   // 512 threads x 16 columns (above: the register budget)
#define NGP_APY_WG_ROWS 256     // non-core rows per workgroup of k_apy_tail (a multiple of every R)
#define NGP_APY_T 512           // threads of k_apy_tail

// per-iteration arguments of an APY set: q = N levels, nc core; the NGP_RS_* rows of the set's scratch (stride q) by pointer
struct ApyStep {
    long long q, nc, ldp, ldk;                 // ldp: row stride of P; ldk: leading dimension of Kc0
    const double *P, *d, *Kc0, *kdiag0;        // P nn x nc row-major; d nn; Kc0 and its diagonal
    double *u;                                 // q
    const double *vu;                          // varU of this sweep
    const double *Yi, *inv, *tz;               // scratch rows of k_rand_levels (q each)
    double *du, *acc, *acc0, *seed, *dlo;      // scratch rows (q each): du; the chain's two accumulators and the seed row; dlo
    double *s, *spart, *qpart, *quad, *uprev;  // nc; nwg x nc; nwg; 1; nn -- the set's own
    unsigned *stale;                           // 1 word: u_n is not the vector s was formed from
    const unsigned *abort_w;
};
inline long long apy_tail_wgs(long long nn) { return (nn + NGP_APY_WG_ROWS - 1) / NGP_APY_WG_ROWS; }
hipError_t apy_seed(const ApyStep &a, hipStream_t stream);   // k_apy_check, the conditional rebuild of s, k_apy_seed
hipError_t apy_tail(const ApyStep &a, hipStream_t stream);   // the fused pass and k_apy_reduce
hipError_t apy_var(const ApyStep &a, double *vu, double df, double scale, int rset, uint64_t seed, uint64_t chain, uint64_t it, hipStream_t stream);
// set-up (ngp_grm_begin_apy .. ngp_grm_apy)
hipError_t apy_rownorm(const double *xc, long long Npad, long long N, long long cpad, double *gdiag, hipStream_t stream);
hipError_t apy_finish(double *panel, long long N, long long ld, long long nc, double *gdiag, double denom, hipStream_t stream);
hipError_t apy_gemm_p(const double *panel, long long N, long long Npad, long long nc, const double *Kc0, long long ldk, double *P, long long ldp, hipStream_t stream);
hipError_t apy_m(const double *panel, long long Npad, long long nc, long long nn, const double *P, long long ldp, const double *gdiag, double *m, double *d,
                 hipStream_t stream);
hipError_t apy_gemm_kcc(const double *P, long long ldp, long long nnpad, const double *d, double *Kcc, long long ldk, hipStream_t stream);
hipError_t apy_digest(const double *A, long long rows, long long cols, long long ld, unsigned long long *rowhash, hipStream_t stream);
// W = K_APY X for the SNP back-solve and GBLUP prediction (k_apy_kw_tail, k_apy_kw_core below; cw by k_bs_cw of ngp_backsolve.h).  X and W
// are N x T, column-major with leading dimension N, levels core first; cw_t = sum_i W[i, t].  The pieces as ApyK holds them: P nnpad x ldp
// row-major with zeros beyond nn and nc, ldp a multiple of 64; d nn; Kc0 column-major (symmetric) with leading dimension ldk.
struct ApyKw {
    long long N, nc, ldp, ldk;
    const double *P, *d, *Kc0;
};
hipError_t apy_kw(const ApyKw &k, const double *X, long long T, double *W, double *cw, hipStream_t stream);

#ifdef NGP_APY_KERNELS

#pragma clang fp contract(off)

typedef double apy_d4 __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------
// One thread per non-core level: a bit pattern of u_n other than the one s was formed from raises the word (an integer OR: no order).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_apy_check(long long nn, const double *__restrict__ un, const double *__restrict__ uprev, unsigned *__restrict__ stale,
                                                   const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nn) return;
    if (__double_as_longlong(un[i]) != __double_as_longlong(uprev[i])) atomicOr(stale, 1u);
}

// ------------------------------------------------------------------------------------------
// The pass over P.  DRAW = 1: the fused pass of an iteration.  DRAW = 0: the rebuild of s from a u_n given from outside -- returns at
// once unless *stale is set; u_r is read, not drawn, everything that concerns s is the same text.  Per step of R rows (row = first
// row of the step + r; rows >= nn are zeros by predicated loads, as are columns >= nc):
//   thread:    a_r = sum over m ascending of P[row][tid + 512 m] * uc[tid + 512 m], from 0.0 (one product, one sum each)
//   wave:      the butterfly a_r = a_r + shfl_xor(a_r, off), off = 32 .. 1
//   thread r:  v = the 8 wave sums added in wave order (from wave 0's);
//              t = d * v;  t = t * iVarU;  rhs = Yi + t;  mean = inv * rhs;  un = mean + tz;  du = un - u(old)
//              e = un - v;  e2 = e * e;  qt = d * e2;  qacc_r = qacc_r + qt          (qacc_r from 0.0, over the steps in row order)
//              w_r = d * un
//   thread:    for r ascending, for m:  t = P[row][tid + 512 m] * w_r;  s_m = s_m - t      (s_m from 0.0: the workgroup's partial)
// At the end the partial of s goes to spart[workgroup][column], and thread 0 adds qacc_0 .. qacc_{R-1} in that order into qpart[workgroup].
// ------------------------------------------------------------------------------------------
template <int CPT, int R, int DRAW>
__global__ __launch_bounds__(NGP_APY_T) void k_apy_tail(ApyStep a) {
    __shared__ double red[NGP_APY_T / 64][R];
    __shared__ double sw[R];
    if (a.abort_w && *a.abort_w != 0u) return;
    if (!DRAW && *a.stale == 0u) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long nc = a.nc, nn = a.q - a.nc;
    const long long row0 = (long long)blockIdx.x * NGP_APY_WG_ROWS;
    const long long row1 = (row0 + NGP_APY_WG_ROWS) < nn ? (row0 + NGP_APY_WG_ROWS) : nn;
    double uc[CPT], s[CPT];
#pragma unroll
    for (int m = 0; m < CPT; m++) {
        const long long c = tid + (long long)NGP_APY_T * m;
        uc[m] = c < nc ? a.u[c] : 0.0;
        s[m] = 0.0;
    }
    const double iVarU = 1.0 / a.vu[0];
    double qacc = 0.0;
    for (long long g = row0; g < row1; g += R) {  // (uniform over the workgroup: every thread meets every barrier)
        double p[R][CPT], dot[R];
#pragma unroll
        for (int r = 0; r < R; r++) {
            const double *prow = a.P + (size_t)(g + r) * (size_t)a.ldp;
            const bool rok = g + r < row1;
#pragma unroll
            for (int m = 0; m < CPT; m++) {
                const long long c = tid + (long long)NGP_APY_T * m;
                p[r][m] = (rok && c < nc) ? prow[c] : 0.0;
            }
        }
#pragma unroll
        for (int r = 0; r < R; r++) {
            double acc = 0.0;
#pragma unroll
            for (int m = 0; m < CPT; m++) {
                const double t = p[r][m] * uc[m];
                acc = acc + t;
            }
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off);
            dot[r] = acc;
        }
        if (lane == 0) {
#pragma unroll
            for (int r = 0; r < R; r++) red[wv][r] = dot[r];
        }
        __syncthreads();
        if (tid < R) {
            const long long i = g + tid;
            double w = 0.0;
            if (i < row1) {
                double v = red[0][tid];
                for (int k = 1; k < NGP_APY_T / 64; k++) v = v + red[k][tid];
                const double d = a.d[i];
                double un;
                if (DRAW) {
                    const long long l = nc + i;
                    double t = d * v;
                    t = t * iVarU;
                    const double rhs = a.Yi[l] + t;
                    const double mean = a.inv[l] * rhs;
                    un = mean + a.tz[l];
                    const double uo = a.u[l];
                    a.du[l] = un - uo;
                    a.u[l] = un;
                    const double e = un - v;
                    const double e2 = e * e;
                    const double qt = d * e2;
                    qacc = qacc + qt;
                } else {
                    un = a.u[nc + i];
                }
                a.uprev[i] = un;
                w = d * un;
            }
            sw[tid] = w;
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; r++) {
            const double w = sw[r];
#pragma unroll
            for (int m = 0; m < CPT; m++) {
                const double t = p[r][m] * w;
                s[m] = s[m] - t;
            }
        }
    }
#pragma unroll
    for (int m = 0; m < CPT; m++) {
        const long long c = tid + (long long)NGP_APY_T * m;
        if (c < nc) a.spart[(size_t)blockIdx.x * (size_t)nc + (size_t)c] = s[m];
    }
    if (DRAW) {  // (the barrier above has passed: red is free)
        if (tid < R) red[0][tid] = qacc;
        __syncthreads();
        if (tid == 0) {
            double qq = red[0][0];
            for (int r = 1; r < R; r++) qq = qq + red[0][r];
            a.qpart[blockIdx.x] = qq;
        }
    }
}

// ------------------------------------------------------------------------------------------
// s_c = spart[0][c] + spart[1][c] + ... in workgroup order (one thread per column; from the first partial), and quad = the same over
// qpart (thread 0 of workgroup 0; DRAW only).  cond: the rebuild's launch, which returns at once unless *stale is set.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_apy_reduce(long long nc, long long nwg, const double *__restrict__ spart, const double *__restrict__ qpart,
                                                    double *__restrict__ s, double *__restrict__ quad, int cond, const unsigned *__restrict__ stale,
                                                    const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    if (cond && *stale == 0u) return;
    const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
    if (c < nc) {
        double acc = spart[c];
        for (long long w = 1; w < nwg; w++) acc = acc + spart[(size_t)w * (size_t)nc + (size_t)c];
        s[c] = acc;
    }
    if (!cond && c == 0) {
        double qq = qpart[0];
        for (long long w = 1; w < nwg; w++) qq = qq + qpart[w];
        quad[0] = qq;
    }
}

// The chain's accumulators of core level l: acc_l = s_l (and the seed row), acc0_l = 0.0; the stale word is cleared (s is current now).
__global__ __launch_bounds__(256) void k_apy_seed(long long nc, const double *__restrict__ s, double *__restrict__ acc, double *__restrict__ acc0,
                                                  double *__restrict__ seed, unsigned *__restrict__ stale, const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    const long long l = (long long)blockIdx.x * 256 + threadIdx.x;
    if (l == 0) *stale = 0u;
    if (l >= nc) return;
    const double v = s[l];
    acc[l] = v; seed[l] = v; acc0[l] = 0.0;
}

// ------------------------------------------------------------------------------------------
// dlo0_l = the part of (Kc0 u_c)_l left of the diagonal, one wave per core row, in the order the blocked chain of ngp_dense.h forms its
// dlo: from 0.0, per full block t in front of l's own the butterfly sum of the 64 products Kc0[l][64 t + j] * u[64 t + j] added to
// the accumulator, then the products of l's own block one after the other, columns ascending (lane 0).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_apy_quad0(const double *__restrict__ K0, long long ld, long long nc, const double *__restrict__ u,
                                                   double *__restrict__ dlo, const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    const int lane = threadIdx.x & 63;
    const long long l = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (l >= nc) return;  // (uniform over the wave)
    const double *row = K0 + (size_t)l * (size_t)ld;
    const long long b0 = l & ~63LL;
    double acc = 0.0;
    for (long long c0 = 0; c0 < b0; c0 += 64) {
        double p = row[c0 + lane] * u[c0 + lane];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) p = p + __shfl_xor(p, off);
        acc = acc + p;
    }
    if (lane != 0) return;
    for (long long c = b0; c < l; c++) {
        const double p = row[c] * u[c];
        acc = acc + p;
    }
    dlo[l] = acc;
}

// ------------------------------------------------------------------------------------------
// varU of an APY set, ONE workgroup of 1024 threads: k_dense_var over the nc core levels with Kc0's diagonal and dlo0,
//   a = Kc0_ll * u_l;  b = 2.0 * dlo0_l;  s = a + b;  p = u_l * s;  acc = acc + p
// the butterfly inside each wave, the 16 wave sums added in wave order, then quad = (that) + (the tail's sum of d_i (u_i - v_i)^2);
// t = scale * df; t = t + quad; varU = t / chi2(df + q) keyed (NGP_KIND_U_CHI2, set), q all N levels.  The quadratic form is left in quad[1].
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_apy_var(long long q, long long nc, const double *__restrict__ kdiag0, const double *__restrict__ u,
                                                  const double *__restrict__ dlo, double *__restrict__ quadw, double *__restrict__ vu, double df,
                                                  double scale, int rset, uint64_t seed, uint64_t chain, uint64_t it,
                                                  const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    __shared__ double wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double acc = 0.0;
    for (long long l = tid; l < nc; l += 1024) {
        const double a = kdiag0[l] * u[l];
        const double b = 2.0 * dlo[l];
        const double s = a + b;
        const double p = u[l] * s;
        acc = acc + p;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off);
    if (lane == 0) wsum[wv] = acc;
    __syncthreads();
    if (tid == 0) {
        double quad = wsum[0];
        for (int k = 1; k < 16; k++) quad = quad + wsum[k];
        quad = quad + quadw[0];
        quadw[1] = quad;
        Rng r = rng_seed(seed, chain, it, NGP_KIND_U_CHI2, (uint64_t)rset);
        const double chi = rng_chisq(r, df + (double)q);
        double t = scale * df;
        t = t + quad;
        vu[0] = t / chi;
    }
}

// ==========================================================================================
// Set-up: the N x nc column panel of G, the non-core diagonal, P, m and Kcc
// ==========================================================================================

// gdiag_i += sum over the chunk's columns, ascending, of xc_ik^2 (one product, one sum each); one thread per row of the centred chunk
__global__ __launch_bounds__(256) void k_apy_rownorm(const double *__restrict__ xc, long long Npad, long long N, long long cpad, double *__restrict__ gdiag) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    double acc = gdiag[i];
    for (long long k = 0; k < cpad; k++) {
        const double x = xc[(size_t)k * (size_t)Npad + (size_t)i];
        const double t = x * x;
        acc = acc + t;
    }
    gdiag[i] = acc;
}

// k_grm_mirror's finish over the panel (column-major, columns 0 .. nc - 1; i >= j computed): v = v / denom, 0.001 added on the diagonal,
// the core block mirrored; and gdiag_i = gdiag_i / denom + 0.001
__global__ __launch_bounds__(256) void k_apy_finish(double *__restrict__ panel, long long N, long long ld, long long nc, double *__restrict__ gdiag, double denom) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    if (blockIdx.y == 0) {
        double g = gdiag[i] / denom;
        gdiag[i] = g + 0.001;
    }
    const long long jend = i < nc ? i : nc - 1;
    for (long long j = blockIdx.y; j <= jend; j += gridDim.y) {
        double v = panel[(size_t)i + (size_t)j * (size_t)ld];
        v = v / denom;
        if (i == j) v = v + 0.001;
        panel[(size_t)i + (size_t)j * (size_t)ld] = v;
        if (i != j && i < nc) panel[(size_t)j + (size_t)i * (size_t)ld] = v;
    }
}

// P = Gnc Kc0 on the matrix cores (v_mfma_f64_16x16x4_f64), k_grm_syrk's conventions: a workgroup of 4 waves owns 64 non-core rows x 64
// core columns, wave w the 32 x 32 quarter (w >> 1, w & 1) as 2 x 2 accumulators of 16 x 16.  Lane l = (cc = l & 15, rr = l >> 4) supplies
// A[row cc][k = rr] = G[nc + row][k] (the panel, column-major; rows >= N are zeros by predicated loads) and B[k = rr][col cc] =
// Kc0[col][k] (symmetric, zero beyond nc: the panel's columns nc .. ldk - 1 meet zeros).  Every P_ic is ONE chain over k ascending, four at
// a time, from 0.0.  D layout: lane l, register v holds row rr + 4 v, column cc.  P is row-major with stride ldp.
__global__ __launch_bounds__(256) void k_apy_gemm_p(const double *__restrict__ panel, long long N, long long Npad, long long nc, const double *__restrict__ K0,
                                                    long long ldk, double *__restrict__ P, long long ldp) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const long long i0 = 64LL * blockIdx.x + 32 * (w >> 1), j0 = 64LL * blockIdx.y + 32 * (w & 1);
    const int rr = l >> 4, cc = l & 15;
    apy_d4 a00 = {0.0, 0.0, 0.0, 0.0}, a01 = a00, a10 = a00, a11 = a00;
    const long long g0 = nc + i0 + cc, g1 = g0 + 16;
    const bool ok0 = g0 < N, ok1 = g1 < N;
    const double *pa = panel + (size_t)rr * (size_t)Npad;
    const double *pb = K0 + (size_t)rr * (size_t)ldk + (size_t)(j0 + cc);
    for (long long k = 0; k < ldk; k += 4) {
        const double x0 = ok0 ? pa[g0] : 0.0, x1 = ok1 ? pa[g1] : 0.0, y0 = pb[0], y1 = pb[16];
        a00 = __builtin_amdgcn_mfma_f64_16x16x4f64(x0, y0, a00, 0, 0, 0);
        a01 = __builtin_amdgcn_mfma_f64_16x16x4f64(x0, y1, a01, 0, 0, 0);
        a10 = __builtin_amdgcn_mfma_f64_16x16x4f64(x1, y0, a10, 0, 0, 0);
        a11 = __builtin_amdgcn_mfma_f64_16x16x4f64(x1, y1, a11, 0, 0, 0);
        pa += 4 * (size_t)Npad; pb += 4 * (size_t)ldk;
    }
    const long long nn = N - nc;
#pragma unroll
    for (int v = 0; v < 4; v++) {
        const long long r = i0 + rr + 4 * v;
        if (r < nn) {
            P[(size_t)r * (size_t)ldp + (size_t)(j0 + cc)] = a00[v];
            P[(size_t)r * (size_t)ldp + (size_t)(j0 + 16 + cc)] = a01[v];
        }
        if (r + 16 < nn) {
            P[(size_t)(r + 16) * (size_t)ldp + (size_t)(j0 + cc)] = a10[v];
            P[(size_t)(r + 16) * (size_t)ldp + (size_t)(j0 + 16 + cc)] = a11[v];
        }
    }
}

// m_i = g_ii - P_i. Gnc_i., d_i = 1 / m_i: one wave per non-core row; lane j adds the columns j, j + 64, ... (from 0.0), the butterfly
__global__ __launch_bounds__(256) void k_apy_m(const double *__restrict__ panel, long long Npad, long long nc, long long nn, const double *__restrict__ P,
                                               long long ldp, const double *__restrict__ gdiag, double *__restrict__ m, double *__restrict__ d) {
    const int lane = threadIdx.x & 63;
    const long long i = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= nn) return;  // (uniform over the wave)
    double acc = 0.0;
    for (long long c = lane; c < nc; c += 64) {
        const double t = P[(size_t)i * (size_t)ldp + (size_t)c] * panel[(size_t)(nc + i) + (size_t)c * (size_t)Npad];
        acc = acc + t;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off);
    if (lane != 0) return;
    const double mi = gdiag[nc + i] - acc;
    m[i] = mi;
    d[i] = 1.0 / mi;
}

// Kcc += P' diag(d) P on the matrix cores, the lower triangle of 64 x 64 tile blocks (blockIdx.x >= blockIdx.y), in k_grm_syrk's
// conventions with the non-core rows in the place of the chunk's columns: A[a][k = i] = P[i][a], B[k = i][b] = d_i * P[i][b] (one
// product, rounded, before the core sees it).  P has nnpad rows (a multiple of 4, zeros beyond nn) and d is zero beyond nn.  The
// accumulators start from Kcc as it lies there (Kc0): every entry is ONE chain over the non-core rows in their order.  Column-major, ld = ldk.
__global__ __launch_bounds__(256) void k_apy_gemm_kcc(const double *__restrict__ P, long long ldp, long long nnpad, const double *__restrict__ d,
                                                      double *__restrict__ Kcc, long long ldk) {
    const int bi = blockIdx.x, bj = blockIdx.y;
    if (bj > bi) return;  // (block-uniform)
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const long long i0 = 64LL * bi + 32 * (w >> 1), j0 = 64LL * bj + 32 * (w & 1);
    const int rr = l >> 4, cc = l & 15;
    apy_d4 a00, a01, a10, a11;
#pragma unroll
    for (int v = 0; v < 4; v++) {
        const long long r = rr + 4 * v;
        a00[v] = Kcc[(size_t)(i0 + r) + (size_t)(j0 + cc) * (size_t)ldk];
        a01[v] = Kcc[(size_t)(i0 + r) + (size_t)(j0 + 16 + cc) * (size_t)ldk];
        a10[v] = Kcc[(size_t)(i0 + 16 + r) + (size_t)(j0 + cc) * (size_t)ldk];
        a11[v] = Kcc[(size_t)(i0 + 16 + r) + (size_t)(j0 + 16 + cc) * (size_t)ldk];
    }
    const double *pa = P + (size_t)rr * (size_t)ldp + (size_t)(i0 + cc);
    const double *pb = P + (size_t)rr * (size_t)ldp + (size_t)(j0 + cc);
    const size_t step = 4 * (size_t)ldp;
    for (long long k = 0; k < nnpad; k += 4) {
        const double dk = d[k + rr];
        const double x0 = pa[0], x1 = pa[16], y0 = dk * pb[0], y1 = dk * pb[16];
        a00 = __builtin_amdgcn_mfma_f64_16x16x4f64(x0, y0, a00, 0, 0, 0);
        a01 = __builtin_amdgcn_mfma_f64_16x16x4f64(x0, y1, a01, 0, 0, 0);
        a10 = __builtin_amdgcn_mfma_f64_16x16x4f64(x1, y0, a10, 0, 0, 0);
        a11 = __builtin_amdgcn_mfma_f64_16x16x4f64(x1, y1, a11, 0, 0, 0);
        pa += step; pb += step;
    }
#pragma unroll
    for (int v = 0; v < 4; v++) {
        const long long r = rr + 4 * v;
        Kcc[(size_t)(i0 + r) + (size_t)(j0 + cc) * (size_t)ldk] = a00[v];
        Kcc[(size_t)(i0 + r) + (size_t)(j0 + 16 + cc) * (size_t)ldk] = a01[v];
        Kcc[(size_t)(i0 + 16 + r) + (size_t)(j0 + cc) * (size_t)ldk] = a10[v];
        Kcc[(size_t)(i0 + 16 + r) + (size_t)(j0 + 16 + cc) * (size_t)ldk] = a11[v];
    }
}

// k_dense_digest for a rows x cols matrix (row l at A + l ld): the same fold, so a square matrix gives k_dense_digest's words
__global__ __launch_bounds__(256) void k_apy_digest(const double *__restrict__ A, long long rows, long long cols, long long ld,
                                                    unsigned long long *__restrict__ rowhash) {
    const int lane = threadIdx.x & 63;
    const long long l = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (l >= rows) return;  // (uniform over the wave)
    const double *row = A + (size_t)l * (size_t)ld;
    unsigned long long x = 1469598103934665603ull;
    for (long long c = lane; c < cols; c += 64) { x ^= (unsigned long long)__double_as_longlong(row[c]); x *= 1099511628211ull; }
    unsigned long long r = 1469598103934665603ull;
    for (int j = 0; j < 64; j++) { r ^= __shfl(x, j); r *= 1099511628211ull; }
    if (lane == 0) rowhash[l] = r;
}

// ==========================================================================================
// W = K_APY X for a batch of T vectors (the draw store U of the SNP back-solve, or the relationship block C' of GBLUP prediction), by
// the factored form -- the N x N matrix is never formed, and Kc0 is used, not Kcc, so that P'DP is not cancelled against itself:
//   E = Xn - P Xc;   Wn = D E;   Wc = Kc0 Xc - P' Wn
// Two kernels on the matrix cores (v_mfma_f64_16x16x4_f64) in the conventions of k_bs_kw and k_grm_syrk: lane l = (cc = l & 15,
// rr = l >> 4) supplies A[row cc][k = rr] and B[k = rr][col cc], the core adds the four products one after the other, k ascending; D:
// lane l, register v holds row rr + 4 v, column cc.  A workgroup of 256 threads owns 64 rows x 64 draws, wave w the 16-draw group w as
// four 16 x 16 accumulators.  Every entry of W is a function of its row and its draw alone: each sum is ONE chain from 0.0 over all of
// its terms in their order, so neither the grid nor T nor the grouping of the draws shows in the bits.
// LDS tiles hold 64 lines (rows of P, or draws) of 64 k-values at a stride of NGP_APY_KS = 66 doubles: the loaders write 64 adjacent
// doubles per wave; the half wave rr = 0, 1 (and 2, 3) reads the doubles 66 cc + rr, dwords 4 cc + 2 rr (mod 64): every bank once.
// ==========================================================================================
#define NGP_APY_KS 66
#define NGP_APY_KW_TAIL_LDS (2 * 64 * NGP_APY_KS * sizeof(double))  // the tile of P and the tile of Xc: 67,584 bytes (dynamic: above 64 KiB)

// The thread's share of the step's two tiles into registers: line w + 4 j (j < 16), k-value l -- a wave reads 64 adjacent doubles of a row
// of P (row-major) or of a draw of Xc.  Rows >= nn, k >= nc of Xc and draws >= T are zeros by predication; a row of P holds zeros from nc
// to ldp (a multiple of 64), so the step's 64 columns lie inside it.
__device__ __forceinline__ void apy_kw_fetch(const double *__restrict__ P, long long ldp, long long nn, long long i0, const double *__restrict__ X, long long N,
                                             long long nc, long long T, long long t0, long long k0, int w, int l, double (&p)[16], double (&x)[16]) {
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const long long i = i0 + w + 4 * j, t = t0 + w + 4 * j, k = k0 + l;
        p[j] = i < nn ? P[(size_t)i * (size_t)ldp + (size_t)k] : 0.0;
        x[j] = (k < nc && t < T) ? X[(size_t)k + (size_t)t * (size_t)N] : 0.0;
    }
}

// Wn: grid (ceil(nn / 64), ceil(T / 64)).  The core is walked in steps of 64: A[row i][k] = P[i][k] is wanted by columns and P lies by rows,
// so its 64 x 64 tile goes through LDS (as the tile of Xc does, shared by the four waves); the global loads of step k + 1 are issued into
// registers before the matrix steps of step k and written to LDS behind them (one buffer: the registers hide the load).  Then, each
// rounded on its own:  acc = (P Xc)[i, t], one chain from 0.0, k ascending in fours;  e = x_{nc + i, t} - acc;  w = d_i * e.
__global__ __launch_bounds__(256) void k_apy_kw_tail(const double *__restrict__ P, long long ldp, const double *__restrict__ d, long long N, long long nc,
                                                     const double *__restrict__ X, long long T, double *__restrict__ W) {
    extern __shared__ double apy_kw_lds[];
    double *sP = apy_kw_lds, *sX = apy_kw_lds + 64 * NGP_APY_KS;
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, rr = l >> 4, cc = l & 15;
    const long long nn = N - nc, i0 = 64LL * blockIdx.x, t0 = 64LL * blockIdx.y;
    apy_d4 acc[4];
#pragma unroll
    for (int s = 0; s < 4; s++) acc[s] = apy_d4{0.0, 0.0, 0.0, 0.0};
    double p[16], x[16];
    apy_kw_fetch(P, ldp, nn, i0, X, N, nc, T, t0, 0, w, l, p, x);
    for (long long k0 = 0; k0 < nc; k0 += 64) {
        __syncthreads();  // (the tiles of the step before have been read)
#pragma unroll
        for (int j = 0; j < 16; j++) {
            sP[(w + 4 * j) * NGP_APY_KS + l] = p[j];
            sX[(w + 4 * j) * NGP_APY_KS + l] = x[j];
        }
        __syncthreads();
        if (k0 + 64 < nc) apy_kw_fetch(P, ldp, nn, i0, X, N, nc, T, t0, k0 + 64, w, l, p, x);  // (uniform; in flight during the matrix steps)
#pragma unroll
        for (int kb = 0; kb < 16; kb++) {
            const double b = sX[(16 * w + cc) * NGP_APY_KS + 4 * kb + rr];
#pragma unroll
            for (int s = 0; s < 4; s++) acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(sP[(16 * s + cc) * NGP_APY_KS + 4 * kb + rr], b, acc[s], 0, 0, 0);
        }
    }
    const long long t = t0 + 16 * w + cc;
    if (t < T) {
#pragma unroll
        for (int s = 0; s < 4; s++)
#pragma unroll
            for (int v = 0; v < 4; v++) {
                const long long i = i0 + 16 * s + rr + 4 * v;
                if (i < nn) {
                    const size_t at = (size_t)(nc + i) + (size_t)t * (size_t)N;
                    const double e = X[at] - acc[s][v];
                    W[at] = d[i] * e;
                }
            }
    }
}

// acc[s] += sum_k A[k][r0 + 16 s + cc] B[k, t0 + 16 w + cc], k ascending in fours over 0 .. klim - 1: k_bs_kw's loop.  Row k of A lies at
// A + k lda with the 64 wanted entries adjacent -- sixteen consecutive doubles per quarter wave, straight from memory into the A operand
// (each element is used once per draw group); the 64 x 64 tile of B (column-major, leading dimension ldb) goes through LDS.  Entries with
// k >= klim, r >= rlim or t >= T are zeros by predicated loads.
__device__ __forceinline__ void apy_kw_chain(const double *__restrict__ A, long long lda, long long rlim, long long klim, long long r0, const double *B,
                                             long long ldb, long long T, long long t0, double *sX, apy_d4 (&acc)[4]) {
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, rr = l >> 4, cc = l & 15;
    for (long long k0 = 0; k0 < klim; k0 += 64) {
        double a[4][16];  // the A tile of this lane: in flight while the B tile is staged
#pragma unroll
        for (int kb = 0; kb < 16; kb++) {
            const long long k = k0 + 4 * kb + rr;
#pragma unroll
            for (int s = 0; s < 4; s++) {
                const long long r = r0 + 16 * s + cc;
                a[s][kb] = (k < klim && r < rlim) ? A[(size_t)k * (size_t)lda + (size_t)r] : 0.0;
            }
        }
        __syncthreads();  // (the tile of the step before has been read)
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const long long k = k0 + l, t = t0 + w + 4 * j;
            sX[(w + 4 * j) * NGP_APY_KS + l] = (k < klim && t < T) ? B[(size_t)k + (size_t)t * (size_t)ldb] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int kb = 0; kb < 16; kb++) {
            const double b = sX[(16 * w + cc) * NGP_APY_KS + 4 * kb + rr];
#pragma unroll
            for (int s = 0; s < 4; s++) acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s][kb], b, acc[s], 0, 0, 0);
        }
    }
}

// Wc: grid (ceil(nc / 64), ceil(T / 64)), after k_apy_kw_tail on the same stream.  Two chains per entry, each from 0.0:
//   a1 = (Kc0 Xc)[c, t], k ascending in fours -- Kc0 is symmetric, row k serves as column k: k_bs_kw's chain over K, so with nc = N this
//        is k_bs_kw's W bit for bit;
//   a2 = sum_i P[i][c] Wn[i, t], i ascending in fours over the non-core rows -- row-major P plays the part the symmetric K plays above.
// w = a1 - a2, one subtraction; without non-core rows the kernel stores a1 itself.
__global__ __launch_bounds__(256) void k_apy_kw_core(const double *__restrict__ K0, long long ldk, const double *__restrict__ P, long long ldp, long long N,
                                                     long long nc, const double *__restrict__ X, long long T, double *W) {
    __shared__ double sX[64 * NGP_APY_KS];
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63, rr = l >> 4, cc = l & 15;
    const long long nn = N - nc, c0 = 64LL * blockIdx.x, t0 = 64LL * blockIdx.y;
    apy_d4 a1[4], a2[4];
#pragma unroll
    for (int s = 0; s < 4; s++) { a1[s] = apy_d4{0.0, 0.0, 0.0, 0.0}; a2[s] = a1[s]; }
    apy_kw_chain(K0, ldk, nc, nc, c0, X, N, T, t0, sX, a1);
    if (nn > 0) apy_kw_chain(P, ldp, nc, nn, c0, W + nc, N, T, t0, sX, a2);  // (uniform over the grid)
    const long long t = t0 + 16 * w + cc;
    if (t < T) {
#pragma unroll
        for (int s = 0; s < 4; s++)
#pragma unroll
            for (int v = 0; v < 4; v++) {
                const long long c = c0 + 16 * s + rr + 4 * v;
                if (c < nc) W[(size_t)c + (size_t)t * (size_t)N] = nn > 0 ? a1[s][v] - a2[s][v] : a1[s][v];
            }
    }
}

#endif  // NGP_APY_KERNELS

}  // namespace ngp
