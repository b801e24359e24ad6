// ngp_fixed_sparse.h -- gfx950 kernels of one fixed-effect set given as a sparse matrix (ngp_add_fixed_set_sparse): a classification
// factor of thousands of levels, or a block of crossed factors and covariates (sampleb!, src/functions.jl:22-36; set-up
// src/mme.jl:120-152).  The step is k_fixed's (ngp_kernels.h) without its zeros: k_fixed only multiplies and adds, a zero entry of X
// or of X'X is a no-op there (fma(0, y, acc) == acc, t - 0.0 == t), so visiting the stored entries in k_fixed's order and combining
// the partial sums along k_fixed's tree gives k_fixed's bits.  DESIGN.md section 2, "Sparse fixed-effect sets", is the normative
// description of every order used here; tests/ref_fixed_sparse.py restates it operation by operation.
//
// Per set and iteration, on the chain's stream, in the set's place among the fixed-effect sets:
//   k_fixs_yi       one 64-lane wave per column: Yi_a = (x_a'ycorr + sum_c X'X[a][c] b_c) iVarE; keeps b_a as b_old
//   k_fixs_gs_*     the Gauss-Seidel over the ridged X'X, level-scheduled: the columns of equal depth side by side
//   k_fixs_update   one thread per record: ycorr_i -= sum_a x_ia (b_a' - b_a)
#pragma once
#include "ngp_common.h"

#pragma clang fp contract(off)

namespace ngp {

// scratch rows of a set (NGP_FS_* x ncol doubles)
#define NGP_FS_YI 0
#define NGP_FS_BOLD 1
#define NGP_FS_DB 2
#define NGP_FS_ROWS 3
// a depth of more columns than this is a launch of its own (k_fixs_gs_wide), a run of narrower depths one workgroup (k_fixs_gs_fused)
#define NGP_FS_FUSE_ROWS 1024

// ------------------------------------------------------------------------------------------
// Yi.  256 threads = 4 waves = 4 columns per workgroup, 1024 LDS accumulators (8 KB) per wave: accumulator t holds what thread t of
// k_fixed holds, the fma chain over the records t, t + 1024, ... from 0.0.  The column's entries (CSC, rows strictly ascending) are
// walked in chunks of 64; the entries of one 1024-row round (row div 1024) never share an accumulator, a chunk that straddles rounds
// is done round by round (the lanes of the first pending round write, the others wait).  Then k_fixed's tree: the butterfly inside
// each group of 64 accumulators, the 16 group sums added in order.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fixs_yi(const double *__restrict__ ycorr, long long ncol, const long long *__restrict__ cptr,
                                                 const int *__restrict__ crow, const double *__restrict__ cval,
                                                 const long long *__restrict__ xptr, const int *__restrict__ xcol,
                                                 const double *__restrict__ xval, const double *__restrict__ b, double *__restrict__ scr,
                                                 const DScal *__restrict__ sc, const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;  // an earlier sweep of this call gave up (ngp_sweep_args.h, abort_w)
    __shared__ double accs[4][1024];
    const int lane = threadIdx.x & 63;
    const long long a = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (a >= ncol) return;  // (uniform over the wave; no workgroup barrier below)
    volatile double *acc = accs[threadIdx.x >> 6];  // volatile: lanes read what other lanes of the wave wrote, in program order
#pragma unroll
    for (int w = 0; w < 16; w++) acc[64 * w + lane] = 0.0;
    const long long p0 = cptr[a], p1 = cptr[a + 1];
    for (long long k0 = p0; k0 < p1; k0 += 64) {  // (uniform)
        const long long k = k0 + lane;
        bool pending = k < p1;
        const int i = pending ? crow[k] : 0;
        const double x = pending ? cval[k] : 0.0;
        const double yv = pending ? ycorr[i] : 0.0;
        const int round = i >> 10;
        unsigned long long m = __ballot(pending);
        while (m != 0ull) {  // (uniform: m is the same in every lane)
            const int first = __shfl(round, (int)__builtin_ctzll(m));  // rows ascend with the lane: the lowest pending lane holds the first round
            if (pending && round == first) {
                acc[i & 1023] = __builtin_fma(x, yv, acc[i & 1023]);
                pending = false;
            }
            m = __ballot(pending);
        }
    }
    double d = 0.0;
#pragma unroll
    for (int w = 0; w < 16; w++) {
        double s = acc[64 * w + lane];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) s = s + __shfl_xor(s, off);
        d = (w == 0) ? s : d + s;
    }
    if (lane != 0) return;
    double xb = 0.0;
    for (long long k = xptr[a]; k < xptr[a + 1]; k++) xb = __builtin_fma(xval[k], b[xcol[k]], xb);
    const double tot = d + xb;
    scr[NGP_FS_YI * ncol + a] = tot * sc->iVarE;
    scr[NGP_FS_BOLD * ncol + a] = b[a];
}

// ------------------------------------------------------------------------------------------
// Gauss-Seidel of k_fixed, level-scheduled.  depth(a) = 0 for a column whose row of X'X has no stored entry left of the diagonal,
// else 1 + max depth(c) over its stored c < a: every b_c (c < a) that column a reads belongs to a smaller depth and is already
// redrawn, every b_c (c > a) is read from b_old (a column of lower depth and higher index may already be redrawn in b).  The
// columns of one depth run side by side, one thread per column; the stream, or a workgroup barrier, orders the depths.
//   order[dptr[d] .. dptr[d + 1])   the columns of depth d, ascending
// b is read and written by many threads in turn, hence neither const nor __restrict__.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void fixs_gs_row(long long a, long long ncol, const long long *__restrict__ xptr, const int *__restrict__ xcol,
                                            const double *__restrict__ xval, const double *__restrict__ diagR, double *b, double *scr,
                                            double iVarE, int fset, uint64_t seed, uint64_t chain, uint64_t it) {
    const double *bold = scr + NGP_FS_BOLD * ncol;
    double d = 0.0;
    for (long long k = xptr[a]; k < xptr[a + 1]; k++) {
        const int c = xcol[k];
        if (c == a) continue;  // (k_fixed: bVec[a] = 0.0 in front of the chain)
        const double bv = (c < a) ? b[c] : bold[c];
        d = __builtin_fma(xval[k], bv, d);
    }
    const double t1 = d * iVarE;
    const double rhsb = scr[NGP_FS_YI * ncol + a] - t1;
    const double lhsb = diagR[a] * iVarE;
    const double inv = 1.0 / lhsb;
    const double meanb = inv * rhsb;
    Rng r = rng_seed(seed, chain, it, NGP_KIND_FIXED_NORMAL, ((uint64_t)(fset + 1) << 20) | (uint64_t)a);
    const double z = rng_normal(r);
    const double sd = det_sqrt(inv);
    const double tz = sd * z;
    const double bn = meanb + tz;
    scr[NGP_FS_DB * ncol + a] = bn - bold[a];
    b[a] = bn;
}

__global__ __launch_bounds__(256) void k_fixs_gs_wide(long long ncol, const long long *__restrict__ xptr, const int *__restrict__ xcol,
                                                      const double *__restrict__ xval, const double *__restrict__ diagR, double *b, double *scr,
                                                      const int *__restrict__ order, long long r0, long long r1, const DScal *__restrict__ sc,
                                                      int fset, uint64_t seed, uint64_t chain, uint64_t it, const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    const long long i = r0 + (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= r1) return;
    fixs_gs_row((long long)order[i], ncol, xptr, xcol, xval, diagR, b, scr, sc->iVarE, fset, seed, chain, it);
}

__global__ __launch_bounds__(1024) void k_fixs_gs_fused(long long ncol, const long long *__restrict__ xptr, const int *__restrict__ xcol,
                                                        const double *__restrict__ xval, const double *__restrict__ diagR, double *b, double *scr,
                                                        const int *__restrict__ order, const long long *__restrict__ dptr, int d0, int d1,
                                                        const DScal *__restrict__ sc, int fset, uint64_t seed, uint64_t chain, uint64_t it,
                                                        const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;  // (uniform over the workgroup)
    const double iVarE = sc->iVarE;
    for (int d = d0; d < d1; d++) {  // (uniform: every thread meets every barrier)
        const long long r1 = dptr[d + 1];
        for (long long i = dptr[d] + threadIdx.x; i < r1; i += 1024)
            fixs_gs_row((long long)order[i], ncol, xptr, xcol, xval, diagR, b, scr, iVarE, fset, seed, chain, it);
        __threadfence_block();
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------
// ycorr_i -= t, t the fma chain from 0.0 over the record's entries (CSR of X, columns ascending) of x_ia db_a
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_fixs_update(double *__restrict__ ycorr, long long N, long long ncol, const long long *__restrict__ rptr,
                                                     const int *__restrict__ rcol, const double *__restrict__ rval,
                                                     const double *__restrict__ scr, const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const double *db = scr + NGP_FS_DB * ncol;
    double t = 0.0;
    for (long long k = rptr[i]; k < rptr[i + 1]; k++) t = __builtin_fma(rval[k], db[rcol[k]], t);
    ycorr[i] = ycorr[i] - t;
}

}  // namespace ngp
