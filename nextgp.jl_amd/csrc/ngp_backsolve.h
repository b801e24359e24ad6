// ngp_backsolve.h -- SNP effects from GBLUP: every kept draw u_t of a dense random-effect set whose K = inv(G) was built by ngp_grm_* is
// solved back to the markers, beta_{j,t} = d_j sum_i (z_ij - mu_j) w_{i,t} with w_t = K u_t ("SNP effects from
// GBLUP": the normative orders).  Kernels of a translation unit of their own (ngp_backsolve_inst.hip), beside the API unit and the sweep
// units: none of those carries code it did not carry before.
//   k_bs_store     u of a kept iteration into column t of the draw store U (q x max_draws, column-major)
//   k_bs_kw        W = K U on the matrix cores (v_mfma_f64_16x16x4_f64): a workgroup owns 64 rows of K x 64 draws, wave w the 16-draw group w
//                  as four 16 x 16 accumulators; K goes from memory straight into the A operand (each element is used once per draw
//                  group), the 64 x 64 tile of U through LDS, shared by the four waves
//   k_bs_cw        cw_t = sum_i w_{i,t}: one wave per draw, lane j adds rows j, j + 64, ... ascending, then the xor butterfly
//   k_bs_colstats  mu_j and d_j of every staged column, by the GRM builder's own statistics (ngp_grm_stats.h)
//   k_bs_cols      R[j,t] = sum_i z_ij w_{i,t} on the matrix cores, then beta = d_j (R - mu_j cw_t) and its sums over the draws in registers
// The accumulator conventions are those of k_grm_syrk (ngp_dense.h): lane l supplies A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15],
// the core adds the four products one after the other, k ascending; D: lane l, register v holds row (l >> 4) + 4 v, column l & 15.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#ifdef NGP_BACKSOLVE_KERNELS
#include "ngp_grm_stats.h"
#endif

namespace ngp {

// the launches (ngp_backsolve_inst.hip); type: 0 f64, 1 f32, 2 u8 genotypes
hipError_t backsolve_store(long long q, const double *u, double *dst, const unsigned *abort_w, hipStream_t stream);
hipError_t backsolve_kw(const double *K, long long ld, long long q, const double *U, long long T, double *W, double *cw, hipStream_t stream);
hipError_t backsolve_cw(const double *W, long long q, long long T, double *cw, hipStream_t stream);  // k_bs_cw alone, over a W formed elsewhere (ngp_apy.h)
struct BsCols {
    int type, method;         // genotype type; GRM method 1 / 2
    const void *src;          // the staged chunk: nc raw columns of N rows, leading dimension ld (elements)
    long long N, ld, nc, P;   // P: all columns of the GRM (method 2's divisor)
    double sum2pq;            // method 1: sum of 2 p q over all columns of the GRM
    const double *W, *cw;     // N x T (column-major, leading dimension N), T
    long long T;
    double *mu, *dj;          // nc scratch entries
    unsigned *bad;            // [0] a non-finite genotype, [1] smallest monomorphic column + 1 under method 2 (as k_grm_cols)
    double *sum, *sumsq;      // the chunk's first column
};
hipError_t backsolve_columns(const BsCols &c, hipStream_t stream);
// k_bs_cols over the rows of a relationship block in the place of genotype columns (ngp_gpred.h): Ct is N x Nc with leading dimension N,
// mu0 holds Nc zeros and d1 Nc ones, so that sum[c] = sum_t m_ct and sumsq[c] = sum_t m_ct^2 with m_ct = sum_i Ct[i, c] W[i, t], k_bs_cols' chain
hipError_t backsolve_project(const double *Ct, long long N, long long Nc, const double *W, long long T, const double *cw, const double *mu0, const double *d1,
                             double *sum, double *sumsq, hipStream_t stream);

#ifdef NGP_BACKSOLVE_KERNELS

#pragma clang fp contract(off)

typedef double bs_d4 __attribute__((ext_vector_type(4)));
#define NGP_BS_US 68  // LDS stride (doubles) of one draw's 64 k-values in k_bs_kw: lanes (cc, rr) read banks 8 cc + 2 rr
#define NGP_BS_WS 65  // LDS stride (doubles) of one row's 64 draws in k_bs_cols: lanes (cc, rr) read banks 32 rr + 2 cc

__global__ __launch_bounds__(256) void k_bs_store(long long q, const double *__restrict__ u, double *__restrict__ dst, const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    const long long l = (long long)blockIdx.x * 256 + threadIdx.x;
    if (l < q) dst[l] = u[l];
}

// W[i, t] = sum_k K[i, k] U[k, t], k ascending in fours.  grid (ceil(q / 64), ceil(T / 64)), 256 threads.  K is symmetric: the A operand
// K[i0 + 16 s + cc][k] is read as K[k][i0 + 16 s + cc], sixteen consecutive doubles per quarter wave.  Rows and k >= q and draws >= T are
// zeros by predicated loads: nothing beyond K's q x q entries or U's T columns is read.
__global__ __launch_bounds__(256) void k_bs_kw(const double *__restrict__ K, long long ld, long long q, const double *__restrict__ U, long long T,
                                               double *__restrict__ W) {
    __shared__ double sU[64 * NGP_BS_US];
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, rr = l >> 4, cc = l & 15;
    const long long i0 = 64LL * blockIdx.x, t0 = 64LL * blockIdx.y;
    bs_d4 acc[4];
#pragma unroll
    for (int s = 0; s < 4; s++) acc[s] = bs_d4{0.0, 0.0, 0.0, 0.0};
    for (long long k0 = 0; k0 < q; k0 += 64) {
        double a[4][16];  // the K tile of this lane: in flight while the U tile is staged
#pragma unroll
        for (int kb = 0; kb < 16; kb++) {
            const long long k = k0 + 4 * kb + rr;
#pragma unroll
            for (int s = 0; s < 4; s++) {
                const long long r = i0 + 16 * s + cc;
                a[s][kb] = (k < q && r < q) ? K[(size_t)k * (size_t)ld + (size_t)r] : 0.0;
            }
        }
        __syncthreads();  // (the tile of the step before has been read)
        for (int e = tid; e < 64 * 64; e += 256) {
            const int kk = e & 63, dd = e >> 6;
            const long long k = k0 + kk, t = t0 + dd;
            sU[dd * NGP_BS_US + kk] = (k < q && t < T) ? U[(size_t)k + (size_t)t * (size_t)q] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int kb = 0; kb < 16; kb++) {
            const double b = sU[(16 * w + cc) * NGP_BS_US + 4 * kb + rr];
#pragma unroll
            for (int s = 0; s < 4; s++) acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s][kb], b, acc[s], 0, 0, 0);
        }
    }
    const long long t = t0 + 16 * w + cc;
    if (t < T) {
#pragma unroll
        for (int s = 0; s < 4; s++)
#pragma unroll
            for (int v = 0; v < 4; v++) {
                const long long r = i0 + 16 * s + rr + 4 * v;
                if (r < q) W[(size_t)r + (size_t)t * (size_t)q] = acc[s][v];
            }
    }
}

__global__ __launch_bounds__(64) void k_bs_cw(const double *__restrict__ W, long long q, double *__restrict__ cw) {
    const int lane = threadIdx.x;
    const double *col = W + (size_t)blockIdx.x * (size_t)q;
    double acc = 0.0;
    for (long long i = lane; i < q; i += 64) acc = acc + col[i];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off);
    if (lane == 0) cw[blockIdx.x] = acc;
}

// one wave per staged column: mu_j = 2 p_j and the weight d_j = 1 / sum 2 p q (method 1), 1 / (P 2 p_j q_j) (method 2)
template <typename TIn>
__global__ __launch_bounds__(64) void k_bs_colstats(const TIn *__restrict__ src, long long N, long long ld, int method, double P, double sum2pq,
                                                    double *__restrict__ mu, double *__restrict__ dj, unsigned *__restrict__ bad) {
    const long long c = blockIdx.x;
    const int lane = threadIdx.x;
    double mean, tp;
    bool nf;
    grm_col_stats<TIn>(src + (size_t)c * (size_t)ld, N, lane, mean, tp, nf);
    if (nf) atomicOr(&bad[0], 1u);
    if (lane != 0) return;
    double d;
    if (method == 2) {
        if (!(tp > 0.0)) atomicMin(&bad[1], (unsigned)c + 1u);
        const double t = P * tp;
        d = 1.0 / t;
    } else d = 1.0 / sum2pq;
    mu[c] = mean;
    dj[c] = d;
}

// sixteen consecutive rows i .. i + 15 of one column as doubles; rows >= N (and every row of a column beyond the chunk) are zeros
template <typename TIn>
__device__ __forceinline__ void bs_load16(const TIn *__restrict__ col, bool on, long long i, long long N, double (&z)[16]) {
    if (on && i + 15 < N) {
#pragma unroll
        for (int k = 0; k < 16; k++) z[k] = (double)col[i + k];
    } else {
#pragma unroll
        for (int k = 0; k < 16; k++) z[k] = (on && i + k < N) ? (double)col[i + k] : 0.0;
    }
}
// bytes: four genotypes per load where the sixteen lie inside the column and on a dword boundary
template <>
__device__ __forceinline__ void bs_load16<uint8_t>(const uint8_t *__restrict__ col, bool on, long long i, long long N, double (&z)[16]) {
    if (on && i + 15 < N && (((uintptr_t)(col + i)) & 3u) == 0u) {
        const unsigned *p = (const unsigned *)(col + i);
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const unsigned x = p[d];
#pragma unroll
            for (int b = 0; b < 4; b++) z[4 * d + b] = (double)((x >> (8 * b)) & 0xFFu);
        }
    } else {
#pragma unroll
        for (int k = 0; k < 16; k++) z[k] = (on && i + k < N) ? (double)col[i + k] : 0.0;
    }
}

// One workgroup per 64 staged columns, 256 threads; wave w owns the columns 16 w .. 16 w + 15 of the tile.  For every group of 64 draws
// the workgroup walks N in tiles of 64 rows: lane (cc, rr) converts the sixteen genotypes z[kb] = Z[i0 + 16 rr + kb][its column cc] in
// registers (the A operand of step kb), the 64 x 64 tile of W goes through LDS once for the four waves (B of step kb, draw group g:
// W[i0 + 16 rr + kb][16 g + cc]), four 16-column x 16-draw accumulators per wave.  Behind the walk, in registers:
//   mc = mu_j * cw_t;  r = R - mc;  beta = d_j * r;  s1 = s1 + beta;  b2 = beta * beta;  s2 = s2 + b2
// draw groups ascending; then the butterfly over the sixteen lanes of a column (xor 8, 4, 2, 1).  A column belongs to one wave: plain
// stores, no atomics.  The genotype tile is read again for every group of 64 draws -- from the cache: 64 columns x N rows.
template <typename TIn>
__global__ __launch_bounds__(256) void k_bs_cols(const TIn *__restrict__ src, long long N, long long ld, long long nc, const double *__restrict__ W,
                                                 long long T, const double *__restrict__ cw, const double *__restrict__ mu,
                                                 const double *__restrict__ dj, double *__restrict__ sum, double *__restrict__ sumsq) {
    __shared__ double sW[64 * NGP_BS_WS];
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, rr = l >> 4, cc = l & 15;
    const long long jA = 64LL * blockIdx.x + 16 * w + cc;  // the column this lane feeds into the A operand
    const bool onA = jA < nc;
    const TIn *col = src + (size_t)(onA ? jA : 0) * (size_t)ld;
    double s1[4], s2[4], m[4], d[4];
#pragma unroll
    for (int v = 0; v < 4; v++) {  // the columns whose results this lane holds (D layout)
        const long long j = 64LL * blockIdx.x + 16 * w + rr + 4 * v;
        s1[v] = 0.0; s2[v] = 0.0;
        m[v] = (j < nc) ? mu[j] : 0.0;
        d[v] = (j < nc) ? dj[j] : 0.0;
    }
    for (long long t0 = 0; t0 < T; t0 += 64) {
        bs_d4 acc[4];
#pragma unroll
        for (int g = 0; g < 4; g++) acc[g] = bs_d4{0.0, 0.0, 0.0, 0.0};
        for (long long i0 = 0; i0 < N; i0 += 64) {
            double z[16];
            bs_load16<TIn>(col, onA, i0 + 16 * rr, N, z);
            __syncthreads();  // (the tile of the step before has been read)
            for (int e = tid; e < 64 * 64; e += 256) {
                const int ii = e & 63, dd = e >> 6;
                const long long i = i0 + ii, t = t0 + dd;
                sW[ii * NGP_BS_WS + dd] = (i < N && t < T) ? W[(size_t)i + (size_t)t * (size_t)N] : 0.0;
            }
            __syncthreads();
#pragma unroll
            for (int kb = 0; kb < 16; kb++)
#pragma unroll
                for (int g = 0; g < 4; g++)
                    acc[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(z[kb], sW[(16 * rr + kb) * NGP_BS_WS + 16 * g + cc], acc[g], 0, 0, 0);
        }
#pragma unroll
        for (int g = 0; g < 4; g++) {
            const long long t = t0 + 16 * g + cc;
            const double c = (t < T) ? cw[t] : 0.0;
#pragma unroll
            for (int v = 0; v < 4; v++) {
                const double mc = m[v] * c;
                const double r = acc[g][v] - mc;
                const double beta = (t < T) ? d[v] * r : 0.0;
                s1[v] = s1[v] + beta;
                const double b2 = beta * beta;
                s2[v] = s2[v] + b2;
            }
        }
    }
#pragma unroll
    for (int v = 0; v < 4; v++) {
#pragma unroll
        for (int off = 8; off >= 1; off >>= 1) {
            s1[v] = s1[v] + __shfl_xor(s1[v], off);
            s2[v] = s2[v] + __shfl_xor(s2[v], off);
        }
        const long long j = 64LL * blockIdx.x + 16 * w + rr + 4 * v;
        if (cc == 0 && j < nc) { sum[j] = s1[v]; sumsq[j] = s2[v]; }
    }
}

#endif  // NGP_BACKSOLVE_KERNELS

}  // namespace ngp
