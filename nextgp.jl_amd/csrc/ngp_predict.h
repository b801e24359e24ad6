// Prediction of new individuals: g = X_new beta of every kept draw, accumulated per marker set ("Prediction";
// section 4.3).  Two kernels behind the sweep and behind k_post, in kept iterations only; neither is part of the sweep's translation
// units.  The prediction panel lies in the tile layout of the training panel (tile_off / tile8_off) with a plan of its own: shards of
// R <= NGP_PRED_MAXR rows.
//
// The arithmetic is fixed by NGP_BLK and NGP_PRED_CB alone -- never by the grid, the chains in the launch or the device:
//   chunk c of set s = the panel's 64-column blocks [tb0 + c CB, tb0 + (c + 1) CB), tb0 = col0(s) / 64, cut to the set's columns;
//   inside a chunk  acc = fma((double)x_ij, beta_j, acc), j ascending, from 0.0;
//   g_s(i) = the chunk sums added in ascending c, from 0.0;  byte tiles: the code sums and sum_j m_j beta_j formed this way each,
//   subtracted once;  g(i) = the g_s(i) added in set order, from 0.0.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ngp_common.h"

namespace ngp {

#define NGP_PRED_CB 32     // 64-column blocks per chunk: chunks of 2048 panel columns
#define NGP_PRED_MAXR 256  // rows per shard of the prediction panel at most (a multiple of 16): one row per thread
#define NGP_PRED_QS 1040   // LDS stride of one 1-KiB row group of a tile (4 rows of floats or 16 rows of bytes x 64 columns) + 16: a wave's
                           // reads of one column fall on 64 different banks
#define NGP_PRED_MAXK 8    // chains one launch serves (NGP_MAXC)

// one work item: the columns [j0, j1) of marker set `set` inside the blocks [t0, t1) (one chunk of the set)
struct PredItem { int set, t0, t1, pad; long long j0, j1; };
// one chain of a launch: its effects, the chunk partials [items][Lp] (and [items] for the mean term), its sums and its last g, [nsets + 1][Np] each
struct PredChain { const double *beta; double *part, *mpart, *sum, *sum2, *last; };
struct PredArgs { PredChain c[NGP_PRED_MAXK]; };

inline size_t predict_lds_bytes(int R, int K, bool u8) { return (size_t)(u8 ? R / 16 : R / 4) * NGP_PRED_QS + (size_t)K * NGP_BLK * sizeof(double); }

// workgroup (item, shard): streams the item's tiles of the shard once -- 16-byte loads in the order they lie in memory, the next
// block's in flight while this one is summed out of LDS -- and carries one fp64 chain per row and chain of the launch.  beta of the
// block is staged in LDS beside the tile.  Writes part[item][row]; no atomics.
template <int K, bool U8>
__global__ __launch_bounds__(256) void k_predict(const void *__restrict__ tiles, const double *__restrict__ pmean, const PredItem *__restrict__ items,
                                                 PredArgs A, int R, int S, long long Lp, const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;  // an earlier sweep of this call gave up: its iteration runs again and must not count twice
    extern __shared__ __attribute__((aligned(16))) unsigned char pred_lds[];
    constexpr int NV = U8 ? 4 : 16;  // 16-byte vectors of a tile per thread at most (R = 256)
    const PredItem it = items[blockIdx.x];
    const int s = blockIdx.y, tid = threadIdx.x;
    const int nvec = (U8 ? R / 16 : R / 4) * NGP_BLK;
    const size_t tile_bytes = U8 ? (size_t)R * NGP_BLK : (size_t)R * NGP_BLK * 4;
    unsigned char *xs = pred_lds;
    double *bs = (double *)(pred_lds + (size_t)(U8 ? R / 16 : R / 4) * NGP_PRED_QS);
    double acc[K];
#pragma unroll
    for (int k = 0; k < K; k++) acc[k] = 0.0;
    uint4 pre[NV];  // the next block's share of this thread, in registers (every index below is a constant after unrolling)
    {
        const uint4 *src = (const uint4 *)((const unsigned char *)tiles + ((size_t)it.t0 * S + s) * tile_bytes);
#pragma unroll
        for (int n = 0; n < NV; n++) pre[n] = (tid + 256 * n < nvec) ? src[tid + 256 * n] : make_uint4(0u, 0u, 0u, 0u);
    }
    for (int t = it.t0; t < it.t1; t++) {
        __syncthreads();  // the last block's reads are done
#pragma unroll
        for (int n = 0; n < NV; n++) {
            const int v = tid + 256 * n;
            if (v < nvec) *(uint4 *)(xs + (size_t)(v >> 6) * NGP_PRED_QS + (size_t)(v & 63) * 16) = pre[n];
        }
#pragma unroll
        for (int k = 0; k < K; k++)  // wave k mod 4 stages chain k's 64 effects (columns of another set: zero, and never read)
            if ((tid >> 6) == (k & 3)) {
                const long long j = (long long)t * NGP_BLK + (tid & 63);
                bs[k * NGP_BLK + (tid & 63)] = (j >= it.j0 && j < it.j1) ? A.c[k].beta[j] : 0.0;
            }
        __syncthreads();
        if (t + 1 < it.t1) {  // in flight while this block is summed
            const uint4 *src = (const uint4 *)((const unsigned char *)tiles + ((size_t)(t + 1) * S + s) * tile_bytes);
#pragma unroll
            for (int n = 0; n < NV; n++) pre[n] = (tid + 256 * n < nvec) ? src[tid + 256 * n] : make_uint4(0u, 0u, 0u, 0u);
        }
        if (tid < R) {
            const int c0 = (int)max(it.j0 - (long long)t * NGP_BLK, 0ll), c1 = (int)min(it.j1 - (long long)t * NGP_BLK, (long long)NGP_BLK);
            const unsigned char *row = U8 ? xs + (size_t)(tid >> 4) * NGP_PRED_QS + (tid & 15) : xs + (size_t)(tid >> 2) * NGP_PRED_QS + (size_t)(tid & 3) * 4;
            if (c0 == 0 && c1 == NGP_BLK) {  // a whole block of the set: the same operations, unrolled
#pragma unroll 16
                for (int c = 0; c < NGP_BLK; c++) {
                    const double x = U8 ? (double)row[c * 16] : (double)*(const float *)(row + c * 16);
#pragma unroll
                    for (int k = 0; k < K; k++) acc[k] = __builtin_fma(x, bs[k * NGP_BLK + c], acc[k]);
                }
            } else {
                for (int c = c0; c < c1; c++) {
                    const double x = U8 ? (double)row[c * 16] : (double)*(const float *)(row + c * 16);
#pragma unroll
                    for (int k = 0; k < K; k++) acc[k] = __builtin_fma(x, bs[k * NGP_BLK + c], acc[k]);
                }
            }
        }
    }
    if (tid < R) {
#pragma unroll
        for (int k = 0; k < K; k++) A.c[k].part[(size_t)blockIdx.x * Lp + (size_t)s * R + tid] = acc[k];
    }
    if (U8 && s == 0) {  // byte tiles: the chunk's sum_j m_j beta_j, one lane per chain, the chain of operations of a row's code sum
#pragma unroll
        for (int k = 0; k < K; k++)
            if (tid == k) {
                double am = 0.0;
                for (long long j = it.j0; j < it.j1; j++) am = __builtin_fma(pmean[j], A.c[k].beta[j], am);
                A.c[k].mpart[blockIdx.x] = am;
            }
    }
}

// thread (row i, chain blockIdx.y): the chunk partials of every set in ascending order, the sets in their order, then the sums
template <bool U8>
__global__ __launch_bounds__(256) void k_predict_combine(PredArgs A, const int *__restrict__ set_item0, int nsets, long long Np, long long Lp,
                                                         const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= Np) return;
    const PredChain C = A.c[blockIdx.y];
    double tot = 0.0;
    for (int s = 0; s < nsets; s++) {
        double g = 0.0, gm = 0.0;
        for (int e = set_item0[s]; e < set_item0[s + 1]; e++) {
            g = g + C.part[(size_t)e * Lp + i];
            if (U8) gm = gm + C.mpart[e];
        }
        if (U8) g = g - gm;
        C.sum[(size_t)s * Np + i] += g;
        C.sum2[(size_t)s * Np + i] += g * g;
        C.last[(size_t)s * Np + i] = g;
        tot = tot + g;
    }
    C.sum[(size_t)nsets * Np + i] += tot;
    C.sum2[(size_t)nsets * Np + i] += tot * tot;
    C.last[(size_t)nsets * Np + i] = tot;
}

}  // namespace ngp
