// Genomic variance of every kept draw: var_i (X beta)_i per window, per marker set and in all ("Genomic variance";
// section 4.3).  Six kernels behind k_post, in kept iterations only, compiled in a translation unit of their own (ngp_genvar_inst.hip
// defines NGP_GENVAR_KERNELS; ngp_api.hip sees the structures and genvar_launch only).  They read the TRAINING tiles (tile_off /
// tile8_off, [t][s][R x 64]) once per pass, however many chains the launch serves.
//
// The arithmetic is fixed by the windows, by NGP_BLK and by NGP_GV_ITEM_COLS alone -- never by the plan (R, S, V, streamer), the
// engine, the chains in the launch or the device:
//   segments of a set = its windows and the gaps between and around them (a gap cut into pieces of NGP_GV_ITEM_COLS columns from its
//   start), ascending;  inside a segment  acc = fma((double)x_ij, beta_j, acc), j ascending, from 0.0  (byte tiles: the code sum, and
//   sum_j m_j beta_j formed the same way, subtracted once per segment);  items = runs of whole segments of at most NGP_GV_ITEM_COLS
//   columns (a longer window is an item of its own);  item value = its segment values added in ascending order from 0.0;  g_s(i) = the
//   item values added in ascending order from 0.0;  g(i) = the g_s(i) added in set order from 0.0.
//   Sums over individuals: every term g 2^(45 - E) and (g g) 2^(46 - 2E) is rounded to an integer (fx_from_f64) and added as a 64-bit
//   integer -- order-free -- with E per slot and draw from sum_j |beta_j| and the panel's largest x'x (gv_exponent).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ngp_common.h"

namespace ngp {

#define NGP_GV_ITEM_COLS 2048  // columns of a work item (and of a piece of a gap) at most
#define NGP_GV_ROWS 256        // rows one workgroup takes: one row per thread.  The tiles of one block are the row groups of ALL shards one
                               // behind the other ([t][s][R x 64], R a multiple of the group), so any 256 consecutive rows of the padded
                               // row space L = R S are contiguous bytes of every block, whatever R is: short shards fill the workgroup
                               // as well as tall ones, and shards of more than 256 rows need no second row per thread
#define NGP_GV_QS 1040         // LDS stride of one 1-KiB row group of a tile (4 rows of floats or 16 rows of bytes x 64 columns) + 16
#define NGP_GV_MAXK 8          // chains one launch serves (NGP_MAXC)
#define NGP_GV_EMAX 400        // |E| at most: every scale 2^(46 - 2E) is a normal double
#define NGP_ABORT_GENVAR 9u    // abort word: a term of the variance sums left its fixed-point range (non-finite effects)

struct GvSeg { long long j0, j1; int slot, pad; };          // panel columns [j0, j1); slot: its window's, -1 for a gap
struct GvItem { int set, g0, g1, pad; long long j0, j1; };  // the segments [g0, g1) of one set: panel columns [j0, j1)
// one chain of a launch: its effects and scalars; item values [items][L]; mean term and sum |beta| per segment; E per slot; integer
// partials of the windows [workgroup column][nwin][2] and of the sets and the total [row block][nsets + 1][2]; the accumulators
// [6][nslots] (sum V | sum V^2 | sum q | sum q^2 | count q > threshold | last V), sum r | sum r^2, the trace [rows][nslots + 1] and the
// counters (kept draws seen | row of the pass under way)
struct GvChain {
    const double *beta;
    const DScal *scal;
    double *part, *segm, *sega;
    int *slot_e;
    long long *qw, *qs;
    double *acc, *ratio, *trace;
    long long *cnt;
};
struct GvArgs { GvChain c[NGP_GV_MAXK]; };

inline size_t genvar_lds_bytes(int K, bool u8) {
    return (size_t)(u8 ? NGP_GV_ROWS / 16 : NGP_GV_ROWS / 4) * NGP_GV_QS + (size_t)K * NGP_BLK * sizeof(double) + (size_t)2 * 4 * K * 2 * sizeof(long long);
}

// smallest k with |x| < 2^k for a finite x of normal size; zero and subnormals: -1022; non-finite: 4000
__host__ __device__ inline int gv_ilog(const double x) {
    union { double d; unsigned long long u; } v;
    v.d = x;
    const int ef = (int)((v.u >> 52) & 0x7ffull);
    if (ef == 0x7ff) return 4000;
    if (ef == 0) return -1022;
    return ef - 1022;
}
// 2^ex > max |x_ij| over the live rows (k_genvar_xmax: once per panel and chain, when the tables are built)
__host__ __device__ inline int gv_xexp(const double xmax) { return gv_ilog(xmax); }
// E of a slot from a = sum |beta_j| over its columns: |g(i)| <= max|x| a < 2^(E - 1), rounding of the sums included
__host__ __device__ inline int gv_exponent(const int ex, const double a) {
    int e = ex + gv_ilog(a) + 1;
    if (e < -NGP_GV_EMAX) e = -NGP_GV_EMAX;
    if (e > NGP_GV_EMAX) e = NGP_GV_EMAX;
    return e;
}

// One pass for the n chains of A (ngp_genvar_inst.hip: the kernels below live in a translation unit of their own, so the device code
// of the API unit and of the sweep units is what it was without them).  thr / trace_rows: each chain's own.
struct GvLaunch {
    GvArgs A;
    int n, u8;
    const void *tiles;
    const double *mean;
    const GvSeg *segs;
    const GvItem *items;
    const int *slot_seg, *set_seg0, *set_item0;
    int nseg, nitems, nsets, nwin, nslots, ex, ncol_w, nblk_r;
    long long N, L;
    unsigned *abort_w;
    hipStream_t stream;
    double thr[NGP_GV_MAXK];
    long long trace_rows[NGP_GV_MAXK];
};
// hipSuccess, or why a launch of the pass was not made (more than NGP_GV_MAXK chains; a launch error)
hipError_t genvar_launch(const GvLaunch &q);
// k_genvar needs more dynamic LDS than the 64-KiB default: raised once, for every instantiation, when the pass is switched on
hipError_t genvar_prepare();
// max over the live rows i < N and all columns of |x_ij| (fp32 tiles) or |(double)code_ij - m_j| (byte tiles) into *out, as the bit
// pattern of a non-negative double (an integer maximum: order-free); *out must be zero before
hipError_t genvar_xmax(const void *tiles, const double *mean, int u8, long long N, long long L, long long nblk, unsigned long long *out, hipStream_t stream);
#define NGP_GV_MAXN (1ll << 18)  // individuals at most: 2^18 terms below 2^44 stay below 2^62 (ngp_enable_genomic_variance refuses more)

#ifdef NGP_GENVAR_KERNELS
// the two fixed-point terms of one value (0 for a masked row); *bad: the value is outside the range its E promised
__device__ inline void gv_terms(const double v, const int e, long long *q1, long long *q2, bool *bad) {
    double a1 = v * fx_pow2(45 - e);
    const double sq = v * v;
    double a2 = sq * fx_pow2(46 - 2 * e);
    if (!(__builtin_fabs(a1) <= 0x1p44 && a2 <= 0x1p44)) { *bad = true; a1 = 0.0; a2 = 0.0; }
    *q1 = fx_from_f64(a1);
    *q2 = fx_from_f64(a2);
}

__device__ inline long long gv_wave_sum(long long q) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) q += __shfl_down(q, o);
    return q;
}

// thread (row i of the padded row space, block blockIdx.x of the panel): the largest |x_ij| of its 64 elements; one atomic max per wave
template <bool U8>
__global__ __launch_bounds__(256) void k_genvar_xmax(const void *__restrict__ tiles, const double *__restrict__ mean, long long N, long long L,
                                                     unsigned long long *out) {
    const long long i = (long long)blockIdx.y * 256 + threadIdx.x, t = blockIdx.x;
    double m = 0.0;
    if (i < N) {
        if (U8) {
            const unsigned char *p = (const unsigned char *)tiles + (size_t)t * L * NGP_BLK + (size_t)(i >> 4) * 1024 + (size_t)(i & 15);
            for (int j = 0; j < NGP_BLK; j++) m = fmax(m, __builtin_fabs((double)p[j * 16] - mean[t * NGP_BLK + j]));
        } else {
            const float *p = (const float *)tiles + (size_t)t * L * NGP_BLK + (size_t)(i >> 2) * 256 + (size_t)(i & 3);
            for (int j = 0; j < NGP_BLK; j++) m = fmax(m, __builtin_fabs((double)p[j * 4]));
        }
    }
    unsigned long long b = (unsigned long long)__double_as_longlong(m);  // (non-negative doubles order as their bit patterns)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long c = (unsigned long long)__shfl_down((long long)b, o);
        b = c > b ? c : b;
    }
    if ((threadIdx.x & 63) == 0 && b != 0ull) atomicMax(out, b);
}

// wave (segment blockIdx.x, chain blockIdx.y): the segment's sum_j m_j beta_j (byte tiles) and sum_j |beta_j|, j ascending, from 0.0.
// The lanes fetch 64 columns at a time into LDS; lane 0 adds them in order (the loads of a chunk do not wait for one another).
template <bool U8>
__global__ __launch_bounds__(64) void k_genvar_prep(const GvSeg *__restrict__ segs, const double *__restrict__ mean, GvArgs A,
                                                    const unsigned *__restrict__ abort_w) {
    if (*abort_w != 0u) return;
    __shared__ double sb[NGP_BLK], sm[NGP_BLK];
    const int g = blockIdx.x, lane = threadIdx.x;
    const GvChain C = A.c[blockIdx.y];
    const GvSeg sg = segs[g];
    double am = 0.0, ab = 0.0;
    for (long long j0 = sg.j0; j0 < sg.j1; j0 += NGP_BLK) {
        const int n = (int)min((long long)NGP_BLK, sg.j1 - j0);
        __syncthreads();
        if (lane < n) {
            sb[lane] = C.beta[j0 + lane];
            if (U8) sm[lane] = mean[j0 + lane];
        }
        __syncthreads();
        if (lane == 0)
            for (int c = 0; c < n; c++) {
                const double b = sb[c];
                if (U8) am = __builtin_fma(sm[c], b, am);
                ab = ab + __builtin_fabs(b);
            }
    }
    if (lane == 0) { C.segm[g] = am; C.sega[g] = ab; }
}

// thread (slot, chain blockIdx.y): E of the slot from the segments' sums of |beta|, added in ascending order (sets in set order)
__global__ __launch_bounds__(256) void k_genvar_scale(const int *__restrict__ slot_seg, const int *__restrict__ set_seg0, int nwin, int nsets, int ex,
                                                      GvArgs A, const unsigned *__restrict__ abort_w) {
    if (*abort_w != 0u) return;
    const int slot = blockIdx.x * 256 + threadIdx.x;
    if (slot >= nwin + nsets + 1) return;
    const GvChain C = A.c[blockIdx.y];
    double a;
    if (slot < nwin) a = C.sega[slot_seg[slot]];
    else {
        const int s0 = slot < nwin + nsets ? slot - nwin : 0, s1 = slot < nwin + nsets ? slot - nwin + 1 : nsets;
        double tot = 0.0;
        a = 0.0;
        for (int s = s0; s < s1; s++) {
            a = 0.0;
            for (int g = set_seg0[s]; g < set_seg0[s + 1]; g++) a = a + C.sega[g];
            tot = tot + a;
        }
        if (slot == nwin + nsets) a = tot;
    }
    C.slot_e[slot] = gv_exponent(ex, a);
}

// workgroup (item, 256 rows of the padded row space): streams the item's tiles of those rows once -- 16-byte loads in the order they lie in
// memory, the next block's in flight while this one is summed out of LDS -- and carries one fp64 chain per row and chain of the
// launch.  At the end of a window the rows' values go to fixed point and are summed as integers (wave shuffles, then LDS): one pair
// per (window, workgroup column, chain), written plainly.  Writes the item values part[item][row]; no atomics but the abort word's.
template <int K, bool U8>
__global__ __launch_bounds__(256) void k_genvar(const void *__restrict__ tiles, const GvItem *__restrict__ items, const GvSeg *__restrict__ segs, GvArgs A,
                                                long long N, long long L, int nwin, unsigned *abort_w) {
    if (*abort_w != 0u) return;  // an earlier sweep of this call gave up: its iteration runs again and must not count twice
    extern __shared__ __attribute__((aligned(16))) unsigned char gv_lds[];
    constexpr int NV = U8 ? 4 : 16;      // 16-byte vectors of a tile per thread at most (256 rows)
    constexpr int NGRP = U8 ? NGP_GV_ROWS / 16 : NGP_GV_ROWS / 4;
    const GvItem it = items[blockIdx.x];
    const int vs = blockIdx.y, tid = threadIdx.x;
    const int rows = (int)min(L - (long long)vs * NGP_GV_ROWS, (long long)NGP_GV_ROWS);  // (L is a multiple of the row group)
    const int nvec = (U8 ? rows / 16 : rows / 4) * NGP_BLK;
    const size_t blk_bytes = U8 ? (size_t)L * NGP_BLK : (size_t)L * NGP_BLK * 4;          // one block of the panel: every shard's tile
    const size_t sub_off = (size_t)vs * NGP_GV_ROWS * NGP_BLK * (U8 ? 1 : 4);
    unsigned char *xs = gv_lds;
    double *bs = (double *)(gv_lds + (size_t)NGRP * NGP_GV_QS);
    long long *red = (long long *)(bs + K * NGP_BLK);  // [2 buffers][4 waves][K][2]
    const long long i = (long long)vs * NGP_GV_ROWS + tid;
    const bool live = tid < rows && i < N;  // padding rows contribute nothing (byte tiles hold code 0 there: -sum m beta otherwise)
    double acc[K], gi[K];
#pragma unroll
    for (int k = 0; k < K; k++) { acc[k] = 0.0; gi[k] = 0.0; }
    const int t0 = (int)(it.j0 / NGP_BLK), t1 = (int)((it.j1 + NGP_BLK - 1) / NGP_BLK);
    uint4 pre[NV];  // the next block's share of this thread, in registers (every index below is a constant after unrolling)
    {
        const uint4 *src = (const uint4 *)((const unsigned char *)tiles + (size_t)t0 * blk_bytes + sub_off);
#pragma unroll
        for (int n = 0; n < NV; n++) pre[n] = (tid + 256 * n < nvec) ? src[tid + 256 * n] : make_uint4(0u, 0u, 0u, 0u);
    }
    int sg = it.g0, buf = 0;
    GvSeg cur = segs[sg];
    bool bad = false;
    for (int t = t0; t < t1; t++) {
        __syncthreads();  // the last block's reads are done
#pragma unroll
        for (int n = 0; n < NV; n++) {
            const int v = tid + 256 * n;
            if (v < nvec) *(uint4 *)(xs + (size_t)(v >> 6) * NGP_GV_QS + (size_t)(v & 63) * 16) = pre[n];
        }
#pragma unroll
        for (int k = 0; k < K; k++)  // wave k mod 4 stages chain k's 64 effects (columns outside the item: zero, and never read)
            if ((tid >> 6) == (k & 3)) {
                const long long j = (long long)t * NGP_BLK + (tid & 63);
                bs[k * NGP_BLK + (tid & 63)] = (j >= it.j0 && j < it.j1) ? A.c[k].beta[j] : 0.0;
            }
        __syncthreads();
        if (t + 1 < t1) {  // in flight while this block is summed
            const uint4 *src = (const uint4 *)((const unsigned char *)tiles + (size_t)(t + 1) * blk_bytes + sub_off);
#pragma unroll
            for (int n = 0; n < NV; n++) pre[n] = (tid + 256 * n < nvec) ? src[tid + 256 * n] : make_uint4(0u, 0u, 0u, 0u);
        }
        const long long jb = (long long)t * NGP_BLK;
        const unsigned char *row = U8 ? xs + (size_t)(tid >> 4) * NGP_GV_QS + (tid & 15) : xs + (size_t)(tid >> 2) * NGP_GV_QS + (size_t)(tid & 3) * 4;
        while (true) {  // the segments that touch this block (the same for every thread of the workgroup)
            const int c0 = (int)max(cur.j0 - jb, 0ll), c1 = (int)min(cur.j1 - jb, (long long)NGP_BLK);
            if (tid < rows) {
                if (c0 == 0 && c1 == NGP_BLK) {  // a whole block of the segment: the same operations, unrolled
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
            if (cur.j1 > jb + NGP_BLK) break;  // the segment goes on in the next block
            // the segment ends here: its value joins the item's, and a window's goes to the integer sums
            double v[K];
#pragma unroll
            for (int k = 0; k < K; k++) {
                v[k] = U8 ? acc[k] - A.c[k].segm[sg] : acc[k];
                gi[k] = gi[k] + v[k];
                acc[k] = 0.0;
            }
            if (cur.slot >= 0) {
                long long *rb = red + (size_t)buf * 4 * K * 2;
#pragma unroll
                for (int k = 0; k < K; k++) {
                    long long q1, q2;
                    gv_terms(live ? v[k] : 0.0, A.c[k].slot_e[cur.slot], &q1, &q2, &bad);
                    q1 = gv_wave_sum(q1);
                    q2 = gv_wave_sum(q2);
                    if ((tid & 63) == 0) { rb[((tid >> 6) * K + k) * 2] = q1; rb[((tid >> 6) * K + k) * 2 + 1] = q2; }
                }
                __syncthreads();
#pragma unroll
                for (int k = 0; k < K; k++)
                    if ((tid >> 1) == k) {
                        const int c = tid & 1;
                        A.c[k].qw[((size_t)vs * nwin + cur.slot) * 2 + c] = ((rb[(0 * K + k) * 2 + c] + rb[(1 * K + k) * 2 + c]) + rb[(2 * K + k) * 2 + c]) + rb[(3 * K + k) * 2 + c];
                    }
                buf ^= 1;  // (the next sum writes the other buffer: this one's reads end before the barrier after that)
            }
            if (++sg >= it.g1) break;
            cur = segs[sg];
            if (cur.j0 >= jb + NGP_BLK) break;  // the next segment starts in a later block
        }
    }
    if (tid < rows) {
#pragma unroll
        for (int k = 0; k < K; k++) A.c[k].part[(size_t)blockIdx.x * L + (size_t)(i)] = gi[k];
    }
    if (bad) atomicCAS(abort_w, 0u, NGP_ABORT_GENVAR);
}

// thread (row i, chain blockIdx.y): the item values of every set in ascending order, the sets in their order; their fixed-point
// terms summed over the 256 rows of the block: one pair per (set or total, row block, chain)
__global__ __launch_bounds__(256) void k_genvar_rows(GvArgs A, const int *__restrict__ set_item0, int nsets, int nwin, long long N, long long L,
                                                     unsigned *abort_w) {
    if (*abort_w != 0u) return;
    __shared__ long long red[2][4][2];
    const int tid = threadIdx.x;
    const long long i = (long long)blockIdx.x * 256 + tid;
    const bool live = i < N;
    const GvChain C = A.c[blockIdx.y];
    double tot = 0.0;
    bool bad = false;
    for (int s = 0; s <= nsets; s++) {
        double g = 0.0;
        if (s < nsets) {
            if (live)
                for (int e = set_item0[s]; e < set_item0[s + 1]; e++) g = g + C.part[(size_t)e * L + i];
            tot = tot + g;
        } else g = tot;
        long long q1, q2;
        gv_terms(live ? g : 0.0, C.slot_e[nwin + s], &q1, &q2, &bad);
        q1 = gv_wave_sum(q1);
        q2 = gv_wave_sum(q2);
        long long(*rb)[2] = red[s & 1];
        if ((tid & 63) == 0) { rb[tid >> 6][0] = q1; rb[tid >> 6][1] = q2; }
        __syncthreads();
        if (tid < 2) C.qs[((size_t)blockIdx.x * (nsets + 1) + s) * 2 + tid] = ((rb[0][tid] + rb[1][tid]) + rb[2][tid]) + rb[3][tid];
    }
    if (bad) atomicCAS(abort_w, 0u, NGP_ABORT_GENVAR);
}

// thread (slot, chain blockIdx.y): the integer partials of the slot added up, converted back once, V of the draw into last[slot]
__global__ __launch_bounds__(256) void k_genvar_var(GvArgs A, int nwin, int nsets, int ncol_w, int nblk_r, long long N, const unsigned *__restrict__ abort_w) {
    if (*abort_w != 0u) return;
    const int slot = blockIdx.x * 256 + threadIdx.x, nslots = nwin + nsets + 1;
    const GvChain C = A.c[blockIdx.y];
    if (slot == 0) C.cnt[1] = C.cnt[0];  // the row of this pass (k_genvar_acc advances cnt[0])
    if (slot >= nslots) return;
    long long q1 = 0, q2 = 0;
    if (slot < nwin)
        for (int v = 0; v < ncol_w; v++) { q1 += C.qw[((size_t)v * nwin + slot) * 2]; q2 += C.qw[((size_t)v * nwin + slot) * 2 + 1]; }
    else
        for (int b = 0; b < nblk_r; b++) { q1 += C.qs[((size_t)b * (nsets + 1) + (slot - nwin)) * 2]; q2 += C.qs[((size_t)b * (nsets + 1) + (slot - nwin)) * 2 + 1]; }
    const int e = C.slot_e[slot];
    const double s1 = fx_to_f64(q1) * fx_pow2(e - 45), s2 = fx_to_f64(q2) * fx_pow2(2 * e - 46);
    double t = s1 * s1;
    t = t / (double)N;
    const double d = s2 - t;
    const double v = d / (double)(N - 1);
    C.acc[(size_t)5 * nslots + slot] = v > 0.0 ? v : 0.0;
}

// thread (slot, chain blockIdx.y): q, the indicator and the sums of the slot; the last slot's thread also r and the draw counter
__global__ __launch_bounds__(256) void k_genvar_acc(GvArgs A, int nslots, double threshold, long long trace_rows, const unsigned *__restrict__ abort_w) {
    if (*abort_w != 0u) return;
    const int slot = blockIdx.x * 256 + threadIdx.x;
    if (slot >= nslots) return;
    const GvChain C = A.c[blockIdx.y];
    const size_t n = (size_t)nslots;
    const double V = C.acc[5 * n + slot], Vg = C.acc[5 * n + n - 1];
    const double q = Vg > 0.0 ? V / Vg : 0.0;
    const long long row = C.cnt[1];
    const double V2 = V * V, q2 = q * q;
    C.acc[slot] += V;
    C.acc[n + slot] += V2;
    C.acc[2 * n + slot] += q;
    C.acc[3 * n + slot] += q2;
    if (q > threshold) C.acc[4 * n + slot] += 1.0;
    if (row < trace_rows) C.trace[(size_t)row * (n + 1) + slot] = V;
    if (slot == nslots - 1) {
        const double den = Vg + C.scal->varE;
        const double r = den > 0.0 ? Vg / den : 0.0;
        const double r2 = r * r;
        C.ratio[0] += r;
        C.ratio[1] += r2;
        if (row < trace_rows) C.trace[(size_t)row * (n + 1) + n] = r;
        C.cnt[0] = row + 1;
    }
}

#endif  // NGP_GENVAR_KERNELS

}  // namespace ngp
