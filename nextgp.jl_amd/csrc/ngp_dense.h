// ngp_dense.h -- gfx950 kernels of GBLUP: the genomic relationship matrix (makeG, src/misc.jl:145-160) built on the matrix cores, and
// the Gauss-Seidel of a random-effect set whose K is a dense q x q matrix (sampleU, src/functions.jl:57-72, over iVarStr = inv(G),
// src/prepMatVec.jl:122-126).  DESIGN.md section 2, "Dense random-effect sets and the GRM", is the normative description of every
// summation order here; tests/ref_gblup.py restates the dense step operation by operation.  No FMA in the dense step (fp contract
// off, no __builtin_fma): every product and sum is rounded on its own.  The matrix core's own accumulation (four products added
// to the accumulator one after the other, rows ascending) is the only fused arithmetic, and only the GRM uses it.
//
// Dense random-effect set, per iteration, between k_rand_levels and k_rand_update (ngp_random.h), blocks of 64 levels:
//   k_dense_dhi     one wave per level: dhi_l = sum over c > l of K_lc u_c (last sweep's u), and the accumulator acc_l = 0.0
//   k_dense_block   one launch per block t, in block order on the chain's stream: every workgroup repeats the 64-step chain of
//                   block t from read-only inputs (acc, dhi, Yi, 1/lhs, tz, the diagonal block), workgroup 0 writes u, du and dlo
//                   of the block; then every workgroup adds K[rows, block t] u_new[block t] to acc of its own rows below the block
//   k_dense_var     u'Ku = sum_l u_l (K_ll u_l + 2 dlo_l) without a second pass over K, then varU as k_rand_var draws it
// K is read once per iteration: the upper triangle by k_dense_dhi, the lower one by the k_dense_block launches (8 q^2 bytes).
#pragma once
#include "ngp_kernels.h"
#include "ngp_random.h"

#pragma clang fp contract(off)

namespace ngp {

// scratch rows of a dense set beyond those of ngp_random.h
#define NGP_RS_ACC 5   // dlo accumulated over the blocks in front of a level's own
#define NGP_RS_DLO 6   // dlo_l of this sweep, complete (k_dense_var)
#define NGP_RS_ROWS_DENSE 7
#define NGP_DENSE_WG_ROWS 64  // rows below the block that one workgroup of k_dense_block updates (no influence on any sum)

// ------------------------------------------------------------------------------------------
// dhi_l = sum_{c > l} K_lc u_c with the u of the last sweep.  256 threads = 4 waves = 4 levels per workgroup.  Lane j of level l's wave
// adds the columns c = 64 m + j, m ascending from l / 64, c > l, c < q (from 0.0; each term one product, one sum); the 64 lane sums
// are combined by the butterfly of k_rand_levels.  Also clears acc_l.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dense_dhi(const double *__restrict__ K, long long ld, long long q, const double *__restrict__ u,
                                                   double *__restrict__ scr, const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    const int lane = threadIdx.x & 63;
    const long long l = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (l >= q) return;  // (uniform over the wave)
    const double *row = K + (size_t)l * (size_t)ld;
    double acc = 0.0;
    for (long long c = (l & ~63LL) + lane; c < q; c += 64) {
        if (c > l) {
            const double t = row[c] * u[c];
            acc = acc + t;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off);
    if (lane != 0) return;
    scr[NGP_RS_DHI * q + l] = acc;
    scr[NGP_RS_ACC * q + l] = 0.0;
}

// ------------------------------------------------------------------------------------------
// Block t = levels 64 t .. min(64 t + 63, q - 1).  256 threads; wave 0 of EVERY workgroup runs the chain (lane j = level 64 t + j):
//   dlo_j = acc_j;  for s = 0 .. n - 1:  lane s: d = dlo + dhi; t = d * iVarU; rhs = Yi - t; mean = inv * rhs; un = mean + tz;
//                                        lanes j > s: p = K[64 t + j][64 t + s] * un_s; dlo_j = dlo_j + p
// (the reference's step for level l, src/functions.jl:63-71, with dot(K[:, l], u) split as ngp_random.h splits it).  Workgroup 0
// writes u, du = u(new) - u(old) and dlo of the block.  Then wave w of workgroup b takes the rows r = 64 (t + 1) + 64 b + w, + 4, ...
// of its 64-row range: lane j forms p = K[r][64 t + j] * un_j, the butterfly adds the 64 products, acc_r = acc_r + (that sum).
// Nothing a workgroup reads is written by another one in the same launch (u, du, dlo of block t are written only, acc of block t is
// read only, acc of the rows below is owned row by row): no flag, no wait, no co-residency needed.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dense_block(const double *__restrict__ K, long long ld, long long q, int t, double *__restrict__ u,
                                                     const double *__restrict__ vu, double *__restrict__ scr,
                                                     const unsigned *__restrict__ abort_w) {
    __shared__ double skd[64 * 65];
    __shared__ double sun[64];
    if (abort_w && *abort_w != 0u) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long b0 = 64LL * t;
    const int n = (int)((q - b0) < 64 ? (q - b0) : 64);
    for (int e = tid; e < 64 * 64; e += 256) {
        const int r = e >> 6, c = e & 63;
        skd[r * 65 + c] = (r < n && c < n) ? K[(size_t)(b0 + r) * (size_t)ld + (size_t)(b0 + c)] : 0.0;
    }
    __syncthreads();
    if (wv == 0) {
        const bool valid = lane < n;
        const long long l = b0 + lane;
        const double iVarU = 1.0 / vu[0];
        double dlo = valid ? scr[NGP_RS_ACC * q + l] : 0.0;
        const double dhi = valid ? scr[NGP_RS_DHI * q + l] : 0.0, Yi = valid ? scr[NGP_RS_YI * q + l] : 0.0;
        const double inv = valid ? scr[NGP_RS_INV * q + l] : 0.0, tz = valid ? scr[NGP_RS_TZ * q + l] : 0.0;
        double mine = 0.0;
        for (int s = 0; s < n; s++) {
            const double d = dlo + dhi;
            const double tt = d * iVarU;
            const double rhs = Yi - tt;
            const double mean = inv * rhs;
            const double un = mean + tz;
            const double uns = __shfl(un, s);
            if (lane == s) mine = un;
            if (lane > s) {
                const double p = skd[lane * 65 + s] * uns;
                dlo = dlo + p;
            }
        }
        sun[lane] = mine;
        if (blockIdx.x == 0 && valid) {
            const double uo = u[l];
            scr[NGP_RS_DU * q + l] = mine - uo;
            scr[NGP_RS_DLO * q + l] = dlo;
            u[l] = mine;
        }
    }
    __syncthreads();
    const long long r0 = b0 + 64 + (long long)blockIdx.x * NGP_DENSE_WG_ROWS;
    const long long r1 = (r0 + NGP_DENSE_WG_ROWS) < q ? (r0 + NGP_DENSE_WG_ROWS) : q;
    const double un = sun[lane];
    for (long long r = r0 + wv; r < r1; r += 4) {  // (rows exist below the block: the block is a full one, 64 t + lane < q)
        double p = K[(size_t)r * (size_t)ld + (size_t)(b0 + lane)] * un;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) p = p + __shfl_xor(p, off);
        if (lane == 0) scr[NGP_RS_ACC * q + r] = scr[NGP_RS_ACC * q + r] + p;
    }
}

// ------------------------------------------------------------------------------------------
// varU of a dense set, ONE workgroup of 1024 threads.  Thread t takes the levels t, t + 1024, ...:
//   a = K_ll * u_l;  b = 2.0 * dlo_l;  s = a + b;  p = u_l * s;  acc = acc + p (from 0.0)
// (u'Ku = sum_l K_ll u_l^2 + 2 sum_l u_l sum_{c < l} K_lc u_c, all of this sweep), then exactly k_rand_var: the butterfly inside each
// wave, the 16 wave sums added in wave order, t = scale * df; t = t + quad; varU = t / chi2(df + q) keyed (NGP_KIND_U_CHI2, set).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_dense_var(long long q, const double *__restrict__ kdiag, const double *__restrict__ u,
                                                    const double *__restrict__ scr, double *__restrict__ vu, double df, double scale, int rset,
                                                    uint64_t seed, uint64_t chain, uint64_t it, const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    __shared__ double wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double acc = 0.0;
    for (long long l = tid; l < q; l += 1024) {
        const double a = kdiag[l] * u[l];
        const double b = 2.0 * scr[NGP_RS_DLO * q + l];
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
        Rng r = rng_seed(seed, chain, it, NGP_KIND_U_CHI2, (uint64_t)rset);
        const double chi = rng_chisq(r, df + (double)q);
        double t = scale * df;
        t = t + quad;
        vu[0] = t / chi;
    }
}

// ------------------------------------------------------------------------------------------
// Digest of a dense K for the model signature of snapshots (set-up, once per matrix): one wave per row; lane j folds the bit
// patterns of the columns j, j + 64, ... (ascending) into an FNV-1a word over 64-bit units, the 64 lane words are folded in lane
// order into the row's word.  Integer arithmetic in one fixed order: the same matrix gives the same words whatever its leading dimension.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dense_digest(const double *__restrict__ K, long long ld, long long q, unsigned long long *__restrict__ rowhash) {
    const int lane = threadIdx.x & 63;
    const long long l = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (l >= q) return;  // (uniform over the wave)
    const double *row = K + (size_t)l * (size_t)ld;
    unsigned long long x = 1469598103934665603ull;
    for (long long c = lane; c < q; c += 64) { x ^= (unsigned long long)__double_as_longlong(row[c]); x *= 1099511628211ull; }
    unsigned long long r = 1469598103934665603ull;
    for (int j = 0; j < 64; j++) { r ^= __shfl(x, j); r *= 1099511628211ull; }
    if (lane == 0) rowhash[l] = r;
}

// ==========================================================================================
// Genomic relationship matrix (VanRaden method 1 / 2).  All in fp64; the panel's fp32 tiles are not involved.
// ==========================================================================================

// One 64-thread workgroup per column of the staged chunk (nc real columns, padded with zero columns to cpad; rows padded with zeros
// to Npad): sum in fp64 (lane j adds rows j, j + 64, ... from 0.0, then the butterfly), mean = sum / N, p = mean / 2,
// tp = (2 p) (1 - p).  Method 1: xc = x - mean, tp goes to twopq[c].  Method 2: xc = (x - mean) / sqrt(tp); a column with tp <= 0 (or
// not a number) is reported through bad[1] (smallest such column of the chunk + 1).  bad[0]: a non-finite genotype was seen.
template <typename TIn>
__global__ __launch_bounds__(64) void k_grm_cols(const TIn *__restrict__ src, long long N, long long ld, long long nc, long long Npad, int method,
                                                 double *__restrict__ xc, double *__restrict__ twopq, unsigned *__restrict__ bad) {
    const long long c = blockIdx.x;
    const int lane = threadIdx.x;
    double *dst = xc + (size_t)c * (size_t)Npad;
    if (c >= nc) {
        for (long long i = lane; i < Npad; i += 64) dst[i] = 0.0;
        return;
    }
    const TIn *col = src + (size_t)c * (size_t)ld;
    double acc = 0.0;
    bool nf = false;
    for (long long i = lane; i < N; i += 64) {
        const double x = (double)col[i];
        nf = nf || !isfinite(x);
        acc = acc + x;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off);
    if (nf) atomicOr(&bad[0], 1u);
    const double mean = acc / (double)N;
    const double p = mean / 2.0;
    const double tp = (2.0 * p) * (1.0 - p);
    double sd = 1.0;
    if (method == 2) {
        if (!(tp > 0.0)) {
            if (lane == 0) atomicMin(&bad[1], (unsigned)c + 1u);
        } else sd = sqrt(tp);
    } else if (lane == 0) twopq[c] = tp;
    for (long long i = lane; i < Npad; i += 64) {
        double v = 0.0;
        if (i < N) {
            v = (double)col[i] - mean;
            if (method == 2) v = v / sd;
        }
        dst[i] = v;
    }
}

// G += Xc Xc' for the staged chunk, lower triangle of 64 x 64 tile blocks (blockIdx.x = row block >= blockIdx.y = column block), on
// the matrix cores: v_mfma_f64_16x16x4_f64.  256 threads = 4 waves; wave w owns the 32 x 32 quarter (w >> 1, w & 1) of the block as
// 2 x 2 accumulators of 16 x 16.  One MFMA contracts FOUR columns of the chunk: lane l supplies A[row (l & 15)][k = l >> 4] and
// B[k = l >> 4][col (l & 15)], both one f64 of the column-major chunk (16 consecutive rows of one column per quarter wave), and the
// core adds the four products to the accumulator one after the other, k ascending.  An accumulator starts from G as the calls before
// left it and walks the chunk's columns in ascending order, so every entry of G is ONE chain over all columns in their order,
// however they were split into calls and chunks (of multiples of four columns).  D layout: lane l, register v holds row
// (l >> 4) + 4 v, column l & 15 (cdna_hip_programming.md, f64 MFMA).  G is column-major with leading dimension Npad.
__global__ __launch_bounds__(256) void k_grm_syrk(const double *__restrict__ xc, long long Npad, long long cpad, double *__restrict__ G) {
    const int bi = blockIdx.x, bj = blockIdx.y;
    if (bj > bi) return;  // (block-uniform)
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const long long i0 = 64LL * bi + 32 * (w >> 1), j0 = 64LL * bj + 32 * (w & 1);
    const int rr = l >> 4, cc = l & 15;
    ngp_d4 a00, a01, a10, a11;
#pragma unroll
    for (int v = 0; v < 4; v++) {
        const long long r = rr + 4 * v;
        a00[v] = G[(size_t)(i0 + r) + (size_t)(j0 + cc) * (size_t)Npad];
        a01[v] = G[(size_t)(i0 + r) + (size_t)(j0 + 16 + cc) * (size_t)Npad];
        a10[v] = G[(size_t)(i0 + 16 + r) + (size_t)(j0 + cc) * (size_t)Npad];
        a11[v] = G[(size_t)(i0 + 16 + r) + (size_t)(j0 + 16 + cc) * (size_t)Npad];
    }
    const double *pa = xc + (size_t)rr * (size_t)Npad + (size_t)(i0 + cc);
    const double *pb = xc + (size_t)rr * (size_t)Npad + (size_t)(j0 + cc);
    const size_t step = 4 * (size_t)Npad;
    for (long long k = 0; k < cpad; k += 4) {
        const double x0 = pa[0], x1 = pa[16], y0 = pb[0], y1 = pb[16];
        a00 = __builtin_amdgcn_mfma_f64_16x16x4f64(x0, y0, a00, 0, 0, 0);
        a01 = __builtin_amdgcn_mfma_f64_16x16x4f64(x0, y1, a01, 0, 0, 0);
        a10 = __builtin_amdgcn_mfma_f64_16x16x4f64(x1, y0, a10, 0, 0, 0);
        a11 = __builtin_amdgcn_mfma_f64_16x16x4f64(x1, y1, a11, 0, 0, 0);
        pa += step; pb += step;
    }
#pragma unroll
    for (int v = 0; v < 4; v++) {
        const long long r = rr + 4 * v;
        G[(size_t)(i0 + r) + (size_t)(j0 + cc) * (size_t)Npad] = a00[v];
        G[(size_t)(i0 + r) + (size_t)(j0 + 16 + cc) * (size_t)Npad] = a01[v];
        G[(size_t)(i0 + 16 + r) + (size_t)(j0 + cc) * (size_t)Npad] = a10[v];
        G[(size_t)(i0 + 16 + r) + (size_t)(j0 + 16 + cc) * (size_t)Npad] = a11[v];
    }
}

// The computed triangle (i >= j, column-major: G[i + j ld]) into the other one, so that the matrix is exactly symmetric; with
// finish != 0 first G_ij = G_ij / denom and 0.001 added to the diagonal (src/misc.jl:150, 155, 158), one division and one sum.
__global__ __launch_bounds__(256) void k_grm_mirror(double *__restrict__ G, long long N, long long ld, int finish, double denom) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    for (long long j = blockIdx.y; j <= i; j += gridDim.y) {
        double v = G[(size_t)i + (size_t)j * (size_t)ld];
        if (finish) {
            v = v / denom;
            if (i == j) v = v + 0.001;
            G[(size_t)i + (size_t)j * (size_t)ld] = v;
        }
        if (i != j) G[(size_t)j + (size_t)i * (size_t)ld] = v;
    }
}

}  // namespace ngp
