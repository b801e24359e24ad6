// ngp_hybrid.h -- gfx950 kernels of single-step GBLUP: the Gauss-Seidel of a random-effect set whose K is a sparse q x q matrix S (CSR,
// a pedigree's A^-1) plus a dense nd x nd block on its LAST nd levels (G_w^-1 - A22^-1 over the genotyped animals), and the set-up of
// that block.  DESIGN.md section 2, "Hybrid random-effect sets (single-step GBLUP)", is the normative description of every summation
// order here; tests/ref_singlestep.py restates the step operation by operation.  No FMA anywhere in this file (fp contract off, no
// __builtin_fma): every product and sum is rounded on its own.
//
// hd = q - nd head levels, then nd trailing levels.  At set-up the entries of S with row and column both trailing are added into the
// dense block (T = D + S_tt, one sum per stored entry) and leave the CSR: a trailing row's CSR holds head columns only, kdiag of a
// trailing level is T_ll.  Per iteration, between k_rand_levels and k_rand_update (ngp_random.h), all on the chain's stream:
//   k_rand_levels       all q levels, unchanged: a head row's dhi runs over its stored columns c > l (trailing ones included, old u);
//                       a trailing row's CSR has no column > l, its dhi is replaced by
//   k_hyb_dhi           k_dense_dhi over T for the trailing rows (last sweep's u)
//   k_rand_sched_* / k_hyb_gs   the head rows 0 .. hd - 1 in level order: the level schedule of ngp_random.h as it is (its plan holds head
//                       rows only), or the serial walk -- rand_gs_row row by row in one thread
//   k_hyb_seed          per trailing row l: seed_l = sum over the stored entries of row l (all head columns), ascending, of S_lc u_c with
//                       this sweep's head values, from 0.0; the two block accumulators start from seed_l and from 0.0
//   k_hyb_block         k_dense_block over T on u + hd, one launch per block of 64 trailing levels: the chain starts from the seeded
//                       accumulator; the second accumulator takes the same products from 0.0 (the dense part of dlo, for u'Ku)
//   k_hyb_var           u'Ku = sum over head rows of u_l (S row l . u)  +  sum over trailing rows of u_l ((T_ll u_l + 2 dd_l) + seed_l):
//                       the cross block u_t' S_th u_h is counted once by the head rows' full stored rows and once by the seeds
// The scratch of a set is NGP_RS_ROWS_HYBRID x q doubles with stride q; the kernels of the trailing block take u + hd, scr + hd and
// the stride, and index rows and levels from 0 as the dense engine does.
#pragma once
#include "ngp_kernels.h"
#include "ngp_random.h"
#include "ngp_dense.h"

#pragma clang fp contract(off)

namespace ngp {

// scratch rows of a hybrid set beyond those of ngp_dense.h (NGP_RS_ACC: the seeded accumulator; NGP_RS_DLO: the dense part, complete)
#define NGP_RS_SEED 7   // seed_l = S_lh u_h of this sweep (trailing rows)
#define NGP_RS_ACC0 8   // the dense part of dlo accumulated over the blocks in front of a level's own, from 0.0
#define NGP_RS_ROWS_HYBRID 9

// ------------------------------------------------------------------------------------------
// The serial head engine: ONE thread walks the head rows 0 .. hd - 1 in order, each by rand_gs_row (ngp_random.h) -- the operations of
// k_rand_gs's loop body on the same values, u in global memory.  q is the stride of the scratch rows only.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_hyb_gs(long long hd, long long q, const long long *__restrict__ kptr, const int *__restrict__ kcol,
                                               const double *__restrict__ kval, double *u, const double *__restrict__ vu, double *scr,
                                               const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    if (threadIdx.x != 0) return;
    const double iVarU = 1.0 / vu[0];
    for (long long l = 0; l < hd; l++) rand_gs_row(l, q, kptr, kcol, kval, u, iVarU, scr);
}

// ------------------------------------------------------------------------------------------
// k_dense_dhi for the trailing block: T is nd x nd (row j at T + j ld), ut = u + hd, st = scr + hd, sq the stride of the scratch rows.
// Lane j of trailing row l's wave adds the columns c = 64 m + j, m ascending from l / 64, c > l, c < nd (from 0.0); the butterfly.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_hyb_dhi(const double *__restrict__ T, long long ld, long long nd, const double *__restrict__ ut,
                                                 double *__restrict__ st, long long sq, const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    const int lane = threadIdx.x & 63;
    const long long l = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (l >= nd) return;  // (uniform over the wave)
    const double *row = T + (size_t)l * (size_t)ld;
    double acc = 0.0;
    for (long long c = (l & ~63LL) + lane; c < nd; c += 64) {
        if (c > l) {
            const double t = row[c] * ut[c];
            acc = acc + t;
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off);
    if (lane == 0) st[NGP_RS_DHI * sq + l] = acc;
}

// ------------------------------------------------------------------------------------------
// The seed of every trailing row, one thread per row (a pedigree's row holds a handful of entries): after the fold every stored entry of
// a trailing row is a head column, so the whole row is walked, ascending, from 0.0, with the head values of THIS sweep.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_hyb_seed(long long hd, long long q, const long long *__restrict__ kptr, const int *__restrict__ kcol,
                                                  const double *__restrict__ kval, const double *__restrict__ u, double *__restrict__ scr,
                                                  const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    const long long l = hd + (long long)blockIdx.x * 256 + threadIdx.x;
    if (l >= q) return;
    double acc = 0.0;
    for (long long k = kptr[l]; k < kptr[l + 1]; k++) {
        const double t = kval[k] * u[kcol[k]];
        acc = acc + t;
    }
    scr[NGP_RS_SEED * q + l] = acc;
    scr[NGP_RS_ACC * q + l] = acc;
    scr[NGP_RS_ACC0 * q + l] = 0.0;
}

// ------------------------------------------------------------------------------------------
// k_dense_block for the trailing block (same launch shape, same chain): block t = trailing levels 64 t .. min(64 t + 63, nd - 1), wave 0
// of EVERY workgroup repeats the chain from read-only inputs, workgroup 0 writes u, du and the dense part dd of dlo; every workgroup
// then adds T[rows, block t] u_new[block t] to BOTH accumulators of its own rows below the block.  dlo_j starts from the seeded
// accumulator and decides the draw; dd_j starts from the unseeded one and takes the same products: it is what k_hyb_var doubles.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_hyb_block(const double *__restrict__ T, long long ld, long long nd, int t, double *__restrict__ ut,
                                                   const double *__restrict__ vu, double *__restrict__ st, long long sq,
                                                   const unsigned *__restrict__ abort_w) {
    __shared__ double skd[64 * 65];
    __shared__ double sun[64];
    if (abort_w && *abort_w != 0u) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const long long b0 = 64LL * t;
    const int n = (int)((nd - b0) < 64 ? (nd - b0) : 64);
    for (int e = tid; e < 64 * 64; e += 256) {
        const int r = e >> 6, c = e & 63;
        skd[r * 65 + c] = (r < n && c < n) ? T[(size_t)(b0 + r) * (size_t)ld + (size_t)(b0 + c)] : 0.0;
    }
    __syncthreads();
    if (wv == 0) {
        const bool valid = lane < n;
        const long long l = b0 + lane;
        const double iVarU = 1.0 / vu[0];
        double dlo = valid ? st[NGP_RS_ACC * sq + l] : 0.0;
        double dd = valid ? st[NGP_RS_ACC0 * sq + l] : 0.0;
        const double dhi = valid ? st[NGP_RS_DHI * sq + l] : 0.0, Yi = valid ? st[NGP_RS_YI * sq + l] : 0.0;
        const double inv = valid ? st[NGP_RS_INV * sq + l] : 0.0, tz = valid ? st[NGP_RS_TZ * sq + l] : 0.0;
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
                dd = dd + p;
            }
        }
        sun[lane] = mine;
        if (blockIdx.x == 0 && valid) {
            const double uo = ut[l];
            st[NGP_RS_DU * sq + l] = mine - uo;
            st[NGP_RS_DLO * sq + l] = dd;
            ut[l] = mine;
        }
    }
    __syncthreads();
    const long long r0 = b0 + 64 + (long long)blockIdx.x * NGP_DENSE_WG_ROWS;
    const long long r1 = (r0 + NGP_DENSE_WG_ROWS) < nd ? (r0 + NGP_DENSE_WG_ROWS) : nd;
    const double un = sun[lane];
    for (long long r = r0 + wv; r < r1; r += 4) {  // (rows exist below the block: the block is a full one, 64 t + lane < nd)
        double p = T[(size_t)r * (size_t)ld + (size_t)(b0 + lane)] * un;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) p = p + __shfl_xor(p, off);
        if (lane == 0) {
            st[NGP_RS_ACC * sq + r] = st[NGP_RS_ACC * sq + r] + p;
            st[NGP_RS_ACC0 * sq + r] = st[NGP_RS_ACC0 * sq + r] + p;
        }
    }
}

// ------------------------------------------------------------------------------------------
// varU of a hybrid set, ONE workgroup of 1024 threads.  Thread t takes the levels t, t + 1024, ... (acc from 0.0):
//   head l:      r = sum over the stored row l, ascending columns (trailing ones included), of S_lc * u_c (from 0.0);  p = u_l * r
//   trailing l:  a = T_ll * u_l;  b = 2.0 * dd_l;  s = a + b;  s = s + seed_l;  p = u_l * s
//   acc = acc + p
// then exactly k_rand_var: the butterfly inside each wave, the 16 wave sums added in wave order, t = sdf + quad (sdf = scale * df, the one
// product formed on the host); varU = t / chi2(df + q) keyed (NGP_KIND_U_CHI2, set).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_hyb_var(long long q, long long hd, const long long *__restrict__ kptr, const int *__restrict__ kcol,
                                                  const double *__restrict__ kval, const double *__restrict__ kdiag, const double *__restrict__ u,
                                                  const double *__restrict__ scr, double *__restrict__ vu, double df, double sdf, int rset,
                                                  uint64_t seed, uint64_t chain, uint64_t it, const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    __shared__ double wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double acc = 0.0;
    for (long long l = tid; l < q; l += 1024) {
        double p;
        if (l < hd) {
            double r = 0.0;
            for (long long k = kptr[l]; k < kptr[l + 1]; k++) {
                const double t = kval[k] * u[kcol[k]];
                r = r + t;
            }
            p = u[l] * r;
        } else {
            const double a = kdiag[l] * u[l];
            const double b = 2.0 * scr[NGP_RS_DLO * q + l];
            double s = a + b;
            s = s + scr[NGP_RS_SEED * q + l];
            p = u[l] * s;
        }
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
        const double t = sdf + quad;
        vu[0] = t / chi;
    }
}

// ------------------------------------------------------------------------------------------
// Set-up.  k_hyb_fold: T[r][c] = T[r][c] + v for every stored entry of S_tt (one thread per entry; an entry occurs once, (r, c) and
// (c, r) are both stored and take the same sum: T stays exactly symmetric).  k_ss_blend: G = (1 - w) G + w A22 entry by entry over the
// N x N matrix (t1 = omw * G; t2 = w * A; G = t1 + t2: both inputs symmetric, so is the result).  k_ss_diff: the computed (lower,
// column-major i >= j) triangle of G_w^-1 minus that of A22^-1; k_grm_mirror (ngp_dense.h) then copies it across.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_hyb_fold(double *__restrict__ T, long long ld, long long n, const int *__restrict__ fr,
                                                  const int *__restrict__ fc, const double *__restrict__ fv) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    const size_t at = (size_t)fr[e] * (size_t)ld + (size_t)fc[e];
    T[at] = T[at] + fv[e];
}

__global__ __launch_bounds__(256) void k_ss_blend(double *__restrict__ G, const double *__restrict__ A, long long N, long long ld, double omw,
                                                  double w) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    for (long long j = blockIdx.y; j < N; j += gridDim.y) {
        const size_t at = (size_t)i + (size_t)j * (size_t)ld;
        const double t1 = omw * G[at];
        const double t2 = w * A[at];
        G[at] = t1 + t2;
    }
}

__global__ __launch_bounds__(256) void k_ss_diff(double *__restrict__ G, const double *__restrict__ A, long long N, long long ld) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    for (long long j = blockIdx.y; j <= i; j += gridDim.y) {
        const size_t at = (size_t)i + (size_t)j * (size_t)ld;
        G[at] = G[at] - A[at];
    }
}

}  // namespace ngp
