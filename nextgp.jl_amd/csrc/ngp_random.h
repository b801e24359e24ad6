// ngp_random.h -- gfx950 kernels of one (1|g) random-effect set per iteration: sampleZ! / sampleU / sampleVarU of the reference
// (src/functions.jl:57-72, 92-97, 498-501; set-up src/mme.jl:165-272).  DESIGN.md "Random-effect sets" is the normative description
// of every summation order and draw key used here; tests/ref_random.py restates it operation by operation.  No FMA anywhere in
// this file (fp contract off, no __builtin_fma): every product and sum is rounded on its own.
//
// Per set and iteration, on the chain's stream, behind the fixed-effect sets and in front of the marker sweep:
//   k_rand_levels   one 64-lane wave per level: Yi_l = (sum_{i in l} ycorr_i + zpz_l u_l) iVarE (ycorr untouched), lhs, 1/lhs, sd, the
//                   keyed normal; a K without off-diagonal entries draws u_l right there, a general K leaves the terms to k_rand_gs
//   k_rand_gs       general K: Gauss-Seidel in level order in ONE wave (only the sparse dot over the levels below l and the draw)
//   k_rand_sched_*  the same Gauss-Seidel level-scheduled: the rows of equal depth side by side (a pedigree's A^-1: 10^5 rows, 10^2 depths)
//   k_rand_update   ycorr_i -= du_{level(i)}  (s_i du under weighted residuals)
//   k_rand_var      u'Ku in a fixed order, then varU = (scale df + u'Ku) / chi2(df + q)
#pragma once
#include "ngp_common.h"

#pragma clang fp contract(off)

namespace ngp {

// scratch rows of a set (NGP_RS_* x q doubles): what k_rand_levels leaves for k_rand_gs, and du for k_rand_update
#define NGP_RS_YI 0
#define NGP_RS_INV 1
#define NGP_RS_TZ 2
#define NGP_RS_DHI 3
#define NGP_RS_DU 4
#define NGP_RS_ROWS 5

// ------------------------------------------------------------------------------------------
// level sums and the per-level terms.  256 threads = 4 waves = 4 levels per workgroup, ceil(q / 4) workgroups.
// Lane j of level l's wave adds the records lrows[lptr[l] + j], lrows[lptr[l] + j + 64], ... (the level's records in ascending
// record order: a stable sort of the records by level, built at set-up) into acc, from 0.0; the 64 lane sums are then combined by
// the butterfly acc = acc + shfl_xor(acc, off), off = 32, 16, 8, 4, 2, 1.  Weighted residuals: the term is (s_i * y~_i).
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rand_levels(const double *__restrict__ ycorr, const double *__restrict__ rs, long long q,
                                                     const long long *__restrict__ lptr, const int *__restrict__ lrows,
                                                     const double *__restrict__ zpz, const double *__restrict__ kdiag,
                                                     const long long *__restrict__ kptr, const int *__restrict__ kcol,
                                                     const double *__restrict__ kval, double *__restrict__ u, const double *__restrict__ vu,
                                                     double *__restrict__ scr, int offdiag, const DScal *__restrict__ sc, int rset,
                                                     uint64_t seed, uint64_t chain, uint64_t it, const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;  // an earlier sweep of this call gave up (ngp_sweep_args.h, abort_w)
    const int lane = threadIdx.x & 63;
    const long long l = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (l >= q) return;  // (uniform over the wave)
    const long long r0 = lptr[l], r1 = lptr[l + 1];
    double acc = 0.0;
    if (rs) {
        for (long long k = r0 + lane; k < r1; k += 64) {
            const int i = lrows[k];
            const double t = rs[i] * ycorr[i];
            acc = acc + t;
        }
    } else {
        for (long long k = r0 + lane; k < r1; k += 64) acc = acc + ycorr[lrows[k]];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off);
    if (lane != 0) return;
    const double iVarE = sc->iVarE, iVarU = 1.0 / vu[0];
    const double uo = u[l];
    const double tu = zpz[l] * uo;
    const double tot = acc + tu;
    const double Yi = tot * iVarE;
    const double t1 = zpz[l] * iVarE;
    const double t2 = kdiag[l] * iVarU;
    const double lhs = t1 + t2;
    const double inv = 1.0 / lhs;
    const double sd = det_sqrt(inv);
    Rng r = rng_seed(seed, chain, it, NGP_KIND_U_NORMAL, ((uint64_t)rset << 40) | (uint64_t)l);
    const double z = rng_normal(r);
    const double tz = sd * z;
    if (!offdiag) {  // K diagonal: rhs = Yi (the dot over the other levels is empty), every level on its own
        const double mean = inv * Yi;
        const double un = mean + tz;
        scr[NGP_RS_DU * q + l] = un - uo;
        u[l] = un;
        return;
    }
    // general K: the part of dot(K[:, l], u) over the levels ABOVE l uses the values of the previous iteration, known now
    // (kptr null: a dense K, whose dhi is k_dense_dhi's -- ngp_dense.h)
    double dhi = 0.0;
    if (kptr) for (long long k = kptr[l]; k < kptr[l + 1]; k++) {
        const int c = kcol[k];
        if (c > l) {
            const double t = kval[k] * u[c];
            dhi = dhi + t;
        }
    }
    scr[NGP_RS_YI * q + l] = Yi;
    scr[NGP_RS_INV * q + l] = inv;
    scr[NGP_RS_TZ * q + l] = tz;
    scr[NGP_RS_DHI * q + l] = dhi;
}

// ------------------------------------------------------------------------------------------
// Gauss-Seidel over a general K (src/functions.jl:63-71), ONE workgroup of one wave; lane 0 walks the levels in order:
//   dlo = sum over the entries of row l with column < l, ascending, of K_lc * u_c (values of this sweep), from 0.0
//   d = dlo + dhi_l;  t = d * iVarU;  rhs = Yi_l - t;  mean = inv_l * rhs;  u_l = mean + tz_l;  du_l = u_l(new) - u_l(old)
// u is held in LDS when 8q bytes fit (use_lds; the lanes copy it in and out), read and written in global memory otherwise.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_rand_gs(long long q, const long long *__restrict__ kptr, const int *__restrict__ kcol,
                                                const double *__restrict__ kval, double *__restrict__ u, const double *__restrict__ vu,
                                                double *__restrict__ scr, int use_lds, const unsigned *__restrict__ abort_w) {
    extern __shared__ double su[];
    if (abort_w && *abort_w != 0u) return;
    const int tid = threadIdx.x;
    double *uu = use_lds ? su : u;
    if (use_lds) {
        for (long long l = tid; l < q; l += 64) su[l] = u[l];
        __syncthreads();
    }
    if (tid == 0) {
        const double iVarU = 1.0 / vu[0];
        const double *Yi = scr + NGP_RS_YI * q, *inv = scr + NGP_RS_INV * q, *tz = scr + NGP_RS_TZ * q, *dhi = scr + NGP_RS_DHI * q;
        double *du = scr + NGP_RS_DU * q;
        for (long long l = 0; l < q; l++) {
            double dlo = 0.0;
            for (long long k = kptr[l]; k < kptr[l + 1]; k++) {
                const int c = kcol[k];
                if (c < l) {
                    const double t = kval[k] * uu[c];
                    dlo = dlo + t;
                }
            }
            const double d = dlo + dhi[l];
            const double t = d * iVarU;
            const double rhs = Yi[l] - t;
            const double mean = inv[l] * rhs;
            const double un = mean + tz[l];
            du[l] = un - uu[l];
            uu[l] = un;
        }
    }
    if (use_lds) {
        __syncthreads();
        for (long long l = tid; l < q; l += 64) u[l] = su[l];
    }
}

// ------------------------------------------------------------------------------------------
// The same Gauss-Seidel, level-scheduled (DESIGN.md "Random-effect sets", the schedule).  depth(l) = 0 for a row without an entry
// left of its diagonal, else 1 + max depth(c) over its columns c < l: every u_c (c < l) that row l reads belongs to a smaller
// depth, and no row reads the u of another row of its own depth.  So the rows of one depth run side by side, one thread per row,
// each doing the operations of k_rand_gs's loop body in the same order on the same values: the result is the same bits.
//   order[dptr[d] .. dptr[d + 1])   the rows of depth d, ascending
//   k_rand_sched_wide    one depth of more than NGP_RS_FUSE_ROWS rows: ceil(rows / 256) workgroups, the rows order[r0 .. r1)
//   k_rand_sched_fused   a run of consecutive narrower depths d0 .. d1 - 1 in ONE workgroup of 1024 threads, a workgroup-scope
//                        fence and __syncthreads() between two depths
// The stream orders the launches; no launch waits for another workgroup.  u is read and written in global memory by many
// threads in turn, hence neither const nor __restrict__ here.
// ------------------------------------------------------------------------------------------
#define NGP_RS_FUSE_ROWS 1024
// the automatic choice of the engine (ngp_set_random_schedule, mode 0): scheduled when the set has more than this many levels per
// depth, serial otherwise.  Measured (tools/random_gs_time.py): the serial walk costs 0.85 us per level with u in
// LDS (1.1 us from global memory), a depth of the fused launch 1.4 - 2.2 us while it is a few rows wide; at 1.9 levels per depth the
// two engines are 10 % apart, at 3.4 the scheduled one is 1.4 times faster
#define NGP_RS_AUTO_LEVELS_PER_DEPTH 2

__device__ __forceinline__ void rand_gs_row(long long l, long long q, const long long *__restrict__ kptr, const int *__restrict__ kcol,
                                            const double *__restrict__ kval, double *u, double iVarU, double *scr) {
    double dlo = 0.0;
    for (long long k = kptr[l]; k < kptr[l + 1]; k++) {
        const int c = kcol[k];
        if (c < l) {
            const double t = kval[k] * u[c];
            dlo = dlo + t;
        }
    }
    const double d = dlo + scr[NGP_RS_DHI * q + l];
    const double t = d * iVarU;
    const double rhs = scr[NGP_RS_YI * q + l] - t;
    const double mean = scr[NGP_RS_INV * q + l] * rhs;
    const double un = mean + scr[NGP_RS_TZ * q + l];
    scr[NGP_RS_DU * q + l] = un - u[l];
    u[l] = un;
}

__global__ __launch_bounds__(256) void k_rand_sched_wide(long long q, const long long *__restrict__ kptr, const int *__restrict__ kcol,
                                                         const double *__restrict__ kval, double *u, const double *__restrict__ vu, double *scr,
                                                         const int *__restrict__ order, long long r0, long long r1,
                                                         const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    const long long i = r0 + (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= r1) return;
    rand_gs_row((long long)order[i], q, kptr, kcol, kval, u, 1.0 / vu[0], scr);
}

__global__ __launch_bounds__(1024) void k_rand_sched_fused(long long q, const long long *__restrict__ kptr, const int *__restrict__ kcol,
                                                           const double *__restrict__ kval, double *u, const double *__restrict__ vu, double *scr,
                                                           const int *__restrict__ order, const long long *__restrict__ dptr, int d0, int d1,
                                                           const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;  // (uniform over the workgroup)
    const double iVarU = 1.0 / vu[0];
    for (int d = d0; d < d1; d++) {  // (uniform: every thread meets every barrier)
        const long long r1 = dptr[d + 1];
        for (long long i = dptr[d] + threadIdx.x; i < r1; i += 1024) rand_gs_row((long long)order[i], q, kptr, kcol, kval, u, iVarU, scr);
        __threadfence_block();
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------
// ycorr_i -= du_{level(i)} (src/functions.jl:93 and :95 in one step); weighted residuals: y~_i -= s_i du
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_rand_update(double *__restrict__ ycorr, const double *__restrict__ rs, long long N,
                                                     const int *__restrict__ level, const double *__restrict__ du,
                                                     const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    const int lv = level[i];
    if (lv < 0) return;  // (a record without a level: ngp_add_random_set_tuple with k = 1)
    double t = du[lv];
    if (rs) t = rs[i] * t;
    ycorr[i] = ycorr[i] - t;
}

// ------------------------------------------------------------------------------------------
// varU (src/functions.jl:498-501), ONE workgroup of 1024 threads.  Thread t takes the levels t, t + 1024, ...:
//   r_l = sum over row l of K, ascending columns, of K_lc * u_c (from 0.0);  p = u_l * r_l;  acc = acc + p (from 0.0)
// then the butterfly of k_rand_levels inside each wave, the 16 wave sums added in wave order by thread 0 (quad = w_0 + w_1 + ...),
//   t = scale * df (sdf: the one product, formed on the host);  t = t + quad;  varU = t / chi2(df + q) keyed (NGP_KIND_U_CHI2, set)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_rand_var(long long q, const long long *__restrict__ kptr, const int *__restrict__ kcol,
                                                   const double *__restrict__ kval, const double *__restrict__ u, double *__restrict__ vu,
                                                   double df, double sdf, int rset, uint64_t seed, uint64_t chain, uint64_t it,
                                                   const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    __shared__ double wsum[16];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double acc = 0.0;
    for (long long l = tid; l < q; l += 1024) {
        double r = 0.0;
        for (long long k = kptr[l]; k < kptr[l + 1]; k++) {
            const double t = kval[k] * u[kcol[k]];
            r = r + t;
        }
        const double p = u[l] * r;
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

}  // namespace ngp
