// ngp_gpred.h -- GBLUP prediction of new individuals: the candidates x records relationship block C of a dense set whose K = inv(G) was
// built by ngp_grm_*, and what turns it into a mean and an honest SD per candidate ("GBLUP prediction": the
// normative orders).  Kernels of a translation unit of their own (ngp_gpred_inst.hip), beside the back-solve's: the API unit and the
// sweep units carry no code they did not carry before.  Everything is fp64.
//   k_gp_colstats  mu_j (and sqrt(2 p_j q_j) under method 2) of every staged column FROM THE RECORDS' genotypes, by the GRM builder's
//                  own statistics (ngp_grm_stats.h); the candidates' columns are only searched for non-finite values
//   k_gp_cross     C += Xc_cand Xc_train' on the matrix cores (v_mfma_f64_16x16x4_f64) and gcc_c += xc^2 in the same pass
//   k_gp_scale     C / denominator, gcc / denominator: the one division of ngp_grm_end
//   k_gp_resid     s_c = gcc_c - sum_i C_ci V_ic with V = K C' (k_bs_kw, the candidates in the place of the draws)
//   k_gp_fill      a constant into an array (mu = 0 and d = 1 of the projection, which is k_bs_cols over the rows of C)
// C is kept as C' : N x Nc column-major with leading dimension N, Ct[i + c N] -- the layout k_bs_kw takes its draws in and k_bs_cols
// its genotype columns, so both serve the candidates without a copy or a transpose.
//
// k_gp_cross.  A workgroup (256 threads) owns 64 candidates x 64 records of C; wave w owns the candidates 16 w .. 16 w + 15 as four
// 16 x 16 accumulators, one per group g of 16 records.  The candidates are the A operand, the records the B operand, in k_grm_syrk's
// conventions: lane l = (cc = l & 15, rr = l >> 4) supplies A[candidate cc][k = rr] and B[k = rr][record cc]; D: lane l, register v
// holds candidate rr + 4 v, record cc.  Both operand tiles go through LDS, 32 columns at a time: an element of the candidates' tile
// feeds four accumulators, an element of the records' tile four waves.  The raw values of the NEXT 32 columns are requested into
// registers (in the input's own type) before the matrix steps of the current ones, and centred as they are written to LDS:
//     x = (double)z - mu_j;  method 2: x = x / sqrt(tp_j)       -- k_grm_cols' two operations, with the records' mu_j and tp_j
// One LDS buffer with that register prefetch was kept, not two buffers: the wait that a second buffer would hide is the global load,
// which the registers hide already, and the registers (176 VGPR + 32 AGPR: two waves per SIMD), not the 40 KiB of LDS, set the occupancy.
// LDS layout: s[k * 80 + row], a column's 64 rows adjacent and 16 doubles of padding.  The half wave rr = 0, 1 (and 2, 3) reads the
// doubles cc and 80 + cc: dwords 2 cc and 32 + 2 cc (mod 64), every bank once; the loaders write 64 adjacent doubles per wave.
// Rows >= Nc / >= N and columns beyond the chunk are zeros by predicated loads (not mu-centred zeros): nothing outside the two staged
// arrays is read.
// The order: every C_ci is ONE chain over all columns in their order, four at a time ascending, the core adding its four products one
// after the other, and the accumulator starts from C as the columns before left it -- k_grm_syrk's chain, with the same operand
// values.  A chunk is padded to four with zero columns, every call but the last brings a multiple of 64, so the split into calls and
// chunks does not show in the bits, and a candidate with the genotypes of record r gets row r of G off the diagonal (before the ridge
// on it).  gcc_c: the workgroups of the first record tile, wave 0, lane = candidate: gcc = gcc + x * x over the columns in their
// order, from gcc as the columns before left it (one chain per candidate, product and sum rounded separately).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#ifdef NGP_GPRED_KERNELS
#include "ngp_grm_stats.h"
#endif

namespace ngp {

// the launches (ngp_gpred_inst.hip); type: 0 f64, 1 f32, 2 u8 genotypes
struct GpCols {
    int type, method;            // genotype type; GRM method 1 / 2
    const void *train, *cand;    // the staged chunk: nc raw columns of N records (leading dimension ldt) and of Nc candidates (ldc)
    long long N, ldt, Nc, ldc, nc;
    double *mu, *sd;             // nc scratch entries
    unsigned *bad;               // [0] a non-finite genotype, [1] smallest monomorphic column + 1 under method 2 (as k_grm_cols)
    double *Ct, *gcc;            // N x (Nc rounded up to 64), leading dimension N; Nc rounded up to 64
};
hipError_t gpred_colstats(const GpCols &c, hipStream_t stream);  // mu, sd and the flags; the caller reads the flags before gpred_cross
hipError_t gpred_cross(const GpCols &c, hipStream_t stream);
hipError_t gpred_scale(double *Ct, long long N, long long Nc, double *gcc, double denom, hipStream_t stream);
hipError_t gpred_resid(const double *Ct, const double *V, long long N, long long Nc, const double *gcc, double *s, hipStream_t stream);
hipError_t gpred_fill(double *p, long long n, double v, hipStream_t stream);

#ifdef NGP_GPRED_KERNELS

#pragma clang fp contract(off)

typedef double gp_d4 __attribute__((ext_vector_type(4)));
#define NGP_GP_KT 32  // columns per LDS tile
#define NGP_GP_LS 80  // LDS stride (doubles) of one column's 64 rows

// blocks 0 .. nc - 1: one wave per column of the records; blocks nc .. 2 nc - 1: the candidates' column, searched for non-finite values
template <typename TIn>
__global__ __launch_bounds__(64) void k_gp_colstats(const TIn *__restrict__ train, long long N, long long ldt, const TIn *__restrict__ cand, long long Nc,
                                                    long long ldc, long long nc, int method, double *__restrict__ mu, double *__restrict__ sd,
                                                    unsigned *__restrict__ bad) {
    const int lane = threadIdx.x;
    long long c = blockIdx.x;
    if (c >= nc) {
        c -= nc;
        const TIn *col = cand + (size_t)c * (size_t)ldc;
        bool nf = false;
        for (long long i = lane; i < Nc; i += 64) nf = nf || !isfinite((double)col[i]);
        if (nf) atomicOr(&bad[0], 1u);
        return;
    }
    double mean, tp;
    bool nf;
    grm_col_stats<TIn>(train + (size_t)c * (size_t)ldt, N, lane, mean, tp, nf);
    if (nf) atomicOr(&bad[0], 1u);
    if (lane != 0) return;
    double s = 1.0;
    if (method == 2) {
        if (!(tp > 0.0)) atomicMin(&bad[1], (unsigned)c + 1u);
        else s = sqrt(tp);
    }
    mu[c] = mean;
    sd[c] = s;
}

template <typename TIn>
__device__ __forceinline__ double gp_centre(TIn z, bool on, double m, double s, int method) {
    double x = (double)z - m;
    if (method == 2) x = x / s;
    return on ? x : 0.0;
}

// grid (ceil(Nc / 64), ceil(N / 64)), 256 threads.  Ct holds 64 ceil(Nc / 64) columns of N rows: the candidates beyond Nc are zeros.
template <typename TIn>
__global__ __launch_bounds__(256) void k_gp_cross(const TIn *__restrict__ train, long long N, long long ldt, const TIn *__restrict__ cand, long long Nc,
                                                  long long ldc, long long nc, int method, const double *__restrict__ mu, const double *__restrict__ sd,
                                                  double *__restrict__ Ct, double *__restrict__ gcc) {
    __shared__ double sA[NGP_GP_KT * NGP_GP_LS];  // the candidates' tile, [column][candidate]
    __shared__ double sB[NGP_GP_KT * NGP_GP_LS];  // the records' tile, [column][record]
    const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, rr = l >> 4, cc = l & 15;
    const long long c0 = 64LL * blockIdx.x, i0 = 64LL * blockIdx.y;
    const long long cpad = (nc + 3) / 4 * 4;
    const bool wave_gcc = blockIdx.y == 0 && w == 0;  // (wave-uniform)
    gp_d4 acc[4];
#pragma unroll
    for (int g = 0; g < 4; g++)
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const long long i = i0 + 16 * g + cc, c = c0 + 16 * w + rr + 4 * v;
            acc[g][v] = (i < N) ? Ct[(size_t)i + (size_t)c * (size_t)N] : 0.0;
        }
    double gc = wave_gcc ? gcc[c0 + l] : 0.0;
    // the loader: thread (row = l, wave w) takes the columns w, w + 4, ... of the tile, of both operands
    const bool onA = c0 + l < Nc, onB = i0 + l < N;
    const TIn *pa = cand + (size_t)(onA ? c0 + l : 0), *pb = train + (size_t)(onB ? i0 + l : 0);
    TIn za[8], zb[8];
    double zm[8], zs[8];
#define NGP_GP_REQUEST(J0)                                                             \
    _Pragma("unroll") for (int e = 0; e < 8; e++) {                                    \
        const long long j = (J0) + w + 4 * e;                                          \
        const bool on = j < nc;                                                        \
        zm[e] = on ? mu[j] : 0.0;                                                      \
        zs[e] = on ? sd[j] : 1.0;                                                      \
        za[e] = (on && onA) ? pa[(size_t)j * (size_t)ldc] : (TIn)0;                    \
        zb[e] = (on && onB) ? pb[(size_t)j * (size_t)ldt] : (TIn)0;                    \
    }
    NGP_GP_REQUEST(0)
    for (long long j0 = 0; j0 < cpad; j0 += NGP_GP_KT) {
        __syncthreads();  // (the tile of the step before has been read)
#pragma unroll
        for (int e = 0; e < 8; e++) {
            const bool on = j0 + w + 4 * e < nc;
            sA[(w + 4 * e) * NGP_GP_LS + l] = gp_centre<TIn>(za[e], on && onA, zm[e], zs[e], method);
            sB[(w + 4 * e) * NGP_GP_LS + l] = gp_centre<TIn>(zb[e], on && onB, zm[e], zs[e], method);
        }
        __syncthreads();
        if (j0 + NGP_GP_KT < cpad) { NGP_GP_REQUEST(j0 + NGP_GP_KT) }  // in flight behind the matrix steps
        const int nk = (int)((cpad - j0 < NGP_GP_KT ? cpad - j0 : NGP_GP_KT) / 4);
        for (int kb = 0; kb < nk; kb++) {
            const double a = sA[(4 * kb + rr) * NGP_GP_LS + 16 * w + cc];
#pragma unroll
            for (int g = 0; g < 4; g++)
                acc[g] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sB[(4 * kb + rr) * NGP_GP_LS + 16 * g + cc], acc[g], 0, 0, 0);
        }
        if (wave_gcc)
            for (int k = 0; k < 4 * nk; k++) {
                const double x = sA[k * NGP_GP_LS + l];
                const double x2 = x * x;
                gc = gc + x2;
            }
    }
#undef NGP_GP_REQUEST
#pragma unroll
    for (int g = 0; g < 4; g++)
#pragma unroll
        for (int v = 0; v < 4; v++) {
            const long long i = i0 + 16 * g + cc, c = c0 + 16 * w + rr + 4 * v;
            if (i < N) Ct[(size_t)i + (size_t)c * (size_t)N] = acc[g][v];
        }
    if (wave_gcc) gcc[c0 + l] = gc;
}

// grid (ceil(N / 256), min(Nc, 65535)); block (0, 0) scales gcc as well
__global__ __launch_bounds__(256) void k_gp_scale(double *__restrict__ Ct, long long N, long long Nc, double *__restrict__ gcc, double denom) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < N)
        for (long long c = blockIdx.y; c < Nc; c += gridDim.y) Ct[(size_t)i + (size_t)c * (size_t)N] = Ct[(size_t)i + (size_t)c * (size_t)N] / denom;
    if (blockIdx.y == 0)
        for (long long c = i; c < Nc; c += (long long)gridDim.x * 256) gcc[c] = gcc[c] / denom;
}

// one wave per candidate: lane j adds C_ci V_ic over the records j, j + 64, ... ascending from 0.0, then the xor butterfly 32 .. 1
__global__ __launch_bounds__(64) void k_gp_resid(const double *__restrict__ Ct, const double *__restrict__ V, long long N, const double *__restrict__ gcc,
                                                 double *__restrict__ s) {
    const int lane = threadIdx.x;
    const double *a = Ct + (size_t)blockIdx.x * (size_t)N, *b = V + (size_t)blockIdx.x * (size_t)N;
    double acc = 0.0;
    for (long long i = lane; i < N; i += 64) {
        const double p = a[i] * b[i];
        acc = acc + p;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off);
    if (lane == 0) s[blockIdx.x] = gcc[blockIdx.x] - acc;
}

__global__ __launch_bounds__(256) void k_gp_fill(double *__restrict__ p, long long n, double v) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) p[i] = v;
}

#endif  // NGP_GPRED_KERNELS

}  // namespace ngp
