// ngp_random_tuple.h -- gfx950 kernels of one correlated (Tuple) random-effect set per iteration: sampleZ!(::Tuple) / sampleU(::Tuple) /
// sampleVarU of the reference (src/functions.jl:75-89, 100-110, 503-506; set-up src/mme.jl:207-239), k = 2 .. NGP_KMAX components over
// one K -- the (ID, Dam) direct-maternal model.  k = 1 runs the kernels of ngp_random.h.  DESIGN.md "Correlated random-effect sets" is the
// normative description of every summation order and draw key used here; tests/ref_random_tuple.py restates it operation by
// operation.  As in ngp_random.h there is no FMA in this file's own arithmetic (fp contract off): every product and sum is rounded
// on its own.  The k x k helpers t_chol / t_spd_inv (ngp_common.h) and the Bartlett factor keep the fused operations they are
// written with in the Tuple marker path.
//
// THE CONDITIONAL.  The reference forms Yi = Zp[i] ycorr on a ycorr that holds every component's Z u and subtracts only the
// K (x) inv(varU) couplings; that leaves Z_a'Z_b u_b of the OTHER levels in the right-hand side (a record of animal a with dam d).
// The device draws the exact Gibbs conditional: K_lc (x) inv(varU) + W_lc / varE for c != l, with the k x k blocks
//   W_lc[a][b] = sum over the records i with level_a(i) = l and level_b(i) = c of 1 (of w_i under weighted residuals)
// u is q x k with the k components of a level adjacent; varU and Sigma_i = inv(varU) are k x k row-major.
//
// Per set and iteration, on the chain's stream, behind the fixed-effect sets and in front of the marker sweep:
//   k_tup_prep        Sigma_i = inv(varU), once per step
//   k_tup_levels      one 64-lane wave per (level, component): S_l[m]; then per level Yi, inv(LHS), L z, dhi
//   k_tup_gs          Gauss-Seidel in level order in ONE wave
//   k_tup_sched_*     the same Gauss-Seidel level-scheduled over the union of the patterns of K and of the off-diagonal W blocks
//   k_tup_update      ycorr_i -= sum_m du_m[level_m(i)]
//   k_tup_var         S = U K U' in a fixed order, Psi = scale + S, varU ~ InverseWishart(df + q, Psi)
#pragma once
#include "ngp_random.h"

#pragma clang fp contract(off)

namespace ngp {

// scratch of a tuple set, doubles: Yi (q k) | inv(LHS) (q k k) | L z (q k) | dhi (q k) | du (q k) | Sigma_i (k k)
struct TupScr {
    double *Yi, *inv, *tz, *dhi, *du, *sig;
};
__host__ __device__ inline size_t tup_scr_len(long long q, int k) { return (size_t)q * (size_t)k * (size_t)(4 + k) + (size_t)(k * k); }
__host__ __device__ inline TupScr tup_scr(double *scr, long long q, int k) {
    const size_t qk = (size_t)q * (size_t)k;
    return {scr, scr + qk, scr + qk + qk * (size_t)k, scr + 2 * qk + qk * (size_t)k, scr + 3 * qk + qk * (size_t)k, scr + 4 * qk + qk * (size_t)k};
}

// Sigma_i = inv(varU) by t_spd_inv; a varU that is not positive definite poisons the chain visibly (NaN), as the Tuple marker path does
__global__ __launch_bounds__(64) void k_tup_prep(int k, const double *__restrict__ vu, double *__restrict__ sig, const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    if (threadIdx.x != 0) return;
    double V[NGP_KMAX * NGP_KMAX], Si[NGP_KMAX * NGP_KMAX];
    for (int a = 0; a < k * k; a++) V[a] = vu[a];
    const int bad = t_spd_inv(V, k, Si);
    for (int a = 0; a < k * k; a++) sig[a] = bad ? __builtin_nan("") : Si[a];
}

// ------------------------------------------------------------------------------------------
// level sums and the per-level terms.  256 threads = 4 waves; a workgroup takes floor(4 / k) levels, wave (j k + m) the component m of
// its level j (k = 3: one wave idles).  lptr / lrows: component m's records by level, lptr[m (q + 1) + l] .. lptr[m (q + 1) + l + 1]
// into lrows, ascending record order, records with level -1 in that component left out.  Lane striding and butterfly of k_rand_levels.
// Then one thread per level, every sum from 0.0 with ascending index:
//   tot_a = S_a + sum_b (Wd_ab * u_b);  Yi_a = tot_a * iVarE                       (Wd = W_ll, k x k, set-up)
//   LHS_ab = (Wd_ab * iVarE) + (K_ll * Sigma_i_ab);  inv = t_spd_inv(LHS);  L = t_chol(inv);  tz_a = sum_{b <= a} (L_ab * z_b)
//   z_b keyed (NGP_KIND_U_NORMAL, (set << 40) | (l k + b));  dhi_a = sum over the entries of row l of K with column c > l of (K_lc * u_c,a)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tup_levels(const double *__restrict__ ycorr, const double *__restrict__ rs, long long q, int k,
                                                    const long long *__restrict__ lptr, const int *__restrict__ lrows,
                                                    const double *__restrict__ wd, const double *__restrict__ kdiag,
                                                    const long long *__restrict__ kptr, const int *__restrict__ kcol,
                                                    const double *__restrict__ kval, const double *__restrict__ u, double *__restrict__ scr,
                                                    const DScal *__restrict__ sc, int rset, uint64_t seed, uint64_t chain, uint64_t it,
                                                    const unsigned *__restrict__ abort_w) {
    __shared__ double ssum[4];
    if (abort_w && *abort_w != 0u) return;  // (uniform over the workgroup)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int lpb = 4 / k, j = wv / k, m = wv - j * k;
    const long long l = (long long)blockIdx.x * lpb + j;
    const bool live = j < lpb && l < q;  // (uniform over the wave)
    if (live) {
        const long long r0 = lptr[(long long)m * (q + 1) + l], r1 = lptr[(long long)m * (q + 1) + l + 1];
        double acc = 0.0;
        if (rs) {
            for (long long p = r0 + lane; p < r1; p += 64) {
                const int i = lrows[p];
                const double t = rs[i] * ycorr[i];
                acc = acc + t;
            }
        } else {
            for (long long p = r0 + lane; p < r1; p += 64) acc = acc + ycorr[lrows[p]];
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off);
        if (lane == 0) ssum[wv] = acc;
    }
    __syncthreads();
    if (!live || lane != 0 || m != 0) return;
    const TupScr T = tup_scr(scr, q, k);
    const double iVarE = sc->iVarE;
    const double *W = wd + (size_t)l * (size_t)(k * k);
    double uo[NGP_KMAX], LHS[NGP_KMAX * NGP_KMAX], inv[NGP_KMAX * NGP_KMAX], L[NGP_KMAX * NGP_KMAX], z[NGP_KMAX];
    for (int a = 0; a < k; a++) uo[a] = u[l * k + a];
    for (int a = 0; a < k; a++) {
        double t = 0.0;
        for (int b = 0; b < k; b++) {
            const double p = W[a * k + b] * uo[b];
            t = t + p;
        }
        const double tot = ssum[j * k + a] + t;
        T.Yi[l * k + a] = tot * iVarE;
    }
    const double kd = kdiag[l];
    for (int a = 0; a < k * k; a++) {
        const double t1 = W[a] * iVarE;
        const double t2 = kd * T.sig[a];
        LHS[a] = t1 + t2;
    }
    int bad = t_spd_inv(LHS, k, inv);
    bad |= t_chol(inv, k, L);
    for (int b = 0; b < k; b++) {
        Rng r = rng_seed(seed, chain, it, NGP_KIND_U_NORMAL, ((uint64_t)rset << 40) | (uint64_t)(l * k + b));
        z[b] = rng_normal(r);
    }
    for (int a = 0; a < k * k; a++) T.inv[(size_t)l * (size_t)(k * k) + a] = inv[a];
    for (int a = 0; a < k; a++) {
        double t = 0.0;
        for (int b = 0; b <= a; b++) {
            const double p = L[a * k + b] * z[b];
            t = t + p;
        }
        T.tz[l * k + a] = bad ? __builtin_nan("") : t;  // a matrix that is not positive definite poisons the chain visibly
    }
    double dhi[NGP_KMAX];
    for (int a = 0; a < k; a++) dhi[a] = 0.0;
    for (long long p = kptr[l]; p < kptr[l + 1]; p++) {
        const long long c = kcol[p];
        if (c > l) {
            const double kv = kval[p];
            for (int a = 0; a < k; a++) {
                const double t = kv * u[c * k + a];
                dhi[a] = dhi[a] + t;
            }
        }
    }
    for (int a = 0; a < k; a++) T.dhi[l * k + a] = dhi[a];
}

// ------------------------------------------------------------------------------------------
// One row of the Gauss-Seidel (src/functions.jl:75-89 with the W blocks), every sum from 0.0 with ascending index:
//   dlo_a = sum over the entries of row l of K with column c < l of (K_lc * u_c,a)                       (values of this sweep)
//   wlo_a = sum over the off-diagonal W blocks of row l with column c < l, then b, of (W_lc[a][b] * du_c,b)
//   d_a = dlo_a + dhi_a;  sd_a = sum_b (Sigma_i_ab * d_b);  t = iVarE * wlo_a;  r = Yi_a - t;  rhs_a = r - sd_a
//   mean_a = sum_b (inv_ab * rhs_b);  u_a = mean_a + tz_a;  du_a = u_a(new) - u_a(old)
// wptr / wcol / wval: CSR of the off-diagonal W blocks, columns ascending, k k doubles per entry.  uu: u, or its copy in LDS.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ void tup_gs_row(long long l, int k, const long long *__restrict__ kptr, const int *__restrict__ kcol,
                                           const double *__restrict__ kval, const long long *__restrict__ wptr, const int *__restrict__ wcol,
                                           const double *__restrict__ wval, double *uu, const TupScr &T, double iVarE) {
    double d[NGP_KMAX], wlo[NGP_KMAX], rhs[NGP_KMAX];
    for (int a = 0; a < k; a++) { d[a] = 0.0; wlo[a] = 0.0; }
    for (long long p = kptr[l]; p < kptr[l + 1]; p++) {
        const long long c = kcol[p];
        if (c < l) {
            const double kv = kval[p];
            for (int a = 0; a < k; a++) {
                const double t = kv * uu[c * k + a];
                d[a] = d[a] + t;
            }
        }
    }
    for (long long p = wptr[l]; p < wptr[l + 1]; p++) {
        const long long c = wcol[p];
        if (c < l) {
            const double *Wb = wval + (size_t)p * (size_t)(k * k);
            for (int a = 0; a < k; a++)
                for (int b = 0; b < k; b++) {
                    const double t = Wb[a * k + b] * T.du[c * k + b];
                    wlo[a] = wlo[a] + t;
                }
        }
    }
    for (int a = 0; a < k; a++) d[a] = d[a] + T.dhi[l * k + a];
    for (int a = 0; a < k; a++) {
        double sd = 0.0;
        for (int b = 0; b < k; b++) {
            const double t = T.sig[a * k + b] * d[b];
            sd = sd + t;
        }
        const double t = iVarE * wlo[a];
        const double r = T.Yi[l * k + a] - t;
        rhs[a] = r - sd;
    }
    const double *inv = T.inv + (size_t)l * (size_t)(k * k);
    for (int a = 0; a < k; a++) {
        double mean = 0.0;
        for (int b = 0; b < k; b++) {
            const double t = inv[a * k + b] * rhs[b];
            mean = mean + t;
        }
        const double un = mean + T.tz[l * k + a];
        T.du[l * k + a] = un - uu[l * k + a];
        uu[l * k + a] = un;
    }
}

// the serial walk: ONE workgroup of one wave, lane 0 walks the levels in order; u in LDS when 8 q k bytes fit (use_lds)
__global__ __launch_bounds__(64) void k_tup_gs(long long q, int k, const long long *__restrict__ kptr, const int *__restrict__ kcol,
                                               const double *__restrict__ kval, const long long *__restrict__ wptr, const int *__restrict__ wcol,
                                               const double *__restrict__ wval, double *__restrict__ u, double *scr,
                                               const DScal *__restrict__ sc, int use_lds, const unsigned *__restrict__ abort_w) {
    extern __shared__ double su[];
    if (abort_w && *abort_w != 0u) return;
    const int tid = threadIdx.x;
    const long long qk = q * k;
    double *uu = use_lds ? su : u;
    if (use_lds) {
        for (long long a = tid; a < qk; a += 64) su[a] = u[a];
        __syncthreads();
    }
    if (tid == 0) {
        const TupScr T = tup_scr(scr, q, k);
        const double iVarE = sc->iVarE;
        for (long long l = 0; l < q; l++) tup_gs_row(l, k, kptr, kcol, kval, wptr, wcol, wval, uu, T, iVarE);
    }
    if (use_lds) {
        __syncthreads();
        for (long long a = tid; a < qk; a += 64) u[a] = su[a];
    }
}

// the level schedule (ngp_random.h, k_rand_sched_*): depth(l) = 0 for a row with no entry of K or of the off-diagonal W blocks left of
// its diagonal, else 1 + max depth(c) over those columns c < l.  A row reads the u and du only of rows of smaller depth.
__global__ __launch_bounds__(256) void k_tup_sched_wide(long long q, int k, const long long *__restrict__ kptr, const int *__restrict__ kcol,
                                                        const double *__restrict__ kval, const long long *__restrict__ wptr,
                                                        const int *__restrict__ wcol, const double *__restrict__ wval, double *u, double *scr,
                                                        const DScal *__restrict__ sc, const int *__restrict__ order, long long r0, long long r1,
                                                        const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    const long long i = r0 + (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= r1) return;
    const TupScr T = tup_scr(scr, q, k);
    tup_gs_row((long long)order[i], k, kptr, kcol, kval, wptr, wcol, wval, u, T, sc->iVarE);
}

__global__ __launch_bounds__(1024) void k_tup_sched_fused(long long q, int k, const long long *__restrict__ kptr, const int *__restrict__ kcol,
                                                          const double *__restrict__ kval, const long long *__restrict__ wptr,
                                                          const int *__restrict__ wcol, const double *__restrict__ wval, double *u, double *scr,
                                                          const DScal *__restrict__ sc, const int *__restrict__ order,
                                                          const long long *__restrict__ dptr, int d0, int d1, const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;  // (uniform over the workgroup)
    const TupScr T = tup_scr(scr, q, k);
    const double iVarE = sc->iVarE;
    for (int d = d0; d < d1; d++) {  // (uniform: every thread meets every barrier)
        const long long r1 = dptr[d + 1];
        for (long long i = dptr[d] + threadIdx.x; i < r1; i += 1024) tup_gs_row((long long)order[i], k, kptr, kcol, kval, wptr, wcol, wval, u, T, iVarE);
        __threadfence_block();
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------
// ycorr_i -= t,  t = sum over the components m in order with level_m(i) >= 0 of du[level_m(i) k + m], from 0.0;  weighted: s_i t
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_tup_update(double *__restrict__ ycorr, const double *__restrict__ rs, long long N, int k,
                                                    const int *__restrict__ level, const double *__restrict__ du,
                                                    const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N) return;
    double t = 0.0;
    for (int m = 0; m < k; m++) {
        const long long lv = level[(long long)m * N + i];
        if (lv >= 0) t = t + du[lv * k + m];
    }
    if (rs) t = rs[i] * t;
    ycorr[i] = ycorr[i] - t;
}

// ------------------------------------------------------------------------------------------
// varU (src/functions.jl:503-506), ONE workgroup of 1024 threads.  Thread t takes the levels t, t + 1024, ...: per level
//   r_b = sum over row l of K, ascending columns, of (K_lc * u_c,b) (from 0.0);  for a <= b: acc_ab = acc_ab + (u_l,a * r_b)
// then per pair the butterfly inside each wave and the 16 wave sums added in wave order: S_ab = S_ba.  Psi = scale + S, and
// varU ~ InverseWishart(df + q, Psi) by the Bartlett construction of k_tuple_draw (ngp_kernels.h): Pi = inv(Psi), L = chol(Pi),
// A lower triangular with A_ii = sqrt(chi2(nu - i)), A_ij normal, varU = inv((L A)(L A)').  Keys: (0, 0) is (NGP_KIND_U_CHI2, set),
// every other (i, j) is (NGP_KIND_U_WISHART, (set << 40) | (i << 4) | j).
// ------------------------------------------------------------------------------------------
#define NGP_TUP_PAIRS (NGP_KMAX * (NGP_KMAX + 1) / 2)
__global__ __launch_bounds__(1024) void k_tup_var(long long q, int k, const long long *__restrict__ kptr, const int *__restrict__ kcol,
                                                  const double *__restrict__ kval, const double *__restrict__ u, double *__restrict__ vu,
                                                  double df, const double *__restrict__ scale, int rset, uint64_t seed, uint64_t chain,
                                                  uint64_t it, const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    __shared__ double wsum[16][NGP_TUP_PAIRS];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double acc[NGP_TUP_PAIRS];
    for (int p = 0; p < NGP_TUP_PAIRS; p++) acc[p] = 0.0;
    for (long long l = tid; l < q; l += 1024) {
        double r[NGP_KMAX];
        for (int b = 0; b < k; b++) r[b] = 0.0;
        for (long long p = kptr[l]; p < kptr[l + 1]; p++) {
            const double kv = kval[p];
            const long long c = kcol[p];
            for (int b = 0; b < k; b++) {
                const double t = kv * u[c * k + b];
                r[b] = r[b] + t;
            }
        }
        int pr = 0;
        for (int a = 0; a < k; a++)
            for (int b = a; b < k; b++, pr++) {
                const double t = u[l * k + a] * r[b];
                acc[pr] = acc[pr] + t;
            }
    }
    const int npair = k * (k + 1) / 2;
    for (int p = 0; p < npair; p++) {
        double a = acc[p];
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) a = a + __shfl_xor(a, off);
        if (lane == 0) wsum[wv][p] = a;
    }
    __syncthreads();
    if (tid != 0) return;
    double Psi[NGP_KMAX * NGP_KMAX];
    int pr = 0;
    for (int a = 0; a < k; a++)
        for (int b = a; b < k; b++, pr++) {
            double tot = wsum[0][pr];
            for (int w = 1; w < 16; w++) tot = tot + wsum[w][pr];
            Psi[a * k + b] = scale[a * k + b] + tot;
            Psi[b * k + a] = scale[b * k + a] + tot;
        }
    const double nu = df + (double)q;
    double Pi[NGP_KMAX * NGP_KMAX], L[NGP_KMAX * NGP_KMAX], A[NGP_KMAX * NGP_KMAX], LA[NGP_KMAX * NGP_KMAX], Wm[NGP_KMAX * NGP_KMAX], res[NGP_KMAX * NGP_KMAX];
    int bad = t_spd_inv(Psi, k, Pi);
    bad |= t_chol(Pi, k, L);
    for (int a = 0; a < k * k; a++) A[a] = 0.0;
    for (int i = 0; i < k; i++)
        for (int j = 0; j <= i; j++) {
            Rng r = (i == 0) ? rng_seed(seed, chain, it, NGP_KIND_U_CHI2, (uint64_t)rset)
                             : rng_seed(seed, chain, it, NGP_KIND_U_WISHART, ((uint64_t)rset << 40) | ((uint64_t)i << 4) | (uint64_t)j);
            if (i == j) { const double ch = rng_chisq(r, nu - (double)i); A[i * k + i] = det_sqrt(ch); }
            else A[i * k + j] = rng_normal(r);
        }
    for (int i = 0; i < k; i++)
        for (int j = 0; j < k; j++) {
            double s = 0.0;
            for (int m = 0; m < k; m++) s = __builtin_fma(L[i * k + m], A[m * k + j], s);
            LA[i * k + j] = s;
        }
    for (int i = 0; i < k; i++)
        for (int j = 0; j < k; j++) {
            double s = 0.0;
            for (int m = 0; m < k; m++) s = __builtin_fma(LA[i * k + m], LA[j * k + m], s);
            Wm[i * k + j] = s;
        }
    bad |= t_spd_inv(Wm, k, res);
    for (int a = 0; a < k * k; a++) vu[a] = bad ? __builtin_nan("") : res[a];
}

}  // namespace ngp
