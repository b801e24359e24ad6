// ngp_diag.h -- convergence diagnostics of the kept draws ("Convergence diagnostics"): a streaming lag-window
// autocovariance of every monitored scalar, one bandwidth-bound update behind each kept iteration, and a finalising kernel that turns
// the sums into mean, variance, ESS and MCSE per parameter (Geyer's initial positive sequence inside the window: bench.py's ess_geyer
// with the autocovariances of lags >= L unknown).
//
// The monitored vector theta[D] is the doubles of the sample record in record order (ngp_state.h, diag_layout).  k_diag_gather copies
// it out of the chain's arrays and device structs by a table built from that layout -- there is no second description of the model.
//
// State per chain, fp64, every row D doubles (on the device the rows lie Dp = D rounded up to even apart, so that every row starts on
// 16 bytes and a lane takes two parameters as a double2; the pad column sees x = 0 and stays 0):
//     x1[D] | S1[2][D] | S2[2][D] | C[L][D] | head[L][D] | ring[L][D]                                   (3 L + 5 rows)
// Draw t (0-based) of value x, split H (draws t < H feed half 0), every product and sum rounded on its own (-ffp-contract=off):
//     if t == 0: x1 = x
//     y = x - x1
//     for k in 1 .. min(t, L-1): C[k] += y * ring[(t-k) mod L]
//     h = t < H ? 0 : 1;  S1[h] += y;  S2[h] += y*y
//     if t < L: head[t] = y
//     ring[t mod L] = y
// Row 0 of C is never written.  Element-wise over D: no atomics, no LDS, no cross-lane traffic; every access is a coalesced row.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace ngp {

#define NGP_DIAG_MAXL 256   // lags of the window: even, 2 .. 256
#define NGP_DIAG_UN 8       // lags whose loads are issued ahead of their read-modify-writes
#define NGP_DIAG_OUT 9      // rows of k_diag_finalise's output: mean | var | ess | mcse | truncated | half_mean[2] | half_var[2]

// one run of theta: `words` doubles at src go to x + off
struct DiagSeg {
    const double *src;
    long long off, words;
};

// rows of the state, in units of the row stride
struct DiagRows {
    static constexpr long long x1 = 0, S1 = 1, S2 = 3, C = 5;
    __host__ __device__ static long long head(int L) { return 5 + (long long)L; }
    __host__ __device__ static long long ring(int L) { return 5 + 2 * (long long)L; }
    __host__ __device__ static long long rows(int L) { return 5 + 3 * (long long)L; }
};

// theta of this draw into x: block (b, s) copies words [256 b, 256 b + 256) of segment s
__global__ __launch_bounds__(256) void k_diag_gather(const DiagSeg *__restrict__ segs, double *__restrict__ x, const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    const DiagSeg g = segs[blockIdx.y];
    const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
    if (k < g.words) x[g.off + k] = g.src[k];
}

// the update for draw t: one lane per pair of parameters (np = Dp / 2 pairs, st the state with rows of np double2)
__global__ __launch_bounds__(256) void k_diag_update(const double2 *__restrict__ x, double2 *__restrict__ st, long long np, int L, long long t, long long H,
                                                     const unsigned *__restrict__ abort_w) {
    if (abort_w && *abort_w != 0u) return;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= np) return;
    double2 *const x1 = st + DiagRows::x1 * np, *const S1 = st + DiagRows::S1 * np, *const S2 = st + DiagRows::S2 * np, *const C = st + DiagRows::C * np;
    double2 *const head = st + DiagRows::head(L) * np, *const ring = st + DiagRows::ring(L) * np;
    const double2 xv = x[i];
    double2 a;
    if (t == 0) { a = xv; x1[i] = xv; } else a = x1[i];
    double2 y;
    y.x = xv.x - a.x; y.y = xv.y - a.y;
    const int kmax = (int)(t < (long long)(L - 1) ? t : (long long)(L - 1));
    int slot = (int)((t + (long long)L - 1) % (long long)L);  // (t - k) mod L at k = 1; one down per lag, wrapping
    for (int k0 = 1; k0 <= kmax; k0 += NGP_DIAG_UN) {
        double2 r[NGP_DIAG_UN], c[NGP_DIAG_UN];
        int s = slot;
#pragma unroll
        for (int u = 0; u < NGP_DIAG_UN; u++) {  // the loads of this group of lags, all independent
            if (k0 + u <= kmax) {
                r[u] = ring[(long long)s * np + i];
                c[u] = C[(long long)(k0 + u) * np + i];
            }
            s = s == 0 ? L - 1 : s - 1;
        }
#pragma unroll
        for (int u = 0; u < NGP_DIAG_UN; u++)
            if (k0 + u <= kmax) {
                double2 p;
                p.x = y.x * r[u].x; p.y = y.y * r[u].y;
                c[u].x = c[u].x + p.x; c[u].y = c[u].y + p.y;
                C[(long long)(k0 + u) * np + i] = c[u];
            }
        slot = s;
    }
    const long long hh = t < H ? 0 : 1;
    double2 s1 = S1[hh * np + i], s2 = S2[hh * np + i], q;
    q.x = y.x * y.x; q.y = y.y * y.y;
    s1.x = s1.x + y.x; s1.y = s1.y + y.y;
    s2.x = s2.x + q.x; s2.y = s2.y + q.y;
    S1[hh * np + i] = s1; S2[hh * np + i] = s2;
    if (t < (long long)L) head[t * np + i] = y;
    ring[(t % (long long)L) * np + i] = y;
}

// One thread per parameter: the sums of n draws into out[NGP_DIAG_OUT][D] ("Convergence diagnostics", finalise).
// st: the state with rows ld doubles apart.
__global__ __launch_bounds__(256) void k_diag_finalise(const double *__restrict__ st, long long ld, long long D, int L, long long n, long long H,
                                                       double *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= D) return;
    const double *const S1 = st + DiagRows::S1 * ld, *const S2 = st + DiagRows::S2 * ld, *const C = st + DiagRows::C * ld;
    const double *const head = st + DiagRows::head(L) * ld, *const ring = st + DiagRows::ring(L) * ld;
    const double nan = __builtin_nan("");
    const double x1 = st[i], dn = (double)n;
    const double s1 = S1[i] + S1[ld + i], s2 = S2[i] + S2[ld + i];
    const double m = s1 / dn;
    const double ms1 = m * s1;
    const double g0 = s2 - ms1;
    const double var = n < 2 ? nan : g0 / (double)(n - 1);
    double ess = dn, trunc = 0.0;
    if (n >= 4 && g0 > 0.0) {
        const long long K = (long long)L < n ? (long long)L : n;
        const double mm = m * m;
        double hs = 0.0, ts = 0.0, tau = -1.0, gprev = g0;
        bool hit = false;
        for (long long k = 1; k < K; k++) {
            hs = hs + head[(k - 1) * ld + i];
            ts = ts + ring[((n - k) % (long long)L) * ld + i];
            const double a = s1 - hs, b = s1 - ts;
            const double ab = a + b;
            const double mab = m * ab;
            const double w = (double)(n - k) * mm;
            const double gk = (C[k * ld + i] - mab) + w;
            if (k & 1) {  // the pair (G[k-1], G[k])
                const double pair = (gprev + gk) / g0;
                if (!(pair > 0.0)) { hit = true; break; }
                tau = tau + 2.0 * pair;
            } else gprev = gk;
        }
        trunc = (!hit && K < n) ? 1.0 : 0.0;
        const double d = tau > 1e-12 ? tau : 1e-12;
        const double e = dn / d;
        ess = e < dn ? e : dn;
    }
    out[i] = m + x1;
    out[D + i] = var;
    out[2 * D + i] = ess;
    out[3 * D + i] = sqrt(var / ess);
    out[4 * D + i] = trunc;
    const long long n0 = n < H ? n : H;
    for (int hh = 0; hh < 2; hh++) {
        const long long nh = hh == 0 ? n0 : n - n0;
        const double dh = (double)nh, a = S1[hh * ld + i], b = S2[hh * ld + i];
        const double mh = a / dh;
        const double mha = mh * a;
        out[(5 + hh) * D + i] = nh < 1 ? nan : mh + x1;
        out[(7 + hh) * D + i] = nh < 2 ? nan : (b - mha) / (double)(nh - 1);
    }
}

}  // namespace ngp
