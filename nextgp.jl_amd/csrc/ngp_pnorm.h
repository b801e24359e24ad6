// ngp_pnorm.h -- the standard normal distribution function of the draw layer and the log of an interval's mass (DESIGN.md section 2,
// "Normal distribution function").  det_pnorm(x) = Phi(x), det_lpdiff(a, b) = log(Phi(b) - Phi(a)).  As everything in ngp_rng.h: a
// fixed, written-down sequence of IEEE-754 double operations (no contraction), built on det_exp / det_log, so that a host restates it
// bit for bit (tests/ref_threshold.py).  Every loop has a constant trip count.
//
// Phi by the rational error functions of the Cephes library (S. L. Moshier, ndtr.c / erf.c / erfc.c, release 2.2, after W. J. Cody,
// "Rational Chebyshev approximations for the error function", Math. Comp. 23 (1969)): with z = x / sqrt 2,
//   |z| < 1        erf(z) = z T(z^2) / U(z^2),                Phi = 0.5 + 0.5 erf(z)
//   1 <= |z| < 8   erfc(|z|) = exp(-z^2) P(|z|) / Q(|z|)      Phi = erfc / 2 (x < 0), 1 - erfc / 2 (x > 0)
//   8 <= |z|       erfc(|z|) = exp(-z^2) R(|z|) / S(|z|)
// The lower tail keeps its relative accuracy down to where exp(-z^2) leaves det_exp's range (z^2 > 708, x < -37.6: Phi = 0).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ngp_rng.h"

#pragma clang fp contract(off)

namespace ngp {

// Horner in the order written: c[0] is the coefficient of the highest power
template <int N>
__device__ inline double pn_horner(const double (&c)[N], double x) {
    double r = c[0];
#pragma unroll
    for (int i = 1; i < N; i++) r = r * x + c[i];
    return r;
}

__device__ inline double det_pnorm(double x) {
    const double T[5] = {9.60497373987051638749E0, 9.00260197203842689217E1, 2.23200534594684319226E3, 7.00332514112805075473E3,
                         5.55923013010394962768E4};
    const double U[6] = {1.0, 3.35617141647503099647E1, 5.21357949780152679795E2, 4.59432382970980127987E3, 2.26290000613890934246E4,
                         4.92673942608635921086E4};
    const double P[9] = {2.46196981473530512524E-10, 5.64189564831068821977E-1, 7.46321056442269912687E0, 4.86371970985681366614E1,
                         1.96520832956077098242E2,   5.26445194995477358631E2,  9.34528527171957607540E2, 1.02755188689515710272E3,
                         5.57535335369399327526E2};
    const double Q[9] = {1.0, 1.32281951154744992508E1, 8.67072140885989742329E1, 3.54937778887819891062E2, 9.75708501743205489753E2,
                         1.82390916687909736289E3, 2.24633760818710981792E3, 1.65666309194161350182E3, 5.57535340817727675546E2};
    const double R[6] = {5.64189583547755073984E-1, 1.27536670759978104416E0, 5.01905042251180477414E0, 6.16021097993053585195E0,
                         7.40974269950448939160E0,  2.97886665372100240670E0};
    const double S[7] = {1.0, 2.26052863220117276590E0, 9.39603524938001434673E0, 1.20489539808096656605E1, 1.70814450747565897222E1,
                         9.60896809063285878198E0, 3.36907645100081516050E0};
    if (x != x) return x;
    const double z = x * 0.70710678118654752440;  // 1 / sqrt 2
    const double az = __builtin_fabs(z);
    if (az < 1.0) {
        const double zz = z * z;
        const double num = pn_horner(T, zz);
        const double den = pn_horner(U, zz);
        const double e = (z * num) / den;
        return 0.5 + 0.5 * e;
    }
    const double q = -(az * az);
    if (q < -708.0) return z > 0.0 ? 1.0 : 0.0;  // (also the two infinities)
    const double ex = det_exp(q);
    double num, den;
    if (az < 8.0) {
        num = pn_horner(P, az);
        den = pn_horner(Q, az);
    } else {
        num = pn_horner(R, az);
        den = pn_horner(S, az);
    }
    const double y = 0.5 * ((ex * num) / den);
    return z > 0.0 ? 1.0 - y : y;
}

// log(Phi(b) - Phi(a)) for a < b, either bound possibly infinite, on the side that does not cancel: 0 <= a takes Phi(-a) - Phi(-b).
// Bounds that are not a < b (a NaN among them), and an interval whose mass is no positive double, give -inf.
__device__ inline double det_lpdiff(double a, double b) {
    const double ninf = -__builtin_huge_val();
    if (!(a < b)) return ninf;
    const double p = (a >= 0.0) ? det_pnorm(-a) - det_pnorm(-b) : det_pnorm(b) - det_pnorm(a);
    if (!(p > 0.0)) return ninf;
    return det_log(p);
}

// probe (ngp_debug_pnorm): which 0: det_pnorm(a[i]); 1: det_lpdiff(a[i], b[i])
__global__ __launch_bounds__(256) void k_debug_pnorm(int which, const double *__restrict__ a, const double *__restrict__ b, long long n,
                                                     double *__restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    out[i] = which == 0 ? det_pnorm(a[i]) : det_lpdiff(a[i], b[i]);
}

}  // namespace ngp
