// The kernels of GBLUP prediction (ngp_gpred.h) and their launches: one translation unit beside the back-solve's, so that neither the API
// unit nor the sweep units carry code they did not carry before (code beside the hot loops costs).
#define NGP_GPRED_KERNELS
#include "ngp_gpred.h"

namespace ngp {

static bool gp_ok(const GpCols &c) {
    // (the records' tiles lie along the grid's second dimension, which ends at 65535)
    return c.nc >= 1 && c.N >= 1 && c.Nc >= 1 && c.ldt >= c.N && c.ldc >= c.Nc && (c.N + 63) / 64 <= 65535 && 2 * c.nc <= 0x7FFFFFFFLL;
}

template <typename TIn>
static void launch_stats(const GpCols &c, hipStream_t stream) {
    hipLaunchKernelGGL(k_gp_colstats<TIn>, dim3((unsigned)(2 * c.nc)), dim3(64), 0, stream, (const TIn *)c.train, c.N, c.ldt, (const TIn *)c.cand, c.Nc, c.ldc,
                       c.nc, c.method, c.mu, c.sd, c.bad);
}

template <typename TIn>
static void launch_cross(const GpCols &c, hipStream_t stream) {
    hipLaunchKernelGGL(k_gp_cross<TIn>, dim3((unsigned)((c.Nc + 63) / 64), (unsigned)((c.N + 63) / 64)), dim3(256), 0, stream, (const TIn *)c.train, c.N, c.ldt,
                       (const TIn *)c.cand, c.Nc, c.ldc, c.nc, c.method, (const double *)c.mu, (const double *)c.sd, c.Ct, c.gcc);
}

hipError_t gpred_colstats(const GpCols &c, hipStream_t stream) {
    if (!gp_ok(c)) return hipErrorInvalidValue;
    switch (c.type) {
        case 0: launch_stats<double>(c, stream); break;
        case 1: launch_stats<float>(c, stream); break;
        case 2: launch_stats<uint8_t>(c, stream); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t gpred_cross(const GpCols &c, hipStream_t stream) {
    if (!gp_ok(c)) return hipErrorInvalidValue;
    switch (c.type) {
        case 0: launch_cross<double>(c, stream); break;
        case 1: launch_cross<float>(c, stream); break;
        case 2: launch_cross<uint8_t>(c, stream); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t gpred_scale(double *Ct, long long N, long long Nc, double *gcc, double denom, hipStream_t stream) {
    if (N < 1 || Nc < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_gp_scale, dim3((unsigned)((N + 255) / 256), (unsigned)(Nc < 65535 ? Nc : 65535)), dim3(256), 0, stream, Ct, N, Nc, gcc, denom);
    return hipGetLastError();
}

hipError_t gpred_resid(const double *Ct, const double *V, long long N, long long Nc, const double *gcc, double *s, hipStream_t stream) {
    if (N < 1 || Nc < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_gp_resid, dim3((unsigned)Nc), dim3(64), 0, stream, Ct, V, N, gcc, s);
    return hipGetLastError();
}

hipError_t gpred_fill(double *p, long long n, double v, hipStream_t stream) {
    if (n < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_gp_fill, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, p, n, v);
    return hipGetLastError();
}

}  // namespace ngp
