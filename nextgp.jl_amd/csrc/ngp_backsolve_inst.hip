// The kernels of the SNP back-solve (ngp_backsolve.h) and their launches: one translation unit, beside the API unit, the genomic-variance
// unit and the sweep units, so that none of those carries code it did not carry before (code beside the hot loops costs).
#define NGP_BACKSOLVE_KERNELS
#include "ngp_backsolve.h"

namespace ngp {

hipError_t backsolve_store(long long q, const double *u, double *dst, const unsigned *abort_w, hipStream_t stream) {
    hipLaunchKernelGGL(k_bs_store, dim3((unsigned)((q + 255) / 256)), dim3(256), 0, stream, q, u, dst, abort_w);
    return hipGetLastError();
}

hipError_t backsolve_kw(const double *K, long long ld, long long q, const double *U, long long T, double *W, double *cw, hipStream_t stream) {
    if (q < 1 || T < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bs_kw, dim3((unsigned)((q + 63) / 64), (unsigned)((T + 63) / 64)), dim3(256), 0, stream, K, ld, q, U, T, W);
    hipLaunchKernelGGL(k_bs_cw, dim3((unsigned)T), dim3(64), 0, stream, (const double *)W, q, cw);
    return hipGetLastError();
}

hipError_t backsolve_cw(const double *W, long long q, long long T, double *cw, hipStream_t stream) {
    if (q < 1 || T < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bs_cw, dim3((unsigned)T), dim3(64), 0, stream, W, q, cw);
    return hipGetLastError();
}

template <typename TIn>
static void launch_cols(const BsCols &c, hipStream_t stream) {
    const TIn *src = (const TIn *)c.src;
    hipLaunchKernelGGL(k_bs_colstats<TIn>, dim3((unsigned)c.nc), dim3(64), 0, stream, src, c.N, c.ld, c.method, (double)c.P, c.sum2pq, c.mu, c.dj, c.bad);
    hipLaunchKernelGGL(k_bs_cols<TIn>, dim3((unsigned)((c.nc + 63) / 64)), dim3(256), 0, stream, src, c.N, c.ld, c.nc, c.W, c.T, c.cw, (const double *)c.mu,
                       (const double *)c.dj, c.sum, c.sumsq);
}

hipError_t backsolve_columns(const BsCols &c, hipStream_t stream) {
    if (c.nc < 1 || c.N < 1 || c.T < 1 || c.ld < c.N) return hipErrorInvalidValue;
    switch (c.type) {
        case 0: launch_cols<double>(c, stream); break;
        case 1: launch_cols<float>(c, stream); break;
        case 2: launch_cols<uint8_t>(c, stream); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t backsolve_project(const double *Ct, long long N, long long Nc, const double *W, long long T, const double *cw, const double *mu0, const double *d1,
                             double *sum, double *sumsq, hipStream_t stream) {
    if (N < 1 || Nc < 1 || T < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_bs_cols<double>, dim3((unsigned)((Nc + 63) / 64)), dim3(256), 0, stream, Ct, N, N, Nc, W, T, cw, mu0, d1, sum, sumsq);
    return hipGetLastError();
}

}  // namespace ngp
