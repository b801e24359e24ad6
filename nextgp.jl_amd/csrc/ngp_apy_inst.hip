// The kernels of APY random-effect sets (ngp_apy.h) and their launches: one translation unit beside the back-solve's and the
// prediction's, so that neither the API unit nor the sweep units carry code they did not carry before.
#define NGP_APY_KERNELS
#include "ngp_apy.h"
#include "ngp_backsolve.h"  // (declarations only: backsolve_cw launches k_bs_cw from the back-solve's unit)

namespace ngp {

static bool apy_ok(const ApyStep &a) { return a.nc >= 1 && a.nc <= NGP_APY_MAX_CORE && a.q >= a.nc && a.ldp >= a.nc && a.ldk >= a.nc; }

// the instantiation is a function of nc alone: cores of at most 2,048 take 4 columns per thread and 8 rows per step, larger ones 16 and 4
template <int DRAW>
static void launch_tail(const ApyStep &a, hipStream_t stream) {
    const unsigned nwg = (unsigned)apy_tail_wgs(a.q - a.nc);
    if (a.nc <= 4 * NGP_APY_T) hipLaunchKernelGGL((k_apy_tail<4, 8, DRAW>), dim3(nwg), dim3(NGP_APY_T), 0, stream, a);
    else hipLaunchKernelGGL((k_apy_tail<16, 4, DRAW>), dim3(nwg), dim3(NGP_APY_T), 0, stream, a);
}

hipError_t apy_seed(const ApyStep &a, hipStream_t stream) {
    if (!apy_ok(a)) return hipErrorInvalidValue;
    const long long nn = a.q - a.nc;
    if (nn > 0) {
        hipLaunchKernelGGL(k_apy_check, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, stream, nn, (const double *)(a.u + a.nc), (const double *)a.uprev, a.stale,
                           a.abort_w);
        launch_tail<0>(a, stream);
        hipLaunchKernelGGL(k_apy_reduce, dim3((unsigned)((a.nc + 255) / 256)), dim3(256), 0, stream, a.nc, apy_tail_wgs(nn), (const double *)a.spart,
                           (const double *)a.qpart, a.s, a.quad, 1, (const unsigned *)a.stale, a.abort_w);
    }
    hipLaunchKernelGGL(k_apy_seed, dim3((unsigned)((a.nc + 255) / 256)), dim3(256), 0, stream, a.nc, (const double *)a.s, a.acc, a.acc0, a.seed, a.stale, a.abort_w);
    return hipPeekAtLastError();  // (not cleared: the caller of the step checks the stream's launches once)
}

hipError_t apy_tail(const ApyStep &a, hipStream_t stream) {
    if (!apy_ok(a)) return hipErrorInvalidValue;
    const long long nn = a.q - a.nc;
    if (nn <= 0) return hipSuccess;  // (all core: s and the tail's quadratic term stay the zeros they were created as)
    launch_tail<1>(a, stream);
    hipLaunchKernelGGL(k_apy_reduce, dim3((unsigned)((a.nc + 255) / 256)), dim3(256), 0, stream, a.nc, apy_tail_wgs(nn), (const double *)a.spart,
                       (const double *)a.qpart, a.s, a.quad, 0, (const unsigned *)a.stale, a.abort_w);
    return hipPeekAtLastError();  // (not cleared: the caller of the step checks the stream's launches once)
}

hipError_t apy_var(const ApyStep &a, double *vu, double df, double scale, int rset, uint64_t seed, uint64_t chain, uint64_t it, hipStream_t stream) {
    if (!apy_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_apy_quad0, dim3((unsigned)((a.nc + 3) / 4)), dim3(256), 0, stream, a.Kc0, a.ldk, a.nc, (const double *)a.u, a.dlo, a.abort_w);
    hipLaunchKernelGGL(k_apy_var, dim3(1), dim3(1024), 0, stream, a.q, a.nc, a.kdiag0, (const double *)a.u, (const double *)a.dlo, a.quad, vu, df, scale, rset, seed,
                       chain, it, a.abort_w);
    return hipPeekAtLastError();  // (not cleared: the caller of the step checks the stream's launches once)
}

hipError_t apy_rownorm(const double *xc, long long Npad, long long N, long long cpad, double *gdiag, hipStream_t stream) {
    if (N < 1 || Npad < N || cpad < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_apy_rownorm, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, stream, xc, Npad, N, cpad, gdiag);
    return hipGetLastError();
}

hipError_t apy_finish(double *panel, long long N, long long ld, long long nc, double *gdiag, double denom, hipStream_t stream) {
    if (N < 1 || ld < N || nc < 1 || nc > N) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_apy_finish, dim3((unsigned)((N + 255) / 256), (unsigned)(nc < 65535 ? nc : 65535)), dim3(256), 0, stream, panel, N, ld, nc, gdiag, denom);
    return hipGetLastError();
}

hipError_t apy_gemm_p(const double *panel, long long N, long long Npad, long long nc, const double *Kc0, long long ldk, double *P, long long ldp, hipStream_t stream) {
    const long long nn = N - nc;
    if (nn < 1 || nc < 1 || ldk % 64 != 0 || ldk < nc || ldp < ldk || Npad < N) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_apy_gemm_p, dim3((unsigned)((nn + 63) / 64), (unsigned)(ldk / 64)), dim3(256), 0, stream, panel, N, Npad, nc, Kc0, ldk, P, ldp);
    return hipGetLastError();
}

hipError_t apy_m(const double *panel, long long Npad, long long nc, long long nn, const double *P, long long ldp, const double *gdiag, double *m, double *d,
                 hipStream_t stream) {
    if (nn < 1 || nc < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_apy_m, dim3((unsigned)((nn + 3) / 4)), dim3(256), 0, stream, panel, Npad, nc, nn, P, ldp, gdiag, m, d);
    return hipGetLastError();
}

hipError_t apy_gemm_kcc(const double *P, long long ldp, long long nnpad, const double *d, double *Kcc, long long ldk, hipStream_t stream) {
    if (nnpad < 4 || nnpad % 4 != 0 || ldk % 64 != 0 || ldp < ldk) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_apy_gemm_kcc, dim3((unsigned)(ldk / 64), (unsigned)(ldk / 64)), dim3(256), 0, stream, P, ldp, nnpad, d, Kcc, ldk);
    return hipGetLastError();
}

hipError_t apy_digest(const double *A, long long rows, long long cols, long long ld, unsigned long long *rowhash, hipStream_t stream) {
    if (rows < 1 || cols < 1 || ld < cols) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_apy_digest, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, stream, A, rows, cols, ld, rowhash);
    return hipGetLastError();
}

// the tail first (Wn), then the core (it reads Wn), then the column sums over the finished W; all core: k_apy_kw_core alone
hipError_t apy_kw(const ApyKw &k, const double *X, long long T, double *W, double *cw, hipStream_t stream) {
    const long long nn = k.N - k.nc;
    if (k.nc < 1 || k.nc > NGP_APY_MAX_CORE || nn < 0 || T < 1 || T > 64LL * 65535 || k.ldp < k.nc || k.ldp % 64 != 0 || k.ldk < k.nc) return hipErrorInvalidValue;
    const unsigned gt = (unsigned)((T + 63) / 64);
    if (nn > 0) {
        const hipError_t e = hipFuncSetAttribute((const void *)k_apy_kw_tail, hipFuncAttributeMaxDynamicSharedMemorySize, (int)NGP_APY_KW_TAIL_LDS);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_apy_kw_tail, dim3((unsigned)((nn + 63) / 64), gt), dim3(256), NGP_APY_KW_TAIL_LDS, stream, k.P, k.ldp, k.d, k.N, k.nc, X, T, W);
    }
    hipLaunchKernelGGL(k_apy_kw_core, dim3((unsigned)((k.nc + 63) / 64), gt), dim3(256), 0, stream, k.Kc0, k.ldk, k.P, k.ldp, k.N, k.nc, X, T, W);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : backsolve_cw(W, k.N, T, cw, stream);
}

}  // namespace ngp
