// The kernels of the genomic-variance pass (ngp_genvar.h) and their launches: one translation unit, beside the API unit and the
// five sweep units, so that none of those carries code it did not carry before (code beside the hot loops costs).
#define NGP_GENVAR_KERNELS
#include "ngp_genvar.h"

#include <cstring>

namespace ngp {

hipError_t genvar_prepare() {
    hipError_t e = hipSuccess;
#define NGP_GV_ATTR(KK)                                                                                                                              \
    if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k_genvar<KK, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)genvar_lds_bytes(KK, true)); \
    if (e == hipSuccess) e = hipFuncSetAttribute((const void *)k_genvar<KK, false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)genvar_lds_bytes(KK, false));
    NGP_GV_ATTR(1) NGP_GV_ATTR(2) NGP_GV_ATTR(3) NGP_GV_ATTR(4) NGP_GV_ATTR(5) NGP_GV_ATTR(6) NGP_GV_ATTR(7) NGP_GV_ATTR(8)
#undef NGP_GV_ATTR
    return e;
}

hipError_t genvar_xmax(const void *tiles, const double *mean, int u8, long long N, long long L, long long nblk, unsigned long long *out, hipStream_t stream) {
    const dim3 grid((unsigned)nblk, (unsigned)((N + 255) / 256));
    if (u8) hipLaunchKernelGGL(k_genvar_xmax<true>, grid, dim3(256), 0, stream, tiles, mean, N, L, out);
    else hipLaunchKernelGGL(k_genvar_xmax<false>, grid, dim3(256), 0, stream, tiles, mean, N, L, out);
    return hipGetLastError();
}

hipError_t genvar_launch(const GvLaunch &q) {
    const GvArgs &A = q.A;
    const int n = q.n;
    if (n < 1 || n > NGP_GV_MAXK) return hipErrorInvalidValue;
    const bool u8 = q.u8 != 0;
    hipStream_t st = q.stream;
    unsigned *ab = q.abort_w;
    const size_t lds = genvar_lds_bytes(n, u8);
    if (u8)
        hipLaunchKernelGGL(k_genvar_prep<true>, dim3((unsigned)q.nseg, (unsigned)n), dim3(64), 0, st, q.segs, q.mean, A, (const unsigned *)ab);
    else
        hipLaunchKernelGGL(k_genvar_prep<false>, dim3((unsigned)q.nseg, (unsigned)n), dim3(64), 0, st, q.segs, q.mean, A, (const unsigned *)ab);
    hipLaunchKernelGGL(k_genvar_scale, dim3((unsigned)((q.nslots + 255) / 256), (unsigned)n), dim3(256), 0, st, q.slot_seg, q.set_seg0, q.nwin, q.nsets, q.ex, A,
                       (const unsigned *)ab);
    const dim3 grid((unsigned)q.nitems, (unsigned)q.ncol_w);
#define NGP_GV_CASE(KK)                                                                                                                   \
    case KK:                                                                                                                              \
        if (u8) {                                                                                                                         \
            hipLaunchKernelGGL((k_genvar<KK, true>), grid, dim3(256), lds, st, q.tiles, q.items, q.segs, A, q.N, q.L, q.nwin, ab);          \
        } else {                                                                                                                          \
            hipLaunchKernelGGL((k_genvar<KK, false>), grid, dim3(256), lds, st, q.tiles, q.items, q.segs, A, q.N, q.L, q.nwin, ab);         \
        }                                                                                                                                 \
        break;
    switch (n) {
        NGP_GV_CASE(1) NGP_GV_CASE(2) NGP_GV_CASE(3) NGP_GV_CASE(4) NGP_GV_CASE(5) NGP_GV_CASE(6) NGP_GV_CASE(7) NGP_GV_CASE(8)
        default: return hipErrorInvalidValue;
    }
#undef NGP_GV_CASE
    hipLaunchKernelGGL(k_genvar_rows, dim3((unsigned)q.nblk_r, (unsigned)n), dim3(256), 0, st, A, q.set_item0, q.nsets, q.nwin, q.N, q.L, ab);
    hipLaunchKernelGGL(k_genvar_var, dim3((unsigned)((q.nslots + 255) / 256), (unsigned)n), dim3(256), 0, st, A, q.nwin, q.nsets, q.ncol_w, q.nblk_r, q.N,
                       (const unsigned *)ab);
    for (int i = 0; i < n; i++) {  // (threshold and trace capacity may differ between the chains of a pass)
        GvArgs one;
        std::memset(&one, 0, sizeof one);
        one.c[0] = A.c[i];
        hipLaunchKernelGGL(k_genvar_acc, dim3((unsigned)((q.nslots + 255) / 256), 1u), dim3(256), 0, st, one, q.nslots, q.thr[i], q.trace_rows[i],
                           (const unsigned *)ab);
    }
    return hipGetLastError();
}

}  // namespace ngp
