// ngp_grm_stats.h -- the column statistics of the genomic relationship matrix (src/misc.jl:149-156), in ONE place: k_grm_cols
// (ngp_dense.h) centres and scales with them, the SNP back-solve (ngp_backsolve.h) weights its columns with them.  Both see the same
// mean, p and 2 p q of a column because both run this text.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace ngp {

// One wave per column (all 64 lanes call it): lane j adds rows j, j + 64, ... in fp64 from 0.0, the butterfly combines the lane sums;
// mean = sum / N, p = mean / 2, tp = (2 p) (1 - p).  nf: this lane saw a non-finite genotype.
template <typename TIn>
__device__ __forceinline__ void grm_col_stats(const TIn *__restrict__ col, long long N, int lane, double &mean, double &tp, bool &nf) {
    double acc = 0.0;
    nf = false;
    for (long long i = lane; i < N; i += 64) {
        const double x = (double)col[i];
        nf = nf || !isfinite(x);
        acc = acc + x;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off);
    mean = acc / (double)N;
    const double p = mean / 2.0;
    tp = (2.0 * p) * (1.0 - p);
}

}  // namespace ngp
