// ngp_sweep_inst.hip -- one instantiation of the persistent sweep kernel (ngp_sweep.h) and the lookup of its host addresses.
// Compiled six times: -DNGP_INST_DBG=0 (lean production kernel, K chains per pass), =1 (diagnostic kernel: time stamps, timing modes;
// tall fp32 panels), =2 (full production kernel: Tuple sets, tall shards), =3 (models with a BayesR set), =4 (models with a BayesRCpi set: one chain, tall fp32 panels, K chains per pass),
// =5 (the lean kernel with the row-owning streamer's direct quads).
#include <hip/hip_runtime.h>

#include "ngp_sweep.h"

#ifndef NGP_INST_DBG
#error "compile with -DNGP_INST_DBG=0, 1, 2, 3, 4 or 5"
#endif

#define NGP_CAT_(a, b) a##b
#define NGP_CAT(a, b) NGP_CAT_(a, b)

namespace ngp {

// sweep_kernel_0 .. sweep_kernel_5 (ngp_sweep_args.h): the kernels this translation unit defines
const void *NGP_CAT(sweep_kernel_, NGP_INST_DBG)(SweepKernel k) {
    switch (k) {
#if NGP_INST_DBG == 0
    case SweepKernel::lean: return (const void *)k_sweep<false>;
    case SweepKernel::multi: return (const void *)k_sweep_multi;
#elif NGP_INST_DBG == 1
    case SweepKernel::diag: return (const void *)k_sweep<true>;
    case SweepKernel::tall: return (const void *)k_sweep_tall;
#elif NGP_INST_DBG == 2
    case SweepKernel::tup: return (const void *)k_sweep_tup;
    case SweepKernel::multi_tup: return (const void *)k_sweep_multi_tup;
#elif NGP_INST_DBG == 3
    case SweepKernel::r: return (const void *)k_sweep_r;
    case SweepKernel::multi_r: return (const void *)k_sweep_multi_r;
#elif NGP_INST_DBG == 4
    case SweepKernel::rc: return (const void *)k_sweep_rc;
    case SweepKernel::tall_rc: return (const void *)k_sweep_tall_rc;
    case SweepKernel::multi_rc: return (const void *)k_sweep_multi_rc;
#elif NGP_INST_DBG == 5
    case SweepKernel::lean_dq: return (const void *)k_sweep_dq;
#endif
    default: return nullptr;
    }
}

}  // namespace ngp
