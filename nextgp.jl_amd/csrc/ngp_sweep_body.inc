// ngp_sweep_body.inc -- body of the persistent sweep kernel, included into every instantiation (k_sweep<DBG>, k_sweep_tup) with the
// compile-time flags DBG, TUP and RCLSV (role_sampler) and DQV (role_streamer_rows: direct quads) in scope.  Text inclusion, not a common function: every kernel then reads its launch arguments as
// its own by-value parameter A (scalar loads from the kernarg segment), exactly as k_sweep always did -- handed on by reference to
// a shared function, the register allocation of the row-owning streamer moved and 50k x 600k lost 1.7 %.
    extern __shared__ __attribute__((aligned(16))) char smem[];
    NGP_DBG_LOCALS
    const int b = blockIdx.x;
    // an earlier launch of this call gave up: nothing runs until the host has looked (the chain stays where that launch found it)
    if (ld_u32(A.abort_w) != 0u) return;
    if (!sweep_census(A, b, smem)) return;
    if (dbg_mode == 1 && b <= A.NG) return;
    if ((dbg_mode == 2 && b != 0) || ((dbg_mode == 3 || dbg_mode == 4) && b == 0)) return;
    if (b == 0)
        role_sampler<DBG, false, TUP, RCLSV>(A, smem);
    else if (b <= A.NG) {
        if (b == A.NG && (A.knob & NGP_KNOB_WARMER)) role_warmer<DBG>(A, smem);  // (that reducer would return at once: no far lag is its)
        else role_reducer<DBG>(A, b - 1, smem);
    } else {
        const int s = b - 1 - A.NG;
        if (A.variant == 2) {  // row-owning waves + loader wave (host: R <= NGP_ROWS_MAX_R, lag 3..6)
            switch (A.D) {
                case 3: role_streamer_rows<DBG, 3, 0, DQV>(A, s, smem); break;
                case 4: role_streamer_rows<DBG, 4, 0, DQV>(A, s, smem); break;
                case 5: role_streamer_rows<DBG, 5, 0, DQV>(A, s, smem); break;
                default: role_streamer_rows<DBG, 6, 0, DQV>(A, s, smem); break;  // (lag 7 was built: 58 VGPRs of the delay line spill, 2.58 -> 3.08 us per block)
            }
            return;
        }
        if (A.variant == 3) {  // compact storage: the same roles over byte tiles (host: R a multiple of 16, lag from the lists below)
            const int nt = ngp_u8_tasks(A.R);
            if (nt == 1) {
                switch (A.D) {
                    case 3: role_streamer_rows<DBG, 3, 1>(A, s, smem); break;
                    case 4: role_streamer_rows<DBG, 4, 1>(A, s, smem); break;
                    case 6: role_streamer_rows<DBG, 6, 1>(A, s, smem); break;
                    case 8: role_streamer_rows<DBG, 8, 1>(A, s, smem); break;
                    default: role_streamer_rows<DBG, 12, 1>(A, s, smem); break;
                }
            } else if (nt == 2) {
                if (A.D == 4) role_streamer_rows<DBG, 4, 2>(A, s, smem);
                else role_streamer_rows<DBG, 8, 2>(A, s, smem);
            } else {
                role_streamer_rows<DBG, 4, 4>(A, s, smem);  // (192 VGPRs of delay line at lag 6 spill)
            }
            return;
        }
        const int tpt = (8 * A.R + NGP_WG - 1) / NGP_WG;  // 1..4
#define NGP_DISPATCH_D(T)                                      \
    switch (A.D) {                                             \
        case 1: role_streamer<DBG, 1, T>(A, s, smem); break;        \
        case 2: role_streamer<DBG, 2, T>(A, s, smem); break;        \
        case 3: role_streamer<DBG, 3, T>(A, s, smem); break;        \
        default: role_streamer<DBG, 4, T>(A, s, smem); break;       \
    }
#define NGP_DISPATCH_D8(T)                                     \
    switch (A.D) {                                             \
        case 5: role_streamer<DBG, 5, T>(A, s, smem); break;        \
        case 6: role_streamer<DBG, 6, T>(A, s, smem); break;        \
        case 7: role_streamer<DBG, 7, T>(A, s, smem); break;        \
        case 8: role_streamer<DBG, 8, T>(A, s, smem); break;        \
        default: NGP_DISPATCH_D(T)                             \
    }
        if (tpt == 1) {
            NGP_DISPATCH_D8(1)
        } else if (tpt == 2) {
            NGP_DISPATCH_D8(2)
        } else {
            switch (A.D) {  // host clamps the lag to 5 for tall shards (register budget of the delay line: 32 VGPRs per lag)
                case 5: role_streamer<DBG, 5, 4>(A, s, smem); break;
                default: NGP_DISPATCH_D(4)
            }
        }
#undef NGP_DISPATCH_D8
#undef NGP_DISPATCH_D
    }
