// ngp_sweep_multi_body.inc -- body of the fused kernel of K chains per pass, included into its instantiations with the compile-time
// flags TUPM / RCLSM in scope: k_sweep_multi (models without a Tuple set: the sampler of k_sweep<false> plus the BayesR chain),
// k_sweep_multi_tup (models with a Tuple set), k_sweep_multi_r (models with a BayesR set: the sampler of k_sweep_r) and k_sweep_multi_rc
// (any chain with a BayesRCpi set: the sampler of k_sweep_rc).  Text inclusion for the reason given in ngp_sweep_body.inc.
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int b = blockIdx.x, K = M.K, NG = M.a[0].NG;
    if (ld_u32(M.a[0].abort_w) != 0u) return;
    if (!sweep_census(M.a[0], b, smem)) return;
#ifndef NGP_MULTI_STRIDE
#define NGP_MULTI_STRIDE 8  // samplers at blocks 0, 8, 16, ...: one XCD under round-robin placement
#endif
    if ((b % NGP_MULTI_STRIDE) == 0 && (b / NGP_MULTI_STRIDE) < K) {
        role_sampler<false, false, TUPM, RCLSM>(multi_chain_args(__builtin_amdgcn_readfirstlane(b / NGP_MULTI_STRIDE)), smem);
        return;
    }
    const int idx = b - min(K, (b + NGP_MULTI_STRIDE - 1) / NGP_MULTI_STRIDE);  // rank among the blocks that are not samplers
    const int NR = ngp_multi_reducers(K, NG, M.pair);
    if (idx < NR) {
        if (M.pair) {  // workgroup (p, g): chain 2 p in waves 0-3, chain 2 p + 1 in waves 4-7 (an unpaired last chain keeps all eight)
            const int pr = idx / NG, wq = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 8));
            if (2 * pr + 1 >= K) role_reducer<false>(multi_chain_args(__builtin_amdgcn_readfirstlane(2 * pr)), idx % NG, smem);
            else role_reducer<false>(multi_chain_args(__builtin_amdgcn_readfirstlane(2 * pr + wq)), idx % NG, smem, 4 * wq, 4);
        } else {
            role_reducer<false>(multi_chain_args(__builtin_amdgcn_readfirstlane(idx / NG)), idx % NG, smem);
        }
        return;
    }
    const int s = idx - NR;
    // host: lag 6 or 8 (shards of at most 64 rows, fp32 tiles), 2..8 chains
#ifdef NGP_MULTI_ONLY  /* resource-usage experiments: one instantiation (hipcc -DNGP_MULTI_ONLY=8 -Rpass-analysis=kernel-resource-usage) */
    role_streamer_multi<8, NGP_MULTI_ONLY>(M, s, smem);
    return;
#endif
#define NGP_MULTI_K(DTV)                                              \
    switch (K) {                                                      \
        case 2: role_streamer_multi<DTV, 2>(M, s, smem); break;       \
        case 3: role_streamer_multi<DTV, 3>(M, s, smem); break;       \
        case 4: role_streamer_multi<DTV, 4>(M, s, smem); break;       \
        case 5: role_streamer_multi<DTV, 5>(M, s, smem); break;       \
        case 6: role_streamer_multi<DTV, 6>(M, s, smem); break;       \
        case 7: role_streamer_multi<DTV, 7>(M, s, smem); break;       \
        default: role_streamer_multi<DTV, 8>(M, s, smem); break;      \
    }
    if (M.a[0].variant == 2) {  // row-owning streamer, lag 4 or 6 (host: fp32 tiles, shards of 64..NGP_ROWS_MAX_R rows), 2 chains
#ifdef NGP_ROWS_MULTI_ONLY  /* resource-usage experiments: one instantiation */
        role_streamer_rows_multi<NGP_ROWS_MULTI_ONLY, 2>(M, s, smem);
#else
        if (M.a[0].D == 4) role_streamer_rows_multi<4, 2>(M, s, smem);
        else if (M.a[0].D == 5) role_streamer_rows_multi<5, 2>(M, s, smem);
        else role_streamer_rows_multi<6, 2>(M, s, smem);
#endif
        return;
    }
    if (M.a[0].variant == 3) {  // compact storage: the lags of the one-chain byte streamer; 2 or 3 chains (four update tasks per lane: 2) -- host: fusable()
        // (four chains were built and measured: their registers spill, 50k x 600k 77 it/s with three chains, 70 with four)
        const int nt = ngp_u8_tasks(M.a[0].R);
#define NGP_BYTES_K(DTV, STV)                                             \
    if (K == 2) role_streamer_rows_multi<DTV, 2, STV>(M, s, smem);        \
    else role_streamer_rows_multi<DTV, 3, STV>(M, s, smem);
        if (nt == 1) {
            if (M.a[0].D == 4) { NGP_BYTES_K(4, 1) }
            else if (M.a[0].D == 6) { NGP_BYTES_K(6, 1) }
            else { NGP_BYTES_K(8, 1) }
        } else if (nt == 2) {
            if (M.a[0].D == 4) { NGP_BYTES_K(4, 2) }
            else { NGP_BYTES_K(8, 2) }
        } else {
            role_streamer_rows_multi<4, 2, 4>(M, s, smem);
        }
#undef NGP_BYTES_K
        return;
    }
    if (M.a[0].D == 6) { NGP_MULTI_K(6) } else { NGP_MULTI_K(8) }
#undef NGP_MULTI_K
