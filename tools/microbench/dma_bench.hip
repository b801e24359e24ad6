// dma_bench.hip -- how should one CU stream its share of the panel?  (diagnostic, not product)
// 246 workgroups x 512 threads, one per CU; workgroup s streams tiles (t, s), t = 0..nb-1, each NQ KiB contiguous,
// into an LDS ring with global_load_lds_dwordx4; nothing is computed.  Variants:
//   0 burst:       per block: issuers wait vmcnt(0), request the whole next tile (split over NI issuer waves), barrier
//   1 continuous:  per block: each issuer requests its share of [tile u+1 quads H.., tile u+2 quads 0..H), waits until at
//                  most its share of H is outstanding, barrier
//   2 free:        issuers never meet a barrier: each keeps at most W requests outstanding (pure bandwidth ceiling)
//   3 lean:        variant 1 with the loader's lean issue sequence (scalar base and LDS address)
//   4 direct:      the row-owning streamer's shape; KD quads per row wave bypass the DMA queue (see direct_quads below)
// build: hipcc --offload-arch=gfx950 -O3 -o dma_bench dma_bench.hip ; run: ./dma_bench variant NI H_or_W [NQ] [nb]
//   variant 4: ./dma_bench 4 KD H [NQ] [nb] [late] [nsleep]; KD = -1 prints the whole table (late 0, 1 x KD 0, 1, 2, three rounds)
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#define QS 1040
__device__ inline void dma16(const void *g, const void *l) {
    const unsigned m = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(__attribute__((address_space(3))) const char *)l);
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, off\n\ts_mov_b32 m0, %0" : "=&s"(keep) : "s"(m), "v"(g) : "memory");
}
// lean form: LDS address and 64-bit global base in SGPRs (wave-uniform), per-lane 32-bit offset in one VGPR
__device__ inline void dma16_s(unsigned lds_addr, const void *gbase, unsigned voff) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %2, %3\n\ts_mov_b32 m0, %0" : "=&s"(keep) : "s"(lds_addr), "v"(voff), "s"(gbase) : "memory");
}
__device__ inline void bar() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
__device__ inline void wait_le(int n) {
#define C(i) case i: asm volatile("s_waitcnt vmcnt(" #i ")" ::: "memory"); break;
    switch (n) { C(1) C(2) C(3) C(4) C(5) C(6) C(7) C(8) C(9) C(10) C(11) C(12) C(13) C(14) C(15) C(16) C(17) C(18) C(19) C(20) C(21) C(22) C(23) C(24)
                 C(25) C(26) C(27) C(28) C(29) C(30) C(31) C(32) C(40) C(48) C(56) C(63) default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
#undef C
}
// four requests for four consecutive quads into four consecutive ring slots (the sweep's loader: one scalar base, the
// immediate offset walks the source and is added to the LDS address too, so M0 advances by QS - 1024)
__device__ inline void dma16_s4(unsigned lds_addr, const void *gbase, unsigned voff) {
    unsigned keep;
    const unsigned m1 = lds_addr + (QS - 1024), m2 = lds_addr + 2 * (QS - 1024), m3 = lds_addr + 3 * (QS - 1024);
    asm volatile(
        "s_mov_b32 %0, m0\n\t"
        "s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %5, %6\n\t"
        "s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %5, %6 offset:1024\n\t"
        "s_mov_b32 m0, %3\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %5, %6 offset:2048\n\t"
        "s_mov_b32 m0, %4\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %5, %6 offset:3072\n\t"
        "s_mov_b32 m0, %0"
        : "=&s"(keep)
        : "s"(lds_addr), "s"(m1), "s"(m2), "s"(m3), "v"(voff), "s"(gbase)
        : "memory");
}
// Variant 4, direct quads: the row-owning streamer's shape (7 row waves + 1 loader wave, ring of 2 NQ + H slots, one barrier
// per tile).  The loader requests quads [0, NQ - 7 KD) by LDS-DMA in the sweep's own sequence (tile u+1 quads H.., tile u+2
// quads 0..H, counted wait, barrier).  Row wave w fetches the KD quads it owns among the last 7 KD (q mod 7 == w) of tile u+1
// with a plain 16-byte-per-lane load into registers during block u -- right behind the barrier (late = 0) or after nsleep x
// s_sleep 4 (late = 1, a stand-in for the row work) -- and stores them into their ring slots with one ds_write_b128 each at
// the start of block u+1.  Every row wave then reads one word of each quad it owns (the GEMV's view), so the sums check
// that both paths delivered.  KD = 0 is the loader alone, with the row waves sleeping and reading the same way.
template <int KD>
__device__ inline unsigned long long direct_quads(const char *tiles, char *smem, int nb, int S, int NQ, int H, int late, int nsleep, int s, int wv, int lane) {
    const int RQ = 2 * NQ + H, NQD = NQ - 7 * KD;
    const size_t tile_bytes = (size_t)NQ * 1024;
    auto wrap = [&](int p) { return p >= RQ ? p - RQ : p; };
    unsigned long long acc = 0;
    int base = 0;
    if (wv == 7) {
        const unsigned ring0 = (unsigned)(size_t)(__attribute__((address_space(3))) const char *)smem;
        const unsigned voff = lane * 16;
        auto dma_quads = [&](int tile, int q0, int q1, int tbase) {
            if (q0 >= q1) return 0;
            const char *g = tiles + ((size_t)tile * S + s) * tile_bytes + (size_t)q0 * 1024;
            int p = wrap(tbase + q0), q = q0;
            for (; q + 4 <= q1; q += 4) {
                if (p + 4 <= RQ) {
                    dma16_s4(ring0 + (unsigned)p * QS, g, voff);
                    p += 4;
                    if (p == RQ) p = 0;
                } else {
                    for (int i = 0; i < 4; i++) {
                        dma16_s(ring0 + (unsigned)p * QS, g + i * 1024, voff);
                        if (++p == RQ) p = 0;
                    }
                }
                g += 4096;
            }
            for (; q < q1; ++q) {
                dma16_s(ring0 + (unsigned)p * QS, g, voff);
                g += 1024;
                if (++p == RQ) p = 0;
            }
            return q1 - q0;
        };
        __builtin_amdgcn_s_setprio(3);
        if (nb > 0) dma_quads(0, 0, NQD, 0);
        if (nb > 1) dma_quads(1, 0, H, NQ);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        bar();
        for (int u = 0; u < nb; ++u) {
            const int base1 = wrap(base + NQ), base2 = wrap(base1 + NQ);
            if (u + 1 < nb) dma_quads(u + 1, H, NQD, base1);
            int n2 = 0;
            if (u + 2 < nb) n2 = dma_quads(u + 2, 0, H, base2);
            wait_le(n2);
            bar();
            acc += *(const unsigned *)(smem + (size_t)base * QS + lane * 16);
            base = base1;
        }
    } else {
        const int qd0 = NQD + ((wv + 7 - NQD % 7) % 7);  // the first direct quad of this wave
        float4 dq0 = make_float4(0.f, 0.f, 0.f, 0.f), dq1 = dq0;  // (named, not an array: an indexed one lands in scratch)
        if (nb > 0) {
            const char *src = tiles + (size_t)s * tile_bytes + (size_t)lane * 16;
            if constexpr (KD > 0) dq0 = *(const float4 *)(src + (size_t)qd0 * 1024);
            if constexpr (KD > 1) dq1 = *(const float4 *)(src + (size_t)(qd0 + 7) * 1024);
        }
        bar();
        for (int u = 0; u < nb; ++u) {
            if constexpr (KD > 0) *(float4 *)(smem + (size_t)wrap(base + qd0) * QS + lane * 16) = dq0;
            if constexpr (KD > 1) *(float4 *)(smem + (size_t)wrap(base + qd0 + 7) * QS + lane * 16) = dq1;
            if (late)
                for (int i = 0; i < nsleep; i++) asm volatile("s_sleep 4" ::: "memory");
            if (u + 1 < nb) {
                const char *src = tiles + ((size_t)(u + 1) * S + s) * tile_bytes + (size_t)lane * 16;
                if constexpr (KD > 0) dq0 = *(const float4 *)(src + (size_t)qd0 * 1024);
                if constexpr (KD > 1) dq1 = *(const float4 *)(src + (size_t)(qd0 + 7) * 1024);
            }
            for (int q = wv; q < NQ; q += 7) acc += *(const unsigned *)(smem + (size_t)wrap(base + q) * QS + lane * 16);
            bar();
            base = wrap(base + NQ);
        }
    }
    return acc;
}
__global__ __launch_bounds__(512) void k(const char *tiles, int nb, int S, int NQ, int variant, int NI, int HW, int nbar, unsigned long long *sink, int nsleep) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int s = blockIdx.x, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const size_t tile_bytes = (size_t)NQ * 1024;
    const int myi = wv - (8 - NI);  // issuer index, < 0: not an issuer
    unsigned long long acc = 0;
    if (variant == 0) {
        for (int u = 0; u < nb; ++u) {
            if (myi >= 0) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                if (u + 1 < nb) {
                    const char *src = tiles + ((size_t)(u + 1) * S + s) * tile_bytes + (size_t)lane * 16;
                    char *dst = smem + (size_t)((u + 1) & 1) * NQ * QS;
                    for (int q = myi; q < NQ; q += NI) dma16(src + (size_t)q * 1024, dst + (size_t)q * QS);
                }
            }
            for (int b = 0; b < nbar; b++) bar();
            acc += *(const unsigned *)(smem + (size_t)(u & 1) * NQ * QS + lane * 16);
        }
    } else if (variant == 1) {
        const int H = HW, RQ = 2 * NQ + H;
        int base = 0;
        auto wrap = [&](int p) { return p >= RQ ? p - RQ : p; };
        if (myi >= 0) {
            const char *src0 = tiles + ((size_t)s) * tile_bytes + (size_t)lane * 16;
            for (int q = myi; q < NQ; q += NI) dma16(src0 + (size_t)q * 1024, smem + (size_t)q * QS);
            for (int q = myi; q < H; q += NI) dma16(src0 + (size_t)S * tile_bytes + (size_t)q * 1024, smem + (size_t)(NQ + q) * QS);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        bar();
        for (int u = 0; u < nb; ++u) {
            int n2 = 0;
            if (myi >= 0) {
                const int base1 = wrap(base + NQ), base2 = wrap(base1 + NQ);
                if (u + 1 < nb) {
                    const char *src = tiles + ((size_t)(u + 1) * S + s) * tile_bytes + (size_t)lane * 16;
                    for (int q = H + ((NI + myi - (H % NI)) % NI); q < NQ; q += NI) dma16(src + (size_t)q * 1024, smem + (size_t)wrap(base1 + q) * QS);
                }
                if (u + 2 < nb) {
                    const char *src = tiles + ((size_t)(u + 2) * S + s) * tile_bytes + (size_t)lane * 16;
                    for (int q = myi; q < H; q += NI, ++n2) dma16(src + (size_t)q * 1024, smem + (size_t)wrap(base2 + q) * QS);
                }
                wait_le(n2);
            }
            for (int b = 0; b < nbar; b++) bar();
            acc += *(const unsigned *)(smem + (size_t)base * QS + lane * 16);
            base = wrap(base + NQ);
        }
    } else if (variant == 3) {
        // variant 1 with the lean issue sequence
        const int H = HW, RQ = 2 * NQ + H;
        int base = 0;
        const unsigned ring0 = (unsigned)(size_t)(__attribute__((address_space(3))) const char *)smem;
        const unsigned voff = lane * 16;
        auto wrap = [&](int p) { return p >= RQ ? p - RQ : p; };
        auto issue = [&](const char *tile_src, int q0, int q1, int tbase) {
            int n = 0;
            int q = q0 + ((NI + myi - (q0 % NI)) % NI);
            int p = wrap(tbase + q);
            const char *g = tile_src + (size_t)q * 1024;
            for (; q < q1; q += NI, ++n) {
                dma16_s(__builtin_amdgcn_readfirstlane(ring0 + (unsigned)p * QS), (const void *)__builtin_amdgcn_readfirstlane((unsigned)(size_t)g) ? g : g, voff);
                p += NI; if (p >= RQ) p -= RQ;
                g += (size_t)NI * 1024;
            }
            return n;
        };
        if (myi >= 0) {
            const char *src0 = tiles + ((size_t)s) * tile_bytes;
            issue(src0, 0, NQ, 0);
            issue(src0 + (size_t)S * tile_bytes, 0, H, NQ);
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        bar();
        for (int u = 0; u < nb; ++u) {
            int n2 = 0;
            if (myi >= 0) {
                const int base1 = wrap(base + NQ), base2 = wrap(base1 + NQ);
                if (u + 1 < nb) issue(tiles + ((size_t)(u + 1) * S + s) * tile_bytes, H, NQ, base1);
                if (u + 2 < nb) n2 = issue(tiles + ((size_t)(u + 2) * S + s) * tile_bytes, 0, H, base2);
                wait_le(n2);
            }
            for (int b = 0; b < nbar; b++) bar();
            acc += *(const unsigned *)(smem + (size_t)base * QS + lane * 16);
            base = wrap(base + NQ);
        }
    } else if (variant == 4) {
        // direct quads: NI carries KD, HW carries H, nbar carries `late`
        if (NI == 0) acc = direct_quads<0>(tiles, smem, nb, S, NQ, HW, nbar, nsleep, s, wv, lane);
        else if (NI == 1) acc = direct_quads<1>(tiles, smem, nb, S, NQ, HW, nbar, nsleep, s, wv, lane);
        else acc = direct_quads<2>(tiles, smem, nb, S, NQ, HW, nbar, nsleep, s, wv, lane);
        if (s == 0 && lane == 0) sink[wv] = acc;
    } else {
        // free-running: issuer i streams quads i, i+NI, ... of the whole shard stream, at most HW outstanding
        if (myi >= 0) {
            const long long total = (long long)nb * NQ;
            int ring = 0;
            const int slots = 120 / NI;  // ring slots of this issuer
            for (long long k = myi; k < total; k += NI) {
                const long long t = k / NQ; const int q = (int)(k - t * NQ);
                const char *src = tiles + ((size_t)t * S + s) * tile_bytes + (size_t)q * 1024 + (size_t)lane * 16;
                dma16(src, smem + (size_t)(myi * slots + ring) * QS);
                if (++ring == slots) ring = 0;
                wait_le(HW);
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    if (acc == 0x123456789ull) sink[0] = acc;
}
int main(int argc, char **argv) {
    const int variant = argc > 1 ? atoi(argv[1]) : 0, NI = argc > 2 ? atoi(argv[2]) : 3, HW = argc > 3 ? atoi(argv[3]) : 24;
    const int NQ = argc > 4 ? atoi(argv[4]) : 51, nb = argc > 5 ? atoi(argv[5]) : 4000, nbar = argc > 6 ? atoi(argv[6]) : 1;
    const int nsleep = argc > 7 ? atoi(argv[7]) : 13;  // variant 4, late = 1: 13 x s_sleep 4 = 3328 clocks, about 1.4 us
    const int S = 246;
    const size_t bytes = (size_t)nb * S * NQ * 1024;
    char *d; unsigned long long *sink;
    if (hipMalloc(&d, bytes) != hipSuccess) { printf("alloc failed\n"); return 1; }
    hipMalloc(&sink, 64);
    hipMemset(d, 1, bytes);
    const size_t lds = (size_t)(2 * NQ + 32) * QS + 1024;
    hipFuncSetAttribute((const void *)k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipEvent_t e0, e1; hipEventCreate(&e0); hipEventCreate(&e1);
    if (variant == 4) {
        // KD < 0: the whole table in one process -- three rounds, every round runs late = 0, 1 x KD = 0, 1, 2 in turn (one
        // untimed launch, one timed), so that every KD > 0 run has a KD = 0 run of the same setting next to it
        const int H = HW, kd_lo = NI < 0 ? 0 : NI, kd_hi = NI < 0 ? 2 : NI, late_lo = NI < 0 ? 0 : nbar, late_hi = NI < 0 ? 1 : nbar;
        if (NQ - 7 * kd_hi < H || H > 32 || NQ < 14) { printf("need NQ - 7 KD >= H, H <= 32\n"); return 1; }
        float best[2][3], worst[2][3];
        for (int l = 0; l < 2; l++) for (int kd = 0; kd < 3; kd++) { best[l][kd] = 1e30f; worst[l][kd] = 0.f; }
        printf("direct quads: NQ %d H %d nb %d nsleep %d (late = 1: plain loads after nsleep x s_sleep 4), us per tile\n", NQ, H, nb, nsleep);
        for (int round = 0; round < 3; round++)
            for (int late = late_lo; late <= late_hi; late++)
                for (int kd = kd_lo; kd <= kd_hi; kd++) {
                    float ms = 0.f;
                    for (int rep = 0; rep < 2; rep++) {
                        hipMemset(sink, 0, 64);
                        hipEventRecord(e0);
                        hipLaunchKernelGGL(k, dim3(S), dim3(512), lds, 0, d, nb, S, NQ, 4, kd, H, late, sink, nsleep);
                        hipEventRecord(e1);
                        if (hipEventSynchronize(e1) != hipSuccess) { printf("launch failed: %s\n", hipGetErrorString(hipGetLastError())); return 1; }
                        hipEventElapsedTime(&ms, e0, e1);
                    }
                    unsigned long long got[8];
                    hipMemcpy(got, sink, 64, hipMemcpyDeviceToHost);
                    bool ok = true;  // the panel is all bytes 1: every word read is 0x01010101
                    for (int w = 0; w < 8; w++) ok = ok && got[w] == (unsigned long long)nb * (w == 7 ? 1 : (NQ - w + 6) / 7) * 0x01010101ull;
                    const float us = ms * 1e3f / nb;
                    if (us < best[late][kd]) best[late][kd] = us;
                    if (us > worst[late][kd]) worst[late][kd] = us;
                    printf("round %d late %d KD %d loader requests %2d: %.4f us/tile, %.0f GB/s, data %s\n", round, late, kd, NQ - 7 * kd, us, bytes / ms / 1e6, ok ? "ok" : "WRONG");
                }
        if (NI < 0)
            for (int late = 0; late < 2; late++)
                for (int kd = 1; kd < 3; kd++)
                    printf("late %d KD %d: slowest %.4f against fastest KD 0 %.4f -> %s\n", late, kd, worst[late][kd], best[late][0],
                           worst[late][kd] < best[late][0] ? "faster" : "not faster");
        return 0;
    }
    for (int rep = 0; rep < 3; rep++) {
        hipEventRecord(e0);
        hipLaunchKernelGGL(k, dim3(S), dim3(512), lds, 0, d, nb, S, NQ, variant, NI, HW, nbar, sink, nsleep);
        hipEventRecord(e1); hipEventSynchronize(e1);
        float ms; hipEventElapsedTime(&ms, e0, e1);
        if (rep == 2) printf("variant %d NI %d HW %d NQ %d nbar %d: %.3f ms, %.2f us/block, %.0f GB/s (%.1f%% of 8 TB/s) err=%s\n", variant, NI, HW, NQ, nbar, ms, ms * 1e3 / nb,
                             bytes / ms / 1e6, bytes / ms / 1e6 / 80.0, hipGetErrorString(hipGetLastError()));
    }
    return 0;
}
