// ngp_bed.h -- PLINK .bed columns on the device ("PLINK .bed panels"): a staged chunk of packed SNP-major
// columns is decoded straight into the sweep's tiles, for both storages, with the records' rows gathered, the genotypes counted and
// the missing calls filled in.  No host matrix of the panel is formed and a quarter of the bytes of ngp_panel_columns_u8 cross PCIe.
//
// Input: nc columns, `stride` bytes apart (stride >= ceil(n_file / 4)).  Sample i of the file sits in bits 2 (i mod 4) .. 2 (i mod 4) + 1
// of byte i / 4.  Two-bit values: 0 = two copies of A1, 1 = missing, 2 = heterozygous, 3 = no copy of A1; the stored value is the count
// of A1 {0 -> 2, 2 -> 1, 3 -> 0}, or of A2 (allele == 2: 0 and 2 swap).  rows[N] (optional) picks the file's samples of the N panel rows,
// any order, repeats allowed; without it row i is sample i.  Only samples < n_file are ever addressed (the host checks rows[] before any
// launch), so the pad bits of a column's last byte and the bytes between ceil(n_file / 4) and stride are never read as genotypes.
//
// k_bed_stats (one workgroup per column) counts c0, c1, c2, cmiss over the N selected rows in integers -- order-independent -- and
// derives from them what the fill kernels need per column: the stored mean m and the value v_miss a missing call takes.
//   training panel:    MEAN   v_miss = mu_obs = sum / n_obs              m = centre ? mu_obs : 0
//                      ROUND  v_miss = g_round = (2 sum + n_obs) / (2 n_obs)   (integer division: the nearest code, ties up)
//                                                                         m = centre ? (sum + cmiss g_round) / N : 0
//                             (what k_u8_colmean gives on the imputed codes: an integer sum over N)
//   prediction panel:  MEAN   v_miss = training mean                      m = centre ? training mean : 0   (the host refuses centre == 0)
//                      ROUND  v_miss = floor(training mean + 0.5) in 0..2
//   with sum = c1 + 2 c2, n_obs = c0 + c1 + c2 and mu_obs = g_round = 0 for a column without an observed call.
// k_bed_fill / k_bed_fill8 have the thread shapes and the stores of k_cols_fill / k_cols_fill8 (ngp_kernels.h) and form
// x = (float)((double)v - m), or (float)(rs_i ((double)v - m)), exactly as those do: on a column without missing calls the tiles are bit
// for bit the tiles of ngp_panel_columns_u8 on the decoded codes.  Under MEAN with centring a missing call is (float)(m - m) = 0.0f.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "ngp_common.h"

namespace ngp {

#define NGP_BED_LUT_A1 0x1Eu  // count of A1 by two-bit value, two bits each: 0 -> 2, 1 -> 3 (missing), 2 -> 1, 3 -> 0
#define NGP_BED_LUT_A2 0x9Cu  // count of A2: 0 -> 0, 1 -> 3 (missing), 2 -> 1, 3 -> 2

// allele count (0, 1, 2) or 3 (missing) of sample idx of one packed column
__device__ __forceinline__ unsigned bed_call(const uint8_t *__restrict__ col, long long idx, unsigned lut) {
    const unsigned code = ((unsigned)col[idx >> 2] >> (2u * (unsigned)(idx & 3))) & 3u;
    return (lut >> (2u * code)) & 3u;
}

// cnt[c][4] = c0, c1, c2, cmiss; mean_out[c] = m; vmiss[c] = v_miss (header).  train_mean: null for a training panel, else the
// training means of these columns.  policy: NGP_BED_MISSING_* (under ERROR the host looks at cmiss and v_miss is never used).
__global__ __launch_bounds__(256) void k_bed_stats(const uint8_t *__restrict__ packed, long long stride, const long long *__restrict__ rows,
                                                   long long N, unsigned lut, int policy, int centre, const double *__restrict__ train_mean,
                                                   long long *__restrict__ cnt, double *__restrict__ mean_out, double *__restrict__ vmiss) {
    __shared__ unsigned long long tot[4];
    const long long c = blockIdx.x;  // column of the chunk
    const uint8_t *col = packed + (size_t)c * stride;
    if (threadIdx.x < 4) tot[threadIdx.x] = 0ull;
    __syncthreads();
    unsigned long long k[4] = {0ull, 0ull, 0ull, 0ull};
    if (rows) {
        for (long long i = threadIdx.x; i < N; i += 256) {
            const unsigned g = bed_call(col, rows[i], lut);
#pragma unroll
            for (int v = 0; v < 4; v++) k[v] += (g == (unsigned)v);
        }
    } else {  // one byte, four samples
        for (long long b = threadIdx.x; 4 * b < N; b += 256) {
            const unsigned byte = col[b];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const unsigned g = (4 * b + r < N) ? ((lut >> (2u * ((byte >> (2 * r)) & 3u))) & 3u) : 4u;
#pragma unroll
                for (int v = 0; v < 4; v++) k[v] += (g == (unsigned)v);
            }
        }
    }
#pragma unroll
    for (int v = 0; v < 4; v++) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) k[v] += __shfl_xor(k[v], off);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int v = 0; v < 4; v++) atomicAdd(&tot[v], k[v]);
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    const long long c0 = (long long)tot[0], c1 = (long long)tot[1], c2 = (long long)tot[2], cm = (long long)tot[3];
    cnt[4 * c + 0] = c0; cnt[4 * c + 1] = c1; cnt[4 * c + 2] = c2; cnt[4 * c + 3] = cm;
    const long long sum = c1 + 2 * c2, nobs = c0 + c1 + c2;
    double m, vm;
    if (train_mean) {
        const double tm = train_mean[c];
        m = centre ? tm : 0.0;
        if (policy == NGP_BED_MISSING_MEAN) vm = tm;
        else {
            const double f = floor(tm + 0.5);
            vm = f < 0.0 ? 0.0 : (f > 2.0 ? 2.0 : f);
        }
    } else if (policy == NGP_BED_MISSING_MEAN) {
        vm = nobs ? (double)sum / (double)nobs : 0.0;
        m = centre ? vm : 0.0;
    } else {
        const long long gr = nobs ? (2 * sum + nobs) / (2 * nobs) : 0;
        vm = (double)gr;
        m = centre ? (double)(sum + cm * gr) / (double)N : 0.0;
    }
    mean_out[c] = m;
    vmiss[c] = vm;
}

// thread = (column c of the chunk, quad Q of the padded panel), as k_cols_fill: one float4 at tile_off.  Without a row map one byte
// holds the quad's four genotypes.
__global__ __launch_bounds__(256) void k_bed_fill(float *__restrict__ tiles, const uint8_t *__restrict__ packed, long long stride,
                                                  const long long *__restrict__ rows, long long N, unsigned lut, long long col0, int R, int S,
                                                  const double *__restrict__ mu, const double *__restrict__ vmiss, const double *__restrict__ rs) {
    const long long Q = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long i0 = 4 * Q;
    if (i0 >= (long long)R * S) return;
    const long long c = blockIdx.y, j = col0 + c;
    const int s = (int)(i0 / R), ii = (int)(i0 - (long long)s * R), jj = (int)(j & (NGP_BLK - 1));
    const uint8_t *col = packed + (size_t)c * stride;
    const double m = mu[c], vm = vmiss[c];
    const unsigned byte = (!rows && i0 < N) ? col[Q] : 0u;
    float v[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        float x = 0.0f;
        if (i0 + r < N) {
            const unsigned g = rows ? bed_call(col, rows[i0 + r], lut) : ((lut >> (2u * ((byte >> (2 * r)) & 3u))) & 3u);
            const double vd = (g == 3u) ? vm : (double)g;
            x = rs ? (float)(rs[i0 + r] * (vd - m)) : (float)(vd - m);
        }
        v[r] = x;
    }
    float *tp = tiles + ((size_t)(j >> 6) * S + s) * ((size_t)R * NGP_BLK) + tile_off(ii, jj);
    *(float4 *)tp = make_float4(v[0], v[1], v[2], v[3]);
}

// compact storage, as k_cols_fill8: thread = (column c of the chunk, unit U of 16 rows) -> the unit's 16 bytes at tile8_off.  A
// missing call stores the column's rounded code (vmiss holds an integer 0..2: ROUND is the only policy byte tiles take).
__global__ __launch_bounds__(256) void k_bed_fill8(uint8_t *__restrict__ tiles8, const uint8_t *__restrict__ packed, long long stride,
                                                   const long long *__restrict__ rows, long long N, unsigned lut, long long col0, int R, int S,
                                                   const double *__restrict__ vmiss) {
    const long long U = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long i0 = 16 * U;
    if (i0 >= (long long)R * S) return;
    const long long c = blockIdx.y, j = col0 + c;
    const int s = (int)(i0 / R), ii = (int)(i0 - (long long)s * R), jj = (int)(j & (NGP_BLK - 1));
    const uint8_t *col = packed + (size_t)c * stride;
    const unsigned gm = (unsigned)vmiss[c];
    unsigned w[4];
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const long long iq = i0 + 4 * q;
        const unsigned byte = (!rows && iq < N) ? col[iq >> 2] : 0u;
        unsigned v = 0;
#pragma unroll
        for (int r = 0; r < 4; r++) {
            if (iq + r < N) {
                const unsigned g = rows ? bed_call(col, rows[iq + r], lut) : ((lut >> (2u * ((byte >> (2 * r)) & 3u))) & 3u);
                v |= ((g == 3u) ? gm : g) << (8 * r);
            }
        }
        w[q] = v;
    }
    uint8_t *tp = tiles8 + ((size_t)(j >> 6) * S + s) * ((size_t)R * NGP_BLK) + tile8_off(ii, jj);
    *(uint4 *)tp = make_uint4(w[0], w[1], w[2], w[3]);
}

}  // namespace ngp
