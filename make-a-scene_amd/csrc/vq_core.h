// The nearest-codebook assignment shared by the vector quantiser's lookup (vq.hip) and the k-means re-initialisation (kmeans.hip):
// row norms, the split partial (min, argmin) per latent row, and the split count.  ONE copy, so both callers take the same index on the
// same numbers (a per-kernel copy of the distance loop is free to be contracted differently by the compiler).
//
// Numerics: fp32 throughout.  dot(z,e) is an exact-fp32 FMA chain (v_mfma_f32_32x32x2_f32), and
// d = fl(fl(|z|^2 + |e|^2) - 2*dot) follows the reference's evaluation order, so indices are
// bit-exact wherever the reference's own top-2 gap exceeds fp32 summation-order noise.
// Ties resolve to the lowest index like torch.argmin.
//
// `skip` (nullable): the k-means fit's device int32 pair {iterations run, converged}.  A kernel given one returns before its first
// load once `converged` is set (uniform across the work-group: nobody stores the pair during these launches); the lookup passes null.
#pragma once
#include "mas_common.h"
#include <math.h>

namespace {

constexpr int NT = 256, ROWS_PER_BLOCK = 128, CODES_PER_TILE = 32, MAX_KSPLIT = 64;

__global__ __launch_bounds__(NT) void row_sqnorm(const float* __restrict__ x, int rows, int D, float* __restrict__ out,
                                                 const int32_t* __restrict__ skip) {
    if (skip && skip[1]) return;
    const int wave = (blockIdx.x * NT + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (wave >= rows) return;
    float s = 0.0f;
    for (int d = lane; d < D; d += 64) { const float v = x[(size_t)wave * D + d]; s += v * v; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) out[wave] = s;
}

struct MinIdx { float v; int i; };
__device__ __forceinline__ void take_min(float& bv, int& bi, float v, int i) {
    if (v < bv || (v == bv && i < bi)) { bv = v; bi = i; }
}

template <int D>
__global__ __launch_bounds__(NT) void vq_partial(const float* __restrict__ z, const float* __restrict__ cb,
                                                 const float* __restrict__ zz, const float* __restrict__ ee, int M, int K,
                                                 int ksplit, float* __restrict__ pval, int* __restrict__ pidx,
                                                 const int32_t* __restrict__ skip) {
    constexpr int HD = D / 2;                  // dims handled by one lane group
    constexpr int LSTR = D + 4;                // LDS row stride (floats): +16 B breaks b128 bank conflicts
    __shared__ __attribute__((aligned(16))) float tile[CODES_PER_TILE * LSTR];
    if (skip && skip[1]) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int g = lane >> 5, l31 = lane & 31;
    const int rb = blockIdx.x / ksplit, sp = blockIdx.x % ksplit;
    const int row = rb * ROWS_PER_BLOCK + wave * 32 + l31;
    const bool row_ok = row < M;

    // B operand: this lane's half of its latent row, resident in registers for the whole kernel
    float zf[HD];
    {
        const float* zp = z + (size_t)(row_ok ? row : 0) * D + g * HD;
#pragma unroll
        for (int q = 0; q < HD / 4; ++q) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(zp + 4 * q);
            zf[4 * q] = row_ok ? v[0] : 0.0f; zf[4 * q + 1] = row_ok ? v[1] : 0.0f;
            zf[4 * q + 2] = row_ok ? v[2] : 0.0f; zf[4 * q + 3] = row_ok ? v[3] : 0.0f;
        }
    }
    const float zzr = row_ok ? zz[row] : 0.0f;

    const int ntiles = (K + CODES_PER_TILE - 1) / CODES_PER_TILE;
    const int tiles_per = (ntiles + ksplit - 1) / ksplit;
    const int t0 = sp * tiles_per, t1 = min(ntiles, t0 + tiles_per);

    float best = INFINITY; int besti = 0x7fffffff;
    for (int t = t0; t < t1; ++t) {
        const int k0 = t * CODES_PER_TILE;
        __syncthreads();
        // stage 32 code vectors (coalesced float4 loads)
        for (int u = tid; u < CODES_PER_TILE * (D / 4); u += NT) {
            const int c = u / (D / 4), q = u % (D / 4);
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (k0 + c < K) v = *reinterpret_cast<const f32x4*>(cb + (size_t)(k0 + c) * D + 4 * q);
            *reinterpret_cast<f32x4*>(&tile[c * LSTR + 4 * q]) = v;
        }
        __syncthreads();
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
        const float* ap = &tile[l31 * LSTR + g * HD];
#pragma unroll
        for (int q = 0; q < HD / 4; ++q) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(ap + 4 * q);
#pragma unroll
            for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], zf[4 * q + j], acc, 0, 0, 0);
        }
        // acc[r] = dot(code k0+acc_row(lane,r), latent row l31)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = k0 + acc_row(lane, r);
            if (k < K) {
                const float d = (zzr + ee[k]) - 2.0f * acc[r];
                if (d < best) { best = d; besti = k; }      // ascending k within a lane: strict < keeps the first
            }
        }
    }
    // merge the two lane groups that share a latent row
    const float ov = __shfl_xor(best, 32); const int oi = __shfl_xor(besti, 32);
    take_min(best, besti, ov, oi);
    if (g == 0 && row_ok) { pval[(size_t)row * ksplit + sp] = best; pidx[(size_t)row * ksplit + sp] = besti; }
}

inline int pick_ksplit(int M, int K) {
    const int rb = mas_cdiv(M, ROWS_PER_BLOCK), ntiles = mas_cdiv(K, CODES_PER_TILE);
    int ks = mas_cdiv(1024, rb);
    if (ks > MAX_KSPLIT) ks = MAX_KSPLIT;
    if (ks > ntiles) ks = ntiles;
    return ks < 1 ? 1 : ks;
}

// the D dispatch of vq_partial: false when D is not one of the four instantiations (nothing launched)
inline bool launch_vq_partial(int D, dim3 grid, hipStream_t s, const float* z, const float* cb, const float* zz, const float* ee, int M,
                              int K, int ksplit, float* pval, int* pidx, const int32_t* skip) {
    switch (D) {
        case 32: hipLaunchKernelGGL(vq_partial<32>, grid, dim3(NT), 0, s, z, cb, zz, ee, M, K, ksplit, pval, pidx, skip); return true;
        case 64: hipLaunchKernelGGL(vq_partial<64>, grid, dim3(NT), 0, s, z, cb, zz, ee, M, K, ksplit, pval, pidx, skip); return true;
        case 128: hipLaunchKernelGGL(vq_partial<128>, grid, dim3(NT), 0, s, z, cb, zz, ee, M, K, ksplit, pval, pidx, skip); return true;
        case 256: hipLaunchKernelGGL(vq_partial<256>, grid, dim3(NT), 0, s, z, cb, zz, ee, M, K, ksplit, pval, pidx, skip); return true;
        default: return false;
    }
}

}  // namespace
