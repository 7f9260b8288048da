// The decode-attention body shared by attn_decode_kernel (attn_decode.hip) and attn_decode_dev_kernel (decode_step.hip), and the head_dim
// dispatch of every decode launcher.  The two kernels must agree bit for bit (tests/test_gpu_decode_graph.py); they do because they
// call this ONE function -- a per-kernel copy of the key loop is free to be contracted differently by the compiler.
#pragma once
#include "mas_common.h"
#include <math.h>
#include <type_traits>

constexpr int DECODE_NT = 256;                   // threads of a decode work-group: 4 waves, one key per lane and pass

// One query against keys 0 .. L-1, by the whole 256-thread work-group: a lane owns keys tid, tid + 256, ..., reads each key's contiguous
// HD-element row, keeps an online-softmax partial (m, l, o[HD]) in registers; the 256 partials are merged once at the end (wave
// butterfly, then LDS across the 4 waves: fixed order, deterministic) and wave 0 writes the HD outputs to dst.
// Q, dst: the query / output row of this (batch, head); K, V: key 0 of it, ld_k / ld_v elements between keys.  Rows 16-byte aligned.
template <typename T, int HD>
__device__ __forceinline__ void attn_decode_body(const T* Q, const T* K, const T* V, T* dst,
                                                 int ld_k, int ld_v, int L, float scale) {
    constexpr int EPU = 16 / (int)sizeof(T);
    constexpr int NU = HD / EPU;                 // 16-byte units per row
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    float qf[HD];                                // the query, pre-scaled (transformer.py:56: q / sqrt(hd))
#pragma unroll
    for (int u = 0; u < NU; ++u) {
        const u32x4 raw = *reinterpret_cast<const u32x4*>(Q + u * EPU);
        const T* e = reinterpret_cast<const T*>(&raw);
#pragma unroll
        for (int j = 0; j < EPU; ++j) qf[u * EPU + j] = (float)e[j] * scale;
    }

    float m = -1e30f, l = 0.0f, o[HD];
#pragma unroll
    for (int d = 0; d < HD; ++d) o[d] = 0.0f;

    for (int key = tid; key < L; key += DECODE_NT) {
        const T* kr = K + (size_t)key * ld_k;
        const T* vr = V + (size_t)key * ld_v;
        float s = 0.0f;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const u32x4 raw = *reinterpret_cast<const u32x4*>(kr + u * EPU);
            const T* e = reinterpret_cast<const T*>(&raw);
#pragma unroll
            for (int j = 0; j < EPU; ++j) s += qf[u * EPU + j] * (float)e[j];
        }
        const float m_new = fmaxf(m, s);
        const float a = __expf(m - m_new), pv = __expf(s - m_new);
        l = l * a + pv;
        m = m_new;
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const u32x4 raw = *reinterpret_cast<const u32x4*>(vr + u * EPU);
            const T* e = reinterpret_cast<const T*>(&raw);
#pragma unroll
            for (int j = 0; j < EPU; ++j) o[u * EPU + j] = o[u * EPU + j] * a + pv * (float)e[j];
        }
    }

    // ---- merge the 64 lanes of a wave: common maximum, rescale, butterfly sums (fixed order: deterministic) ----
    float mw = m;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mw = fmaxf(mw, __shfl_xor(mw, off));
    const float f = __expf(m - mw);              // lanes without a key: m = -1e30 -> f = 0 (or 1 when the whole wave is empty: l = o = 0)
    l *= f;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) l += __shfl_xor(l, off);
#pragma unroll
    for (int d = 0; d < HD; ++d) {
        float x = o[d] * f;
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
        o[d] = x;
    }
    // ---- merge the 4 waves through LDS ----
    __shared__ float red[4][HD + 2];
    if (lane == 0) {
        red[wave][HD] = mw; red[wave][HD + 1] = l;
    }
    if (lane < HD / 1 && lane < 64) {
        // lane d (and d + 64 for hd = 128) publishes o[d]: every lane holds the full sums, pick by a static unrolled select
#pragma unroll
        for (int d = 0; d < HD; ++d) if ((d & 63) == lane) red[wave][d] = o[d];
    }
    __syncthreads();
    if (wave == 0) {
        const float m0 = red[0][HD], m1 = red[1][HD], m2 = red[2][HD], m3 = red[3][HD];
        const float mt = fmaxf(fmaxf(m0, m1), fmaxf(m2, m3));
        const float f0 = __expf(m0 - mt), f1 = __expf(m1 - mt), f2 = __expf(m2 - mt), f3 = __expf(m3 - mt);
        const float lt = red[0][HD + 1] * f0 + red[1][HD + 1] * f1 + red[2][HD + 1] * f2 + red[3][HD + 1] * f3;
        const float inv = 1.0f / lt;
        for (int d = lane; d < HD; d += 64)
            dst[d] = (T)((red[0][d] * f0 + red[1][d] * f1 + red[2][d] * f2 + red[3][d] * f3) * inv);
    }
}

// The head dims the decode kernels are built for: f(std::integral_constant<int, HD>{}) for hd in {16, 32, 64, 128}; false for any other.
template <typename F>
bool decode_dispatch_hd(int hd, F&& f) {
    switch (hd) {
        case 16: f(std::integral_constant<int, 16>{}); return true;
        case 32: f(std::integral_constant<int, 32>{}); return true;
        case 64: f(std::integral_constant<int, 64>{}); return true;
        case 128: f(std::integral_constant<int, 128>{}); return true;
        default: return false;
    }
}
