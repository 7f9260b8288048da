// The key-range walk of the shared-prompt decode attention (attn_decode_shared.hip): QT query rows against ONE contiguous range of keys,
// by a 256-lane work-group that loads every 16-byte unit of a key / value row once and uses it for all QT queries.  The lane layout is
// attn_decode_split_partial_kernel's (attn_decode_split.hip): the HD-element row of a key is spread over G = HD*sizeof(T)/16 lanes, the
// work-group holds 256/G key slots, KU keys per slot are loaded before the first is used, the dot products are finished by log2(G)
// butterfly shuffles.  A lane keeps, per query, the online-softmax state (m, l) of its key slot and the 16/sizeof(T) elements of o it
// owns; per query the slots are merged as there (common maximum, rescale, butterfly sums, then the 4 waves through LDS: fixed order)
// and the un-normalised state {o[HD], m, l} goes to dst[i] -- m = -1e30, l = 0, o = 0 for a range without keys.
// Both launches' users -- the prompt tile (QT = DECODE_SHARED_QT) and a candidate's own keys (QT = 1) -- call this ONE function, and
// every query slot of it runs the same instruction sequence (explicit fmaf: nothing left to contract differently per slot), so a row's
// bits do not depend on its place in the tile.
#pragma once
#include "attn_decode_core.h"

constexpr int DECODE_TILE_GRAN = 32;             // a split's key range is a multiple of this
constexpr int DECODE_TILE_KU = 4;                // keys in flight per slot

// floats of LDS the walk needs for QT queries
template <int HD, int QT>
constexpr int decode_tile_lds_floats() { return QT * 4 * (HD + 2); }

// [begin, end) of split `split` of `nsplit` over L keys: chunks of ceil(L / nsplit) rounded up to DECODE_TILE_GRAN (end <= begin: no key)
__device__ __forceinline__ void decode_tile_range(int L, int nsplit, int split, int& begin, int& end) {
    const int chunk = ((L + nsplit - 1) / nsplit + DECODE_TILE_GRAN - 1) / DECODE_TILE_GRAN * DECODE_TILE_GRAN;
    begin = split * chunk;
    end = min(L, begin + chunk);
}

// Q[i]: query row i of this head; K, V: key 0 of this head, ld_k / ld_v elements between keys (all 16-byte aligned); dst[i]: where the
// HD + 2 floats of query i's state go, or null (a clamped row past the end of its group: computed, not stored); red: the LDS above.
// Called by all 256 lanes of the work-group (shuffles and one __syncthreads()).
template <typename T, int HD, int QT>
__device__ __forceinline__ void decode_tile_partial(const T* const (&Q)[QT], const T* K, const T* V, int ld_k, int ld_v, int begin, int end,
                                                    float scale, float* const (&dst)[QT], float* red) {
    constexpr int EPU = 16 / (int)sizeof(T);     // elements of a 16-byte unit
    constexpr int G = HD / EPU;                  // lanes per key row (2 .. 32)
    constexpr int KPP = DECODE_NT / G;           // key slots of the work-group
    constexpr int KU = DECODE_TILE_KU;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int u = tid % G, slot = tid / G;
    K += u * EPU;
    V += u * EPU;

    float qf[QT][EPU];                           // this lane's unit of every query, pre-scaled (transformer.py:56: q / sqrt(hd))
#pragma unroll
    for (int i = 0; i < QT; ++i) {
        const u32x4 raw = *reinterpret_cast<const u32x4*>(Q[i] + u * EPU);
        const T* e = reinterpret_cast<const T*>(&raw);
#pragma unroll
        for (int j = 0; j < EPU; ++j) qf[i][j] = (float)e[j] * scale;
    }

    float m[QT], l[QT], o[QT][EPU];
#pragma unroll
    for (int i = 0; i < QT; ++i) {
        m[i] = -1e30f; l[i] = 0.0f;
#pragma unroll
        for (int j = 0; j < EPU; ++j) o[i][j] = 0.0f;
    }

    for (int base = begin; base < end; base += KPP * KU) {      // uniform over the work-group: the shuffles below see every lane
        u32x4 kraw[KU], vraw[KU];
#pragma unroll
        for (int t = 0; t < KU; ++t) {
            const int key = base + t * KPP + slot;
            kraw[t] = u32x4{0u, 0u, 0u, 0u};
            vraw[t] = u32x4{0u, 0u, 0u, 0u};
            if (key < end) {                     // rows from `end` on are never loaded
                kraw[t] = *reinterpret_cast<const u32x4*>(K + (size_t)key * ld_k);
                vraw[t] = *reinterpret_cast<const u32x4*>(V + (size_t)key * ld_v);
            }
        }
#pragma unroll
        for (int t = 0; t < KU; ++t) {
            const int key = base + t * KPP + slot;
            const T* ke = reinterpret_cast<const T*>(&kraw[t]);
            const T* ve = reinterpret_cast<const T*>(&vraw[t]);
            float kf[EPU], vf[EPU], s[QT];       // the unit is converted once for the QT queries
#pragma unroll
            for (int j = 0; j < EPU; ++j) { kf[j] = (float)ke[j]; vf[j] = (float)ve[j]; }
#pragma unroll
            for (int i = 0; i < QT; ++i) {
                float x = 0.0f;
#pragma unroll
                for (int j = 0; j < EPU; ++j) x = fmaf(qf[i][j], kf[j], x);
#pragma unroll
                for (int off = G / 2; off >= 1; off >>= 1) x += __shfl_xor(x, off);   // the G lanes of the row: the same sum in each
                s[i] = x;
            }
            if (key < end) {
#pragma unroll
                for (int i = 0; i < QT; ++i) {
                    const float m_new = fmaxf(m[i], s[i]);
                    const float a = __expf(m[i] - m_new), pv = __expf(s[i] - m_new);
                    l[i] = fmaf(l[i], a, pv);
                    m[i] = m_new;
#pragma unroll
                    for (int j = 0; j < EPU; ++j) o[i][j] = fmaf(pv, vf[j], o[i][j] * a);
                }
            }
        }
    }

#pragma unroll
    for (int i = 0; i < QT; ++i) {
        // ---- merge the 64 / G slots of a wave: common maximum, rescale, butterfly sums (fixed order: deterministic) ----
        float mw = m[i];
#pragma unroll
        for (int off = 32; off >= G; off >>= 1) mw = fmaxf(mw, __shfl_xor(mw, off));
        const float f = __expf(m[i] - mw);       // slots without a key: m = -1e30 -> f = 0 (or 1 when the whole wave is empty: l = o = 0)
        float lw = l[i] * f;
#pragma unroll
        for (int off = 32; off >= G; off >>= 1) lw += __shfl_xor(lw, off);
        float* r = red + (i * 4 + wave) * (HD + 2);
#pragma unroll
        for (int j = 0; j < EPU; ++j) {
            float x = o[i][j] * f;
#pragma unroll
            for (int off = 32; off >= G; off >>= 1) x += __shfl_xor(x, off);
            if (lane < G) r[lane * EPU + j] = x;
        }
        if (lane == 0) {
            r[HD] = mw; r[HD + 1] = lw;
        }
    }
    // ---- merge the 4 waves through LDS, write each query's state ----
    __syncthreads();
    if (tid < HD + 2) {
#pragma unroll
        for (int i = 0; i < QT; ++i) {
            const float* r = red + i * 4 * (HD + 2);
            const float m0 = r[HD], m1 = r[(HD + 2) + HD], m2 = r[2 * (HD + 2) + HD], m3 = r[3 * (HD + 2) + HD];
            const float mt = fmaxf(fmaxf(m0, m1), fmaxf(m2, m3));
            const float f0 = __expf(m0 - mt), f1 = __expf(m1 - mt), f2 = __expf(m2 - mt), f3 = __expf(m3 - mt);
            const float x = fmaf(r[3 * (HD + 2) + tid], f3, fmaf(r[2 * (HD + 2) + tid], f2, fmaf(r[(HD + 2) + tid], f1, r[tid] * f0)));
            if (dst[i]) dst[i][tid] = tid == HD ? mt : x;        // o[d] and, at HD + 1, l
        }
    }
}
