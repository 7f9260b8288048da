// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11) and the dropout keep rules built on it.
// Header-only; every function is __host__ __device__ under hipcc and plain C++ elsewhere, so host code and the CPU restatement in
// tests/helpers/philox_ref.py follow the same arithmetic.  The (seed, offset, b, h, query, key) -> (counter, key, slot) mapping is
// part of the C contract: include/mas_hip.h, "Dropout".
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MAS_HD __host__ __device__ __forceinline__
#else
#define MAS_HD inline
#endif

struct MasU32x4 { uint32_t x, y, z, w; };

MAS_HD uint32_t mas_mulhi32(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umulhi(a, b);
#else
    return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}

// ctr (c0..c3), key (k0, k1) -> four 32-bit words
MAS_HD MasU32x4 mas_philox4x32_10(MasU32x4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) { k0 += 0x9E3779B9u; k1 += 0xBB67AE85u; }
        const uint32_t hi0 = mas_mulhi32(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
        const uint32_t hi1 = mas_mulhi32(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
        c = MasU32x4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    }
    return c;
}

// ---- keep rule: a 16-bit value u keeps its element iff u >= t, t = round(p * 65536); kept values are scaled by 65536 / (65536 - t)
//      (unbiased for the p = t / 65536 actually used).  t >= 65536 (p = 1) keeps nothing; the scale is then 0, so no inf reaches a product.
MAS_HD uint32_t mas_drop_threshold(float p) {
    const float t = p * 65536.0f + 0.5f;
    return t <= 0.0f ? 0u : (t >= 65536.0f ? 65536u : (uint32_t)t);
}
MAS_HD float mas_drop_scale(uint32_t t) { return t >= 65536u ? 0.0f : 65536.0f / (float)(65536u - t); }

// bits 0/1: keep flags of the low / high 16-bit half of w
MAS_HD uint32_t mas_keep2(uint32_t w, uint32_t t) { return ((w & 0xffffu) >= t ? 1u : 0u) | ((w >> 16) >= t ? 2u : 0u); }

// ---- attention mapping.  One call per (bh = b*H + h, 4-query block, 4-key block, query half):
//        counter = (key >> 2, query >> 1, bh, lo32(offset)),  key = (lo32(seed), hi32(seed)),
//        16-bit slot j = 4 * (query & 1) + (key & 3), slot j = bits 16 (j & 1) .. +15 of word j >> 1.
// Query-major form (lane = query, registers = runs of 4 keys): keep flags of keys kb4 .. kb4 + 3 (kb4 % 4 == 0) for one query.
MAS_HD uint32_t mas_attn_keep_q(uint32_t s0, uint32_t s1, uint32_t off, uint32_t bh, uint32_t query, uint32_t kb4, uint32_t t) {
    const MasU32x4 r = mas_philox4x32_10(MasU32x4{kb4 >> 2, query >> 1, bh, off}, s0, s1);
    const uint32_t w0 = (query & 1) ? r.z : r.x, w1 = (query & 1) ? r.w : r.y;
    return mas_keep2(w0, t) | (mas_keep2(w1, t) << 2);
}
// Key-major form (lane = key, registers = runs of 4 queries): keep flags of queries qb4 .. qb4 + 3 (qb4 % 4 == 0) for one key (2 calls).
MAS_HD uint32_t mas_attn_keep_k(uint32_t s0, uint32_t s1, uint32_t off, uint32_t bh, uint32_t key, uint32_t qb4, uint32_t t) {
    uint32_t m = 0;
#pragma unroll
    for (uint32_t half = 0; half < 2; ++half) {
        const MasU32x4 r = mas_philox4x32_10(MasU32x4{key >> 2, (qb4 >> 1) + half, bh, off}, s0, s1);
        const uint32_t sh = 16 * (key & 1), hiword = (key & 2) != 0;
        const uint32_t even = hiword ? r.y : r.x, odd = hiword ? r.w : r.z;      // query 2 half (slot key & 3), query 2 half + 1 (slot 4 + key & 3)
        m |= ((((even >> sh) & 0xffffu) >= t ? 1u : 0u) | (((odd >> sh) & 0xffffu) >= t ? 2u : 0u)) << (2 * half);
    }
    return m;
}

// ---- element-wise mapping (mas_dropout_apply): element i of the flat tensor uses call (lo32(i >> 3), hi32(i >> 3), 0, lo32(offset)),
//      same key, slot i & 7.  Keep flags of elements 8 g .. 8 g + 7 (bit e = element 8 g + e).
MAS_HD uint32_t mas_ew_keep8(uint32_t s0, uint32_t s1, uint32_t off, uint64_t group, uint32_t t) {
    const MasU32x4 r = mas_philox4x32_10(MasU32x4{(uint32_t)group, (uint32_t)(group >> 32), 0u, off}, s0, s1);
    return mas_keep2(r.x, t) | (mas_keep2(r.y, t) << 2) | (mas_keep2(r.z, t) << 4) | (mas_keep2(r.w, t) << 6);
}

// ---- sampling mapping (mas_sample_tokens): vocabulary entry j of output row r at decode step k uses
//        counter = (j >> 2, k, r, lo32(offset)),  key = (lo32(seed), hi32(seed)),  32-bit slot j & 3 (word x, y, z, w);
//      u = ((bits >> 9) + 0.5) * 2^-23: 23 random bits, every step exact in float32 ((bits >> 9) + 0.5 < 2^23 needs at most 24
//      significant bits), so u lies in [2^-24, 1 - 2^-24], strictly inside (0, 1), and -log(-log u) is finite at both ends.  (With 24
//      bits, (2^24 - 1) + 0.5 rounds to 2^24 in float32 and u = 1 gives a +inf score.)
MAS_HD MasU32x4 mas_sample_bits4(uint32_t s0, uint32_t s1, uint32_t off, uint32_t row, uint32_t step, uint32_t j4) {
    return mas_philox4x32_10(MasU32x4{j4, step, row, off}, s0, s1);
}
MAS_HD float mas_sample_uniform(uint32_t bits) { return ((float)(bits >> 9) + 0.5f) * 1.1920928955078125e-7f; }
