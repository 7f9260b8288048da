// The keyed bijection of [0, N) of include/mas_hip.h ("Codebook reservoir"), shared by reservoir.hip (streams 0 and 1: positions and
// drop set) and kmeans.hip (stream 2: the initial centroids).  Header-only like mas_philox.h: __host__ __device__ under hipcc, plain C++
// elsewhere, so tests/helpers/reservoir_ref.py's restatement is checked against this very arithmetic compiled for the host.
//
// A balanced Feistel network over 2h bits (4^h >= N), round function = word x of Philox4x32-10 at counter (right half, round, stream,
// calls) under the key (lo32(seed), hi32(seed)); values >= N are walked round the cycle until one lands below N (the cycle through
// x < N returns to x, so the walk ends).
#pragma once
#include "mas_philox.h"

#ifndef RSV_ROUNDS
#define RSV_ROUNDS 4
#endif

MAS_HD uint32_t rsv_half_bits(uint32_t N) {
    uint32_t h = 1;
    while (h < 15 && (1u << (2 * h)) < N) ++h;
    return h;
}
MAS_HD uint32_t rsv_feistel(uint32_t x, uint32_t h, uint32_t stream, uint32_t calls, uint32_t k0, uint32_t k1) {
    const uint32_t mask = (1u << h) - 1u;
    uint32_t l = x >> h, r = x & mask;
#pragma unroll
    for (uint32_t round = 0; round < RSV_ROUNDS; ++round) {
        const uint32_t f = mas_philox4x32_10(MasU32x4{r, round, stream, calls}, k0, k1).x & mask;
        const uint32_t t = l ^ f;
        l = r;
        r = t;
    }
    return (l << h) | r;
}
MAS_HD uint32_t rsv_perm(uint32_t x, uint32_t N, uint32_t h, uint32_t stream, uint32_t calls, uint32_t k0, uint32_t k1) {
    uint32_t y = rsv_feistel(x, h, stream, calls, k0, k1);
    while (y >= N) y = rsv_feistel(y, h, stream, calls, k0, k1);
    return y;
}
