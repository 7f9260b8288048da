// The 64-lane butterfly reductions of gfx950, one spelling for every kernel that needs the same tree: xor offsets 32, 16, ..., 1,
// so every lane ends with the wave's value and the order of the additions is fixed.  Users: token_loss.hip, token_readout.hip (through
// token_row_core.h) and transformer_ew.hip's LayerNorm.  Reductions of another shape (sub-wave groups, LDS trees) stay where they are.
#pragma once
#include "mas_common.h"
#include <math.h>

namespace {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wave_min(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
// how many ACTIVE lanes of the wave hold the predicate: one compare into a lane mask and two scalar instructions.  The callers add it up in
// every active lane; lane 0 has the wave's smallest row index and is active whenever any lane of its wave is, so ITS total is the wave's.
__device__ __forceinline__ int wave_count(bool p) { return __popcll(__ballot(p)); }

}  // namespace
