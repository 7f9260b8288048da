// The per-element arithmetic of the VQ-SEG objective, shared by seg_loss.hip (dense targets) and seg_labels.hip (targets derived from label
// planes): the two ops evaluate every element with THIS code, so they cannot drift.  Formulas: the head of seg_loss.hip, DESIGN 2.10.
#pragma once
#include "mas_common.h"
#include <math.h>

namespace {

constexpr int SEG_NT = 256;              // lanes per work-group of every kernel of the objective

template <typename T> __device__ __forceinline__ float to_f(T v) { return (float)v; }

__device__ __forceinline__ bool aligned_to(const void* p, unsigned bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }

// N consecutive elements as fp32; `vec`: p is aligned to min(16, N sizeof(T)) bytes and is read in loads of that size
template <typename T, int N> struct Chunk {
    static constexpr int CE = (N * (int)sizeof(T) > 16) ? 16 / (int)sizeof(T) : N;
    static constexpr unsigned BYTES = CE * sizeof(T);
};
template <typename T, int N>
__device__ __forceinline__ void ld_n(const T* p, bool vec, float (&v)[N]) {
    if constexpr (N == 1) {
        v[0] = to_f(p[0]);
    } else {
        constexpr int CE = Chunk<T, N>::CE;
        typedef T VT __attribute__((ext_vector_type(CE)));
        if (vec) {
#pragma unroll
            for (int k = 0; k < N / CE; ++k) {
                const VT raw = *reinterpret_cast<const VT*>(p + k * CE);
#pragma unroll
                for (int e = 0; e < CE; ++e) v[k * CE + e] = to_f((T)raw[e]);
            }
        } else {
#pragma unroll
            for (int e = 0; e < N; ++e) v[e] = to_f(p[e]);
        }
    }
}
template <typename T, int N>
__device__ __forceinline__ void st_n(T* p, bool vec, const float (&v)[N]) {     // N sizeof(T) <= 16; the one rounding from fp32
    if constexpr (N == 1) {
        p[0] = (T)v[0];
    } else {
        typedef T VT __attribute__((ext_vector_type(N)));
        if (vec) {
            VT raw;
#pragma unroll
            for (int e = 0; e < N; ++e) raw[e] = (T)v[e];
            *reinterpret_cast<VT*>(p) = raw;
        } else {
#pragma unroll
            for (int e = 0; e < N; ++e) p[e] = (T)v[e];
        }
    }
}

// v = q d + r for v < 2^31, d >= 1, inv = 1.0f / d: the fp32 quotient is off by one at the most, which the remainder shows
__device__ __forceinline__ void divmod(unsigned v, unsigned d, float inv, unsigned& q, unsigned& r) {
    unsigned qq = (unsigned)((float)v * inv);
    int rr = (int)(v - qq * d);
    if (rr < 0) { qq -= 1; rr += (int)d; }
    else if (rr >= (int)d) { qq += 1; rr -= (int)d; }
    q = qq; r = (unsigned)rr;
}

struct Pre {                                     // what forward and backward share of one element
    float e, u, lw, omt;
    __device__ __forceinline__ Pre(float x, float t, float wm1) {
        e = __expf(-fabsf(x));
        u = 1.0f + e;
        lw = fmaf(wm1, t, 1.0f);
        omt = 1.0f - t;
    }
};
__device__ __forceinline__ void elem_fwd(float x, float t, float wm1, bool mse_on, float& bce, float& sq) {
    const Pre p(x, t, wm1);
    const float sp = fmaxf(-x, 0.0f) + __logf(p.u);
    bce += fmaf(p.lw, sp, p.omt * x);
    if (mse_on) {
        const float r = __builtin_amdgcn_rcpf(p.u);
        const float d = (x >= 0.0f ? r : p.e * r) - t;
        sq = fmaf(d, d, sq);
    }
}
__device__ __forceinline__ float elem_bwd(float x, float t, float wm1, bool mse_on, float scale) {
    const Pre p(x, t, wm1);
    const float r = __builtin_amdgcn_rcpf(p.u), er = p.e * r;
    const float s = x >= 0.0f ? r : er, oms = x >= 0.0f ? er : r;
    float d = fmaf(-p.lw, oms, p.omt);
    if (mse_on) d = fmaf(2.0f * (s - t) * s, oms, d);
    return scale * d;
}

// {bce, mse} of the work-group: fp64 tree over the lanes in a fixed order
__device__ __forceinline__ void block_sums(double b, double s, double* __restrict__ partials) {
    __shared__ double s_b[SEG_NT], s_s[SEG_NT];
    const int tid = threadIdx.x;
    s_b[tid] = b; s_s[tid] = s;
    __syncthreads();
    for (int o = SEG_NT / 2; o >= 1; o >>= 1) {
        if (tid < o) { s_b[tid] += s_b[tid + o]; s_s[tid] += s_s[tid + o]; }
        __syncthreads();
    }
    if (tid == 0) { partials[2 * (size_t)blockIdx.x] = s_b[0]; partials[2 * (size_t)blockIdx.x + 1] = s_s[0]; }
}

}  // namespace
