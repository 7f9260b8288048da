// Element-wise dropout y = x o Z * s (ResnetBlock's dropout, reference models/modules.py:99,127), Z from Philox4x32-10 over the flat
// element index (mapping: include/mas_hip.h, "Dropout"; generator and keep rule: mas_philox.h).  One Philox call covers 8 consecutive
// elements: one 16-byte load and store for bf16, two for fp32.  The backward is the same call on dy with the same seed.
#include "mas_common.h"
#include "mas_philox.h"
#include <stdint.h>

namespace {

constexpr int DT_NT = 256;

template <typename T>
__global__ __launch_bounds__(DT_NT) void dropout_apply_kernel(const T* __restrict__ x, T* __restrict__ y, long long n,
                                                              const long long* seed, unsigned t, float sc) {
    const unsigned long long sd = (unsigned long long)seed[0];
    const unsigned s0 = (unsigned)sd, s1 = (unsigned)(sd >> 32), off = (unsigned)(unsigned long long)seed[1];
    const long long groups = (n + 7) / 8, full = n / 8;
    for (long long g = (long long)blockIdx.x * DT_NT + threadIdx.x; g < groups; g += (long long)gridDim.x * DT_NT) {
        const unsigned km = mas_ew_keep8(s0, s1, off, (uint64_t)g, t);
        if (g < full) {
            if constexpr (sizeof(T) == 2) {
                u32x4 raw = *reinterpret_cast<const u32x4*>(x + g * 8);
                bf16x8 v = *reinterpret_cast<const bf16x8*>(&raw);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = (T)(((km >> e) & 1) ? (float)v[e] * sc : 0.0f);
                *reinterpret_cast<u32x4*>(y + g * 8) = *reinterpret_cast<const u32x4*>(&v);
            } else {
#pragma unroll
                for (int hlf = 0; hlf < 2; ++hlf) {
                    f32x4 v = *reinterpret_cast<const f32x4*>(x + g * 8 + 4 * hlf);
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = ((km >> (4 * hlf + e)) & 1) ? v[e] * sc : 0.0f;
                    *reinterpret_cast<f32x4*>(y + g * 8 + 4 * hlf) = v;
                }
            }
        } else {                                   // the last, partial group
            for (long long i = g * 8; i < n; ++i) y[i] = (T)(((km >> (i - g * 8)) & 1) ? (float)x[i] * sc : 0.0f);
        }
    }
}

}  // namespace

extern "C" int mas_dropout_apply(const void* x, void* y, long long n, int dtype, float p, const int64_t* seed, void* stream) {
    MAS_ENTER();
    if (!x || !y || !seed) MAS_FAIL(MAS_EINVAL, "dropout_apply: null argument");
    if (n < 0) MAS_FAIL(MAS_EINVAL, "dropout_apply: n = %lld", n);
    if (!(p >= 0.0f && p <= 1.0f)) MAS_FAIL(MAS_EINVAL, "dropout_apply: p = %g outside [0, 1]", (double)p);
    if (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) != 0)
        MAS_FAIL(MAS_EINVAL, "dropout_apply: x and y must be 16-byte aligned");
    if (n == 0) return MAS_OK;
    const unsigned t = mas_drop_threshold(p);
    const float sc = mas_drop_scale(t);
    const long long groups = (n + 7) / 8;
    const unsigned blocks = (unsigned)(groups / DT_NT + 1 < 256 * 32 ? groups / DT_NT + 1 : 256 * 32);   // grid-stride beyond 32 per CU
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long long* sd = reinterpret_cast<const long long*>(seed);
    if (dtype == MAS_BF16)
        hipLaunchKernelGGL(dropout_apply_kernel<bf16_t>, dim3(blocks), dim3(DT_NT), 0, s, reinterpret_cast<const bf16_t*>(x),
                           reinterpret_cast<bf16_t*>(y), n, sd, t, sc);
    else if (dtype == MAS_F32)
        hipLaunchKernelGGL(dropout_apply_kernel<float>, dim3(blocks), dim3(DT_NT), 0, s, reinterpret_cast<const float*>(x),
                           reinterpret_cast<float*>(y), n, sd, t, sc);
    else
        MAS_FAIL(MAS_EUNSUPPORTED, "dropout_apply: dtype %d", dtype);
    MAS_CHECK_LAUNCH("dropout_apply");
    return MAS_OK;
}
