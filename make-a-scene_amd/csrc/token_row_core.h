// The row walk of the stage-2 token kernels, shared by token_loss.hip (the loss) and token_readout.hip (what a run is judged by), so that
// the two cannot drift.  The head of token_loss.hip describes the walk: one work-group of NT lanes per row, 16-byte
// units and a tail, RESIDENT rows kept in registers, every other row STREAMED with an online (m, l) per lane.
#pragma once
#include "mas_common.h"
#include "mas_wave.h"
#include <math.h>

namespace {

constexpr int NT = 256, NW = NT / 64;
constexpr int KMAX = 4;                 // register-resident 16-byte units per lane: V <= 256 * 4 * (8 bf16 | 4 fp32)

template <typename T> struct Unit { static constexpr int N = 16 / (int)sizeof(T); };

template <typename T, int N>
__device__ __forceinline__ void cvt_unit(const u32x4& raw, float (&v)[N]) {
    const T* e = reinterpret_cast<const T*>(&raw);
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = (float)e[i];
}
template <typename T, int N>
__device__ __forceinline__ void ld_unit(const T* p, float (&v)[N]) {
    const u32x4 raw = *reinterpret_cast<const u32x4*>(p);
    cvt_unit<T, N>(raw, v);
}
template <typename T, int N>
__device__ __forceinline__ void st_unit(T* p, const float (&v)[N]) {
    u32x4 raw;
    T* e = reinterpret_cast<T*>(&raw);
#pragma unroll
    for (int i = 0; i < N; ++i) e[i] = (T)v[i];              // the one rounding from fp32
    *reinterpret_cast<u32x4*>(p) = raw;
}

template <typename T>
__device__ __forceinline__ const T* row_ptr(const T* x, long long r, long long inner, long long outer_stride, long long ld) {
    return x + (r / inner) * outer_stride + (r % inner) * ld;
}
__device__ __forceinline__ bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// How row r is cut.  The row is RESIDENT when `nfull <= KMAX * NT && V - e0 <= NT`.  Each kernel spells that test at its own branch, and
// writes its own loops over the units and the tail: as a function (or as visitors taking the loop bodies) the same operations come out of
// the compiler in another block order and with other registers, which a listing diff cannot tell from a change.
template <typename T> struct RowPlan {
    const T* xr;
    int nfull;                              // 16-byte units; the rest of the row goes element by element
    int e0;                                 // the first tail column
};
template <typename T>
__device__ __forceinline__ RowPlan<T> row_plan(const T* x, long long r, int V, long long inner, long long outer_stride, long long ld) {
    const T* xr = row_ptr(x, r, inner, outer_stride, ld);
    const int nfull = aligned16(xr) ? V / Unit<T>::N : 0;
    return {xr, nfull, nfull * Unit<T>::N};
}

template <int N>
__device__ __forceinline__ float unit_max(const float (&v)[N]) {
    float um = v[0];
#pragma unroll
    for (int e = 1; e < N; ++e) um = fmaxf(um, v[e]);
    return um;
}

// what the exponentials are taken against: the maximum, or 0 while there is none (a row, or a lane's share, of -inf alone)
__device__ __forceinline__ float exp_shift(float m) { return m == -INFINITY ? 0.0f : m; }

// the work-group's exchange of maxima: every lane leaves with the row's.  (s_max is free again after the caller's next barrier.)
__device__ __forceinline__ float row_max(float m, float (&s_max)[NW], int lane, int wave) {
    m = wave_max(m);
    if (lane == 0) s_max[wave] = m;
    __syncthreads();
    return fmaxf(fmaxf(s_max[0], s_max[1]), fmaxf(s_max[2], s_max[3]));
}

// one work-group per row; past 2^20 rows the work-groups walk the rows with the grid as stride
inline unsigned row_grid(long long rows) { return (unsigned)(rows < (1LL << 20) ? rows : (1LL << 20)); }

// what every entry point that reads logits rows checks first (label_smoothing: 0 where the entry has none)
inline int row_check(const char* what, const void* logits, int dtype, long long rows, int V, long long inner, long long outer_stride,
                     long long ld, const void* target, float eps) {
    if (!logits || !target) MAS_FAIL(MAS_EINVAL, "%s: null argument", what);
    if (rows <= 0 || V <= 0 || inner <= 0) MAS_FAIL(MAS_EINVAL, "%s: rows=%lld V=%d inner=%lld must be positive", what, rows, V, inner);
    if (outer_stride < 0 || ld < 0) MAS_FAIL(MAS_EINVAL, "%s: negative stride (outer_stride=%lld ld=%lld)", what, outer_stride, ld);
    if (!(eps >= 0.0f && eps <= 1.0f)) MAS_FAIL(MAS_EINVAL, "%s: label_smoothing=%g outside [0, 1]", what, (double)eps);
    if (dtype != MAS_BF16 && dtype != MAS_F32) MAS_FAIL(MAS_EUNSUPPORTED, "%s: dtype %d (fp32 / bf16 logits)", what, dtype);
    return MAS_OK;
}

}  // namespace
