// What object.hip (LPIPS on every object crop of an atlas) and lpips.hip (LPIPS on whole images) share: NHWC maps, 8 channels per lane,
// bf16 or fp32 storage, fp32 arithmetic, no float atomics.  The pieces here are the ones whose move left both files' device code
// unchanged, instruction for instruction.
// Kept in both files, in the same words: the per-pixel head arithmetic (head_fwd_kernel, head_bwd_kernel with its |f| = 0 rule) and the
// first-maximum routing of pool_bwd_kernel.  As function templates they compile to the same operations with operands and registers
// swapped, which nothing short of a run on the GPU tells from a change; an edit to one file's copy belongs in the other's too.
// Different in the two files, on purpose:
//   pool_fwd : object.hip takes fmaxf over the window (its ReLU has turned every NaN into 0); lpips.hip scans the window as torch does, a
//              NaN replacing the maximum;
//   finalize : object.hip adds a cell's few partial sums serially, one lane per cell; lpips.hip has up to 2^18 per image and level and
//              adds them as 256 chains and a tree;
//   relu_fwd : object.hip also zeroes what lies outside the cells' rectangles; lpips.hip has no cells and keeps a NaN, as F.relu does;
//   head_c_ok: each file says which head widths its entry points take (a power of two in 64 .. 512 there, VGG16's list here: the same
//              four today, but the object term's atlas and the whole-image path need not move together);
//   lpips.hip also bounds the pixels of one image (check_image).
#pragma once
#include "mas_common.h"

namespace {

constexpr int NT = 256;
constexpr int CP = MAS_OBJ_CANVAS_C;       // canvas channels: RGB + zeros (one 16-byte vector in bf16)
constexpr int HEAD_PASSES = 4;             // pixel passes of one head block: 8192 / C pixels = HEAD_PASSES * NT / (C / 8)

template <typename T> using V8 = typename Vec8<T>::type;

__device__ __forceinline__ float ld_img(const MasFaceImage& im, long long off) {
    return im.dtype == MAS_BF16 ? (float)reinterpret_cast<const bf16_t*>(im.data)[off] : reinterpret_cast<const float*>(im.data)[off];
}

__device__ __forceinline__ long long gsize() { return (long long)gridDim.x * NT; }
__device__ __forceinline__ long long gtid() { return (long long)blockIdx.x * NT + threadIdx.x; }

// sum over the G lanes of one pixel group (G a power of two <= 64, groups aligned inside the wave)
__device__ __forceinline__ float group_sum(float v, int G) {
    for (int m = G >> 1; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

// the last step of pool_bwd: the gradient g passes where the activation av of the level below is positive (its ReLU mask)
template <typename T>
__device__ __forceinline__ V8<T> relu_mask(V8<T> av, const float (&g)[8]) {
    V8<T> o;
#pragma unroll
    for (int k = 0; k < 8; ++k) o[k] = (T)((float)av[k] > 0.0f ? g[k] : 0.0f);
    return o;
}

// a head block's partial sum: lane g * G speaks for pixel group g; lane 0 adds the NT / G groups in group order
__device__ __forceinline__ void head_block_sum(float acc, float (&red)[NT], int G, float* dst) {
    red[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.0f;
        for (int g = 0; g < NT / G; ++g) s += red[g * G];
        *dst = s;
    }
}

inline int grid_for(long long n) {
    long long g = (n + NT - 1) / NT;
    const long long cap = 16LL * mas_num_cus();
    return (int)(g > cap ? cap : (g < 1 ? 1 : g));
}

inline bool dt_ok(int dt) { return dt == MAS_F32 || dt == MAS_BF16; }

inline int check_img(const MasFaceImage* im, const char* what) {
    if (!im || !im->data) MAS_FAIL(MAS_EINVAL, "%s: null image", what);
    if (!dt_ok(im->dtype)) MAS_FAIL(MAS_EINVAL, "%s: dtype %d", what, im->dtype);
    if (im->C != 3 || im->N <= 0 || im->H <= 0 || im->W <= 0) MAS_FAIL(MAS_EINVAL, "%s: need [N>0, 3, H>0, W>0], got C=%d", what, im->C);
    return MAS_OK;
}

}  // namespace
