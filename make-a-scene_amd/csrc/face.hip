// FaceLoss (reference losses/face_loss.py) on gfx950: the passes of the face-aware VQ-IMG term that are not convolutions.
//
// The network is a frozen caffe-style ResNet-50 in evaluation mode on at most six 254 x 254 face crops per call; its 52 1x1 / 3x3
// convolutions run on the library's convolution kernels (mas_conv_fwd), everything else is here:
//   crop + Resize(256) + CenterCrop(254) of every face row, and its adjoint as a gather (no atomics: overlapping boxes are summed in
//     row order, so d rec is bitwise reproducible -- torch's bilinear backward on the GPU scatters with atomics);
//   the 7x7 / stride-2 stem and its data gradient (direct: 3 input channels do not fill an MFMA tile);
//   bn1 + ReLU + MaxPool(3, 2, ceil) in one pass, and its backward in one pass (one byte per output: the window index of the first
//     maximum, torch's tie rule);
//   the 53 evaluation-mode BatchNorm affine pairs from the running statistics, one launch per forward (never cached: DDP's
//     broadcast_buffers rewrites the buffers before every forward);
//   the Bottleneck join relu(bn3(y3) + shortcut) and the ReLU-mask-times-scale backward passes;
//   the feature L1 distances (fixed-order two-stage sums) and their gradient seeds;
//   the crop, its adjoint and the L1 passes once more with the rows read from a device table of six fixed slots (*_dev): launch
//     arguments, grids and shapes that do not depend on the boxes, for a captured graph.
// Activations are NHWC in bf16 or fp32; arithmetic in fp32.
#include "mas_common.h"

namespace {

constexpr int NT = 256;
constexpr int FS = MAS_FACE_SIZE;          // 254
constexpr int STEM_C = 64;
constexpr int STEM_O = 127;                // (254 + 6 - 7) / 2 + 1
constexpr int STEM_TAPS = 7 * 7 * 3;
constexpr int L1_QUADS = 4;                // quads per thread and block pass of the L1 partial sums
constexpr int L1_CHUNK = NT * 4 * L1_QUADS;

struct RowTable { MasFaceRow r[MAS_FACE_MAX_ROWS]; };

template <typename T> __device__ __forceinline__ float round_to(float v) { return (float)(T)v; }

__device__ __forceinline__ float ld_any(const void* p, int dtype, long long off) {
    return dtype == MAS_BF16 ? (float)reinterpret_cast<const bf16_t*>(p)[off] : reinterpret_cast<const float*>(p)[off];
}

// ---- torch's antialiased bilinear resize weights (aten UpSampleKernel, _compute_indices_min_size_weights_aa, align_corners = False):
// output i of an in_size -> out_size resize reads inputs [lo, hi) with triangle weights of support max(scale, 1), normalised by their sum.
// Upscaling (scale < 1) this is plain bilinear with edge clamping.
__device__ __forceinline__ float tri(float x) { x = fabsf(x); return x < 1.0f ? 1.0f - x : 0.0f; }
struct Taps { int lo, hi; float center, inv, total; };
__device__ __forceinline__ Taps make_taps(int i, int in_size, float scale) {
    const float support = scale >= 1.0f ? scale : 1.0f;
    Taps t;
    t.inv = scale >= 1.0f ? 1.0f / scale : 1.0f;
    t.center = scale * ((float)i + 0.5f);
    t.lo = max((int)(t.center - support + 0.5f), 0);
    t.hi = min((int)(t.center + support + 0.5f), in_size);
    float tot = 0.0f;
    for (int j = t.lo; j < t.hi; ++j) tot += tri(((float)j - t.center + 0.5f) * t.inv);
    t.total = tot;
    return t;
}
__device__ __forceinline__ float tap_weight(const Taps& t, int j) {
    if (j < t.lo || j >= t.hi || t.total == 0.0f) return 0.0f;
    return tri(((float)j - t.center + 0.5f) * t.inv) / t.total;
}

// one thread per output pixel of one row (blockIdx.y = row): three channels
template <typename TO>
__global__ __launch_bounds__(NT) void crop_fwd_kernel(MasFaceImage img, MasFaceImage rec, RowTable rows, TO* __restrict__ out) {
    const int r = blockIdx.y;
    const int p = blockIdx.x * NT + threadIdx.x;
    if (p >= FS * FS) return;
    const MasFaceRow row = rows.r[r];
    const MasFaceImage& im = row.src ? rec : img;
    const int oy = p / FS, ox = p % FS;
    const float sy = (float)row.h / (float)row.rh, sx = (float)row.w / (float)row.rw;
    const Taps ty = make_taps(oy + row.ct, row.h, sy), tx = make_taps(ox + row.cl, row.w, sx);
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (int j = ty.lo; j < ty.hi; ++j) {
        const float wy = tap_weight(ty, j);
        const int iy = row.top + j;
        float h[3] = {0.0f, 0.0f, 0.0f};
        if (iy >= 0 && iy < im.H) {
            for (int i = tx.lo; i < tx.hi; ++i) {
                const int ix = row.left + i;
                if (ix < 0 || ix >= im.W) continue;
                const float wx = tap_weight(tx, i);
                const long long base = (long long)row.b * im.sn + (long long)iy * im.sh + (long long)ix * im.sw;
#pragma unroll
                for (int c = 0; c < 3; ++c) h[c] += wx * ld_any(im.data, im.dtype, base + c * im.sc);
            }
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[c] += wy * h[c];
    }
    TO* o = out + ((size_t)r * FS * FS + p) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (TO)acc[c];
}

// one thread per pixel of d rec: the rows whose box covers it, in table order; inside a row the output pixels whose taps reach it
template <typename TR>
__global__ __launch_bounds__(NT) void crop_bwd_kernel(const float* __restrict__ dfaces, RowTable rows, int n_rows, MasFaceImage drec) {
    const long long p = (long long)blockIdx.x * NT + threadIdx.x;
    const long long hw = (long long)drec.H * drec.W;
    if (p >= (long long)drec.N * hw) return;
    const int b = (int)(p / hw);
    const int y = (int)((p % hw) / drec.W), x = (int)(p % drec.W);
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (int r = 0; r < n_rows; ++r) {
        const MasFaceRow row = rows.r[r];
        const int cy = y - row.top, cx = x - row.left;
        if (row.b != b || cy < 0 || cy >= row.h || cx < 0 || cx >= row.w) continue;
        const float sy = (float)row.h / (float)row.rh, sx = (float)row.w / (float)row.rw;
        const float supy = sy >= 1.0f ? sy : 1.0f, supx = sx >= 1.0f ? sx : 1.0f;
        // resized indices i whose window [center - support, center + support) can hold the input index: center = s (i + 0.5)
        const int ylo = max((int)floorf(((float)cy + 0.5f - supy) / sy - 0.5f) - 1, row.ct);
        const int yhi = min((int)ceilf(((float)cy + 0.5f + supy) / sy - 0.5f) + 1, row.ct + FS - 1);
        const int xlo = max((int)floorf(((float)cx + 0.5f - supx) / sx - 0.5f) - 1, row.cl);
        const int xhi = min((int)ceilf(((float)cx + 0.5f + supx) / sx - 0.5f) + 1, row.cl + FS - 1);
        const float* d = dfaces + (size_t)r * FS * FS * 3;
        for (int i = ylo; i <= yhi; ++i) {
            const float wy = tap_weight(make_taps(i, row.h, sy), cy);
            if (wy == 0.0f) continue;
            float h[3] = {0.0f, 0.0f, 0.0f};
            for (int k = xlo; k <= xhi; ++k) {
                const float wx = tap_weight(make_taps(k, row.w, sx), cx);
                if (wx == 0.0f) continue;
                const float* g = d + ((size_t)(i - row.ct) * FS + (k - row.cl)) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) h[c] += wx * g[c];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += wy * h[c];
        }
    }
    TR* o = reinterpret_cast<TR*>(drec.data);
    const long long base = (long long)b * drec.sn + (long long)y * drec.sh + (long long)x * drec.sw;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[base + c * drec.sc] = (TR)acc[c];
}

// ---- the rows in a DEVICE table of MAS_FACE_SLOTS slots (MAS_FACE_TABLE_INTS int32, include/mas_hip.h): arguments, grids and shapes do
// not depend on the boxes.
// A slot counts as empty unless its flag is set AND its fields could have passed check_rows (the host's check is the contract; this
// one keeps a table that was never written, or written for other images, from indexing outside them).
constexpr int SLOTS = MAS_FACE_SLOTS;
constexpr int PAIRS = SLOTS / 2;
struct FaceSlots { MasFaceRow row[SLOTS]; int32_t valid[SLOTS]; int32_t n_pairs; int32_t pad_; };       // the table's ints, named
static_assert(sizeof(MasFaceRow) == 10 * sizeof(int32_t) && sizeof(FaceSlots) == MAS_FACE_TABLE_INTS * sizeof(int32_t), "the table's layout");

__device__ __forceinline__ bool slot_ok(const MasFaceRow& r, int valid, int n_images) {
    return valid != 0 && (unsigned)r.src <= 1u && (unsigned)r.b < (unsigned)n_images && r.h > 0 && r.w > 0 && r.rh >= FS && r.rw >= FS &&
           r.ct >= 0 && r.cl >= 0 && r.ct <= r.rh - FS && r.cl <= r.rw - FS;
}

// bit q: pair q = (slot q, slot PAIRS + q) is valid.  The table's address and the indices are uniform: scalar loads, once per wave.
// (The L1 passes read feature rows only, never the images: any b >= 0 is in range for them.)
__device__ __forceinline__ unsigned pair_mask(const FaceSlots* __restrict__ t) {
    const int np = min(max(t->n_pairs, 0), PAIRS);
    unsigned m = 0u;
#pragma unroll
    for (int q = 0; q < PAIRS; ++q)
        if (q < np && slot_ok(t->row[q], t->valid[q], 0x7fffffff) && slot_ok(t->row[PAIRS + q], t->valid[PAIRS + q], 0x7fffffff)) m |= 1u << q;
    return m;
}
__device__ __forceinline__ int row_of(long long e, long long chw) { return (e >= chw) + (e >= 2 * chw); }     // e < PAIRS * chw
static_assert(PAIRS == 3, "row_of counts two row boundaries");

// crop_fwd_kernel with the row read from the table (blockIdx.y = slot); an empty slot's row is zeros
template <typename TO>
__global__ __launch_bounds__(NT) void crop_fwd_dev_kernel(MasFaceImage img, MasFaceImage rec, const FaceSlots* __restrict__ table,
                                                          TO* __restrict__ out) {
    const int r = blockIdx.y;
    const int p = blockIdx.x * NT + threadIdx.x;
    if (p >= FS * FS) return;
    const MasFaceRow row = table->row[r];
    const MasFaceImage& im = row.src ? rec : img;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    if (slot_ok(row, table->valid[r], im.N)) {
        const int oy = p / FS, ox = p % FS;
        const float sy = (float)row.h / (float)row.rh, sx = (float)row.w / (float)row.rw;
        const Taps ty = make_taps(oy + row.ct, row.h, sy), tx = make_taps(ox + row.cl, row.w, sx);
        for (int j = ty.lo; j < ty.hi; ++j) {
            const float wy = tap_weight(ty, j);
            const int iy = row.top + j;
            float h[3] = {0.0f, 0.0f, 0.0f};
            if (iy >= 0 && iy < im.H) {
                for (int i = tx.lo; i < tx.hi; ++i) {
                    const int ix = row.left + i;
                    if (ix < 0 || ix >= im.W) continue;
                    const float wx = tap_weight(tx, i);
                    const long long base = (long long)row.b * im.sn + (long long)iy * im.sh + (long long)ix * im.sw;
#pragma unroll
                    for (int c = 0; c < 3; ++c) h[c] += wx * ld_any(im.data, im.dtype, base + c * im.sc);
                }
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += wy * h[c];
        }
    }
    TO* o = out + ((size_t)r * FS * FS + p) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[c] = (TO)acc[c];
}

// crop_bwd_kernel over slots PAIRS .. SLOTS - 1 in that order (dfaces [PAIRS][FS][FS][3]): the slots that hold a rec row
template <typename TR>
__global__ __launch_bounds__(NT) void crop_bwd_dev_kernel(const float* __restrict__ dfaces, const FaceSlots* __restrict__ table,
                                                          MasFaceImage drec) {
    const long long p = (long long)blockIdx.x * NT + threadIdx.x;
    const long long hw = (long long)drec.H * drec.W;
    if (p >= (long long)drec.N * hw) return;
    const int b = (int)(p / hw);
    const int y = (int)((p % hw) / drec.W), x = (int)(p % drec.W);
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (int r = 0; r < PAIRS; ++r) {
        const MasFaceRow row = table->row[PAIRS + r];
        if (!slot_ok(row, table->valid[PAIRS + r], drec.N) || row.src != 1) continue;
        const int cy = y - row.top, cx = x - row.left;
        if (row.b != b || cy < 0 || cy >= row.h || cx < 0 || cx >= row.w) continue;
        const float sy = (float)row.h / (float)row.rh, sx = (float)row.w / (float)row.rw;
        const float supy = sy >= 1.0f ? sy : 1.0f, supx = sx >= 1.0f ? sx : 1.0f;
        const int ylo = max((int)floorf(((float)cy + 0.5f - supy) / sy - 0.5f) - 1, row.ct);
        const int yhi = min((int)ceilf(((float)cy + 0.5f + supy) / sy - 0.5f) + 1, row.ct + FS - 1);
        const int xlo = max((int)floorf(((float)cx + 0.5f - supx) / sx - 0.5f) - 1, row.cl);
        const int xhi = min((int)ceilf(((float)cx + 0.5f + supx) / sx - 0.5f) + 1, row.cl + FS - 1);
        const float* d = dfaces + (size_t)r * FS * FS * 3;
        for (int i = ylo; i <= yhi; ++i) {
            const float wy = tap_weight(make_taps(i, row.h, sy), cy);
            if (wy == 0.0f) continue;
            float h[3] = {0.0f, 0.0f, 0.0f};
            for (int k = xlo; k <= xhi; ++k) {
                const float wx = tap_weight(make_taps(k, row.w, sx), cx);
                if (wx == 0.0f) continue;
                const float* g = d + ((size_t)(i - row.ct) * FS + (k - row.cl)) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) h[c] += wx * g[c];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] += wy * h[c];
        }
    }
    TR* o = reinterpret_cast<TR*>(drec.data);
    const long long base = (long long)b * drec.sn + (long long)y * drec.sh + (long long)x * drec.sw;
#pragma unroll
    for (int c = 0; c < 3; ++c) o[base + c * drec.sc] = (TR)acc[c];
}

// the stem's weights in LDS as [kh][kw][ci][co] fp32 (37.6 KB): every lane of a wave reads the same address (broadcast)
__device__ __forceinline__ void stage_stem_weights(const float* __restrict__ w, float* ws) {
    for (int i = threadIdx.x; i < STEM_TAPS * STEM_C; i += NT) {
        const int co = i % STEM_C, tap = i / STEM_C;
        const int kh = tap / 21, kw = (tap / 3) % 7, ci = tap % 3;
        ws[i] = w[((co * 3 + ci) * 7 + kh) * 7 + kw];
    }
    __syncthreads();
}

// one thread per output pixel of one row: 64 accumulators
template <typename T>
__global__ __launch_bounds__(NT) void stem_fwd_kernel(const T* __restrict__ x, const float* __restrict__ w, T* __restrict__ y) {
    __shared__ float ws[STEM_TAPS * STEM_C];
    stage_stem_weights(w, ws);
    const int r = blockIdx.y;
    const int p = blockIdx.x * NT + threadIdx.x;
    if (p >= STEM_O * STEM_O) return;
    const int oy = p / STEM_O, ox = p % STEM_O;
    const T* xr = x + (size_t)r * FS * FS * 3;
    float acc[STEM_C];
#pragma unroll
    for (int c = 0; c < STEM_C; ++c) acc[c] = 0.0f;
    for (int kh = 0; kh < 7; ++kh) {
        const int iy = 2 * oy - 3 + kh;
        if (iy < 0 || iy >= FS) continue;
        for (int kw = 0; kw < 7; ++kw) {
            const int ix = 2 * ox - 3 + kw;
            if (ix < 0 || ix >= FS) continue;
            const T* px = xr + ((size_t)iy * FS + ix) * 3;
#pragma unroll
            for (int ci = 0; ci < 3; ++ci) {
                const float v = (float)px[ci];
                const f32x4* wr = reinterpret_cast<const f32x4*>(ws + ((kh * 7 + kw) * 3 + ci) * STEM_C);
#pragma unroll
                for (int q = 0; q < STEM_C / 4; ++q) {
                    const f32x4 wv = wr[q];
                    acc[4 * q + 0] += v * wv[0]; acc[4 * q + 1] += v * wv[1];
                    acc[4 * q + 2] += v * wv[2]; acc[4 * q + 3] += v * wv[3];
                }
            }
        }
    }
    T* o = y + ((size_t)r * STEM_O * STEM_O + p) * STEM_C;
#pragma unroll
    for (int q = 0; q < STEM_C / 4; ++q) Quad<T>::st(o + 4 * q, f32x4{acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]});
}

// one thread per input pixel of one row: the <= 4 x 4 taps of matching parity
template <typename T>
__global__ __launch_bounds__(NT) void stem_dgrad_kernel(const T* __restrict__ dy, const float* __restrict__ w, float* __restrict__ dx) {
    __shared__ float ws[STEM_TAPS * STEM_C];
    stage_stem_weights(w, ws);
    const int r = blockIdx.y;
    const int p = blockIdx.x * NT + threadIdx.x;
    if (p >= FS * FS) return;
    const int iy = p / FS, ix = p % FS;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (int kh = (iy + 3) & 1; kh < 7; kh += 2) {
        const int oy = (iy + 3 - kh) >> 1;
        if (oy < 0 || oy >= STEM_O) continue;
        for (int kw = (ix + 3) & 1; kw < 7; kw += 2) {
            const int ox = (ix + 3 - kw) >> 1;
            if (ox < 0 || ox >= STEM_O) continue;
            const T* g = dy + (((size_t)r * STEM_O + oy) * STEM_O + ox) * STEM_C;
            const float* wt = ws + (kh * 7 + kw) * 3 * STEM_C;
#pragma unroll 4
            for (int q = 0; q < STEM_C / 4; ++q) {
                const f32x4 gv = Quad<T>::ld(g + 4 * q);
#pragma unroll
                for (int ci = 0; ci < 3; ++ci) {
                    const f32x4 wv = *reinterpret_cast<const f32x4*>(wt + ci * STEM_C + 4 * q);
                    acc[ci] += gv[0] * wv[0] + gv[1] * wv[1] + gv[2] * wv[2] + gv[3] * wv[3];
                }
            }
        }
    }
    float* o = dx + ((size_t)r * FS * FS + p) * 3;
#pragma unroll
    for (int ci = 0; ci < 3; ++ci) o[ci] = acc[ci];
}

// one block per BatchNorm layer
__global__ __launch_bounds__(NT) void bn_fold_kernel(const MasFaceBnItem* __restrict__ items, float* __restrict__ ss) {
    const MasFaceBnItem it = items[blockIdx.x];
    for (int c = threadIdx.x; c < it.C; c += NT) {
        const float scale = it.weight[c] / sqrtf(it.var[c] + it.eps);
        ss[2 * (it.off + c)] = scale;
        ss[2 * (it.off + c) + 1] = it.bias[c] - it.mean[c] * scale;
    }
}

__host__ __device__ __forceinline__ int pool_out(int n) {     // MaxPool2d(3, 2, padding 0, ceil_mode): the last window starts inside
    int o = (n - 3 + 1) / 2 + 1;
    if ((o - 1) * 2 >= n) --o;
    return o;
}

// one thread per output quad (4 channels)
template <typename T>
__global__ __launch_bounds__(NT) void pool_fwd_kernel(const T* __restrict__ y, const float* __restrict__ ss, T* __restrict__ z,
                                                      unsigned* __restrict__ idx, int R, int H, int W, int C, int Ho, int Wo) {
    const int cq = C / 4;
    const long long total = (long long)R * Ho * Wo * cq;
    const long long t = (long long)blockIdx.x * NT + threadIdx.x;
    if (t >= total) return;
    const int q = (int)(t % cq); long long rest = t / cq;
    const int ow = (int)(rest % Wo); rest /= Wo;
    const int oh = (int)(rest % Ho); const int r = (int)(rest / Ho);
    const f32x4 sc = {ss[8 * q], ss[8 * q + 2], ss[8 * q + 4], ss[8 * q + 6]};
    const f32x4 sh = {ss[8 * q + 1], ss[8 * q + 3], ss[8 * q + 5], ss[8 * q + 7]};
    float best[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    unsigned bi[4] = {0u, 0u, 0u, 0u};
    for (int kh = 0; kh < 3; ++kh) {
        const int ih = 2 * oh + kh;
        if (ih >= H) break;
        for (int kw = 0; kw < 3; ++kw) {
            const int iw = 2 * ow + kw;
            if (iw >= W) break;
            const f32x4 v = Quad<T>::ld(y + (((size_t)r * H + ih) * W + iw) * C + 4 * q);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float u = round_to<T>(fmaxf(v[j] * sc[j] + sh[j], 0.0f));     // the stored ReLU output, compared as torch compares it
                if (u > best[j]) { best[j] = u; bi[j] = (unsigned)(kh * 3 + kw); }
            }
        }
    }
    const size_t o = (((size_t)r * Ho + oh) * Wo + ow) * C + 4 * q;
    Quad<T>::st(z + o, f32x4{best[0], best[1], best[2], best[3]});
    idx[o / 4] = bi[0] | (bi[1] << 8) | (bi[2] << 16) | (bi[3] << 24);
}

// one thread per input quad: gather the outputs whose first maximum sits here (fixed order), then ReLU' * scale, plus the seed
template <typename T>
__global__ __launch_bounds__(NT) void pool_bwd_kernel(const T* __restrict__ y, const float* __restrict__ ss, const T* __restrict__ dz,
                                                      const unsigned* __restrict__ idx, const T* __restrict__ seed, T* __restrict__ dy,
                                                      int R, int H, int W, int C, int Ho, int Wo) {
    const int cq = C / 4;
    const long long total = (long long)R * H * W * cq;
    const long long t = (long long)blockIdx.x * NT + threadIdx.x;
    if (t >= total) return;
    const int q = (int)(t % cq); long long rest = t / cq;
    const int iw = (int)(rest % W); rest /= W;
    const int ih = (int)(rest % H); const int r = (int)(rest / H);
    float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    const int oh0 = max((ih - 1) / 2, 0), oh1 = min(ih / 2, Ho - 1);
    const int ow0 = max((iw - 1) / 2, 0), ow1 = min(iw / 2, Wo - 1);
    for (int oh = oh0; oh <= oh1; ++oh) {
        for (int ow = ow0; ow <= ow1; ++ow) {
            const unsigned k = (unsigned)((ih - 2 * oh) * 3 + (iw - 2 * ow));
            const size_t o = (((size_t)r * Ho + oh) * Wo + ow) * C + 4 * q;
            const unsigned m = idx[o / 4];
            const f32x4 g = Quad<T>::ld(dz + o);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (((m >> (8 * j)) & 0xffu) == k) acc[j] += g[j];
        }
    }
    const size_t i = (((size_t)r * H + ih) * W + iw) * C + 4 * q;
    const f32x4 v = Quad<T>::ld(y + i);
    f32x4 out;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float sc = ss[8 * q + 2 * j], sh = ss[8 * q + 2 * j + 1];
        out[j] = v[j] * sc + sh > 0.0f ? acc[j] * sc : 0.0f;
    }
    if (seed) out += Quad<T>::ld(seed + i);
    Quad<T>::st(dy + i, out);
}

template <typename T>
__global__ __launch_bounds__(NT) void join_fwd_kernel(const T* __restrict__ y3, const float* __restrict__ ss3, const T* __restrict__ r,
                                                      const float* __restrict__ ssr, T* __restrict__ out, long long n4, int C) {
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n4; i += (long long)gridDim.x * NT) {
        const int c = (int)((i * 4) % C);
        const f32x4 a = Quad<T>::ld(y3 + 4 * i), b = Quad<T>::ld(r + 4 * i);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float u = a[j] * ss3[2 * (c + j)] + ss3[2 * (c + j) + 1];
            const float v = ssr ? b[j] * ssr[2 * (c + j)] + ssr[2 * (c + j) + 1] : b[j];
            o[j] = fmaxf(u + v, 0.0f);
        }
        Quad<T>::st(out + 4 * i, o);
    }
}

// g = [mask > 0] (dout + dadd); outa = g * sa; outb = ssb ? g * sb : g (when outb is given)
template <typename T>
__global__ __launch_bounds__(NT) void mask_scale_kernel(const T* __restrict__ dout, const T* __restrict__ dadd, const T* __restrict__ mask,
                                                        const float* __restrict__ ssa, T* __restrict__ outa, const float* __restrict__ ssb,
                                                        T* __restrict__ outb, long long n4, int C) {
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < n4; i += (long long)gridDim.x * NT) {
        const int c = (int)((i * 4) % C);
        const f32x4 m = Quad<T>::ld(mask + 4 * i);
        f32x4 g = {0.0f, 0.0f, 0.0f, 0.0f};
        if (dout) g += Quad<T>::ld(dout + 4 * i);
        if (dadd) g += Quad<T>::ld(dadd + 4 * i);
        f32x4 a, b;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            g[j] = m[j] > 0.0f ? g[j] : 0.0f;
            a[j] = g[j] * ssa[2 * (c + j)];
            b[j] = ssb ? g[j] * ssb[2 * (c + j)] : g[j];
        }
        Quad<T>::st(outa + 4 * i, a);
        if (outb) Quad<T>::st(outb + 4 * i, b);
    }
}

template <typename T>
__global__ __launch_bounds__(NT) void subsample2x_kernel(const T* __restrict__ x, T* __restrict__ y, int N, int H, int W, int C, int Ho, int Wo) {
    constexpr int EPU = 16 / (int)sizeof(T);
    const int upp = C / EPU;
    const long long total = (long long)N * Ho * Wo * upp;
    for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
        const int cu = (int)(i % upp); long long r = i / upp;
        const int wo = (int)(r % Wo); r /= Wo;
        const int ho = (int)(r % Ho); const int n = (int)(r / Ho);
        *reinterpret_cast<u32x4*>(y + (size_t)i * EPU) =
            *reinterpret_cast<const u32x4*>(x + (((size_t)n * H + 2 * ho) * W + 2 * wo) * C + cu * EPU);
    }
}

__device__ __forceinline__ float block_sum(float v, float* red) {     // fixed-order tree over the NT lanes; all threads get the sum
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = NT / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const float out = red[0];
    __syncthreads();
    return out;
}

struct L1Blocks { int blk0[6]; };

template <typename T>
__global__ __launch_bounds__(NT) void l1_partial_kernel(MasFaceFeats f, L1Blocks lb, float* __restrict__ partial) {
    __shared__ float red[NT];
    const int b = blockIdx.x;
    int fi = 0;
    while (fi < 4 && b >= lb.blk0[fi + 1]) ++fi;
    const T* p = reinterpret_cast<const T*>(f.p[fi]);
    const long long n = (long long)f.half * f.chw[fi];
    const long long start = (long long)(b - lb.blk0[fi]) * L1_CHUNK;
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < L1_QUADS; ++k) {
        const long long e = start + 4 * ((long long)k * NT + threadIdx.x);
        if (e < n) {
            const f32x4 a = Quad<T>::ld(p + e), c = Quad<T>::ld(p + n + e);
            s += fabsf(a[0] - c[0]) + fabsf(a[1] - c[1]) + fabsf(a[2] - c[2]) + fabsf(a[3] - c[3]);
        }
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) partial[b] = s;
}

__global__ __launch_bounds__(NT) void l1_final_kernel(MasFaceFeats f, L1Blocks lb, const float* __restrict__ partial, float* __restrict__ out6) {
    __shared__ float red[NT];
    float d[5];
    for (int fi = 0; fi < 5; ++fi) {
        float s = 0.0f;
        for (int i = lb.blk0[fi] + threadIdx.x; i < lb.blk0[fi + 1]; i += NT) s += partial[i];
        d[fi] = f.alpha[fi] * (block_sum(s, red) / (float)f.chw[fi]);
    }
    if (threadIdx.x == 0) {
        float tot = 0.0f;
        for (int fi = 0; fi < 5; ++fi) { out6[fi] = d[fi]; tot += d[fi]; }
        out6[5] = tot;
    }
}

struct SeedPtrs { void* p[5]; };

template <typename T>
__global__ __launch_bounds__(NT) void l1_bwd_kernel(MasFaceFeats f, L1Blocks lb, int row0, int nb, const float* __restrict__ dl6, SeedPtrs seeds) {
    const int b = blockIdx.x;
    int fi = 0;
    while (fi < 4 && b >= lb.blk0[fi + 1]) ++fi;
    const long long chw = f.chw[fi];
    const long long e = 4 * ((long long)(b - lb.blk0[fi]) * NT + threadIdx.x);
    if (e >= (long long)nb * chw) return;
    const T* p = reinterpret_cast<const T*>(f.p[fi]);
    const float coef = (dl6[fi] + dl6[5]) * f.alpha[fi] / (float)chw;
    const f32x4 a = Quad<T>::ld(p + (long long)row0 * chw + e), c = Quad<T>::ld(p + (long long)(row0 - f.half) * chw + e);
    f32x4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = a[j] > c[j] ? coef : (a[j] < c[j] ? -coef : 0.0f);
    Quad<T>::st(reinterpret_cast<T*>(seeds.p[fi]) + e, o);
}

// l1_partial_kernel over PAIRS pairs of capacity (f.half == PAIRS: p0 = rows 0 .. PAIRS - 1, p1 = rows PAIRS .. SLOTS - 1).  The valid pairs
// are a prefix of the element range, and a block's elements are those of l1_partial_kernel's block of the same index for half = n_pairs:
// with the masked lanes adding 0 as its out-of-range lanes do, partial[blk0[fi] + k] holds the same bits for every k it has, and 0 beyond.
template <typename T>
__global__ __launch_bounds__(NT) void l1_partial_dev_kernel(MasFaceFeats f, L1Blocks lb, const FaceSlots* __restrict__ table,
                                                            float* __restrict__ partial) {
    __shared__ float red[NT];
    const int b = blockIdx.x;
    int fi = 0;
    while (fi < 4 && b >= lb.blk0[fi + 1]) ++fi;
    const T* p = reinterpret_cast<const T*>(f.p[fi]);
    const long long chw = f.chw[fi];
    const long long n = (long long)PAIRS * chw;
    const long long start = (long long)(b - lb.blk0[fi]) * L1_CHUNK;
    const unsigned mask = pair_mask(table);
    float s = 0.0f;
#pragma unroll
    for (int k = 0; k < L1_QUADS; ++k) {
        const long long e = start + 4 * ((long long)k * NT + threadIdx.x);
        if (e < n && ((mask >> row_of(e, chw)) & 1u)) {             // (chw is a multiple of 4: a quad never straddles two rows)
            const f32x4 a = Quad<T>::ld(p + e), c = Quad<T>::ld(p + n + e);
            s += fabsf(a[0] - c[0]) + fabsf(a[1] - c[1]) + fabsf(a[2] - c[2]) + fabsf(a[3] - c[3]);
        }
    }
    s = block_sum(s, red);
    if (threadIdx.x == 0) partial[b] = s;
}

// l1_bwd_kernel for slots PAIRS .. SLOTS - 1: every element of the seeds is written, zeros where the pair is invalid or the slot holds a gt row
template <typename T>
__global__ __launch_bounds__(NT) void l1_bwd_dev_kernel(MasFaceFeats f, L1Blocks lb, const FaceSlots* __restrict__ table,
                                                        const float* __restrict__ dl6, SeedPtrs seeds) {
    const int b = blockIdx.x;
    int fi = 0;
    while (fi < 4 && b >= lb.blk0[fi + 1]) ++fi;
    const long long chw = f.chw[fi];
    const long long n = (long long)PAIRS * chw;
    const long long e = 4 * ((long long)(b - lb.blk0[fi]) * NT + threadIdx.x);
    if (e >= n) return;
    const int q = row_of(e, chw);
    f32x4 o = {0.0f, 0.0f, 0.0f, 0.0f};
    if (((pair_mask(table) >> q) & 1u) && table->row[PAIRS + q].src == 1) {
        const T* p = reinterpret_cast<const T*>(f.p[fi]);
        const float coef = (dl6[fi] + dl6[5]) * f.alpha[fi] / (float)chw;
        const f32x4 a = Quad<T>::ld(p + n + e), c = Quad<T>::ld(p + e);
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = a[j] > c[j] ? coef : (a[j] < c[j] ? -coef : 0.0f);
    }
    Quad<T>::st(reinterpret_cast<T*>(seeds.p[fi]) + e, o);
}

int ew_grid(long long n4) {
    long long g = (n4 + NT - 1) / NT;
    const long long cap = 8LL * mas_num_cus();
    return (int)(g > cap ? cap : (g < 1 ? 1 : g));
}

bool dtype_ok(int dt) { return dt == MAS_F32 || dt == MAS_BF16; }

int check_image(const MasFaceImage* im, const char* what) {
    if (!im || !im->data) MAS_FAIL(MAS_EINVAL, "%s: null image", what);
    if (!dtype_ok(im->dtype)) MAS_FAIL(MAS_EINVAL, "%s: dtype %d", what, im->dtype);
    if (im->C != 3 || im->N <= 0 || im->H <= 0 || im->W <= 0) MAS_FAIL(MAS_EINVAL, "%s: need [N>0, 3, H>0, W>0], got C=%d", what, im->C);
    return MAS_OK;
}

int check_rows(const MasFaceRow* rows, int n_rows, const char* what, const MasFaceImage* img, const MasFaceImage* rec) {
    if (!rows) MAS_FAIL(MAS_EINVAL, "%s: null row table", what);
    if (n_rows <= 0 || n_rows > MAS_FACE_MAX_ROWS) MAS_FAIL(MAS_EINVAL, "%s: %d rows (1..%d)", what, n_rows, MAS_FACE_MAX_ROWS);
    for (int i = 0; i < n_rows; ++i) {
        const MasFaceRow& r = rows[i];
        const MasFaceImage* im = r.src ? rec : img;
        if (r.h <= 0 || r.w <= 0 || r.rh < FS || r.rw < FS || r.ct < 0 || r.cl < 0 || r.ct + FS > r.rh || r.cl + FS > r.rw || r.b < 0 ||
            (im && r.b >= im->N) || (r.src != 0 && r.src != 1))
            MAS_FAIL(MAS_EINVAL, "%s: row %d has an invalid geometry", what, i);
    }
    return MAS_OK;
}

int check_feats(const MasFaceFeats* f, const char* what) {
    if (!f) MAS_FAIL(MAS_EINVAL, "%s: null feature table", what);
    if (!dtype_ok(f->dtype)) MAS_FAIL(MAS_EINVAL, "%s: dtype %d", what, f->dtype);
    if (f->half <= 0) MAS_FAIL(MAS_EINVAL, "%s: half = %d", what, f->half);
    for (int i = 0; i < 5; ++i) {
        if (!f->p[i]) MAS_FAIL(MAS_EINVAL, "%s: null feature %d", what, i);
        if (f->chw[i] <= 0 || f->chw[i] % 4) MAS_FAIL(MAS_EINVAL, "%s: feature %d has %d elements per row (a positive multiple of 4)", what, i, f->chw[i]);
    }
    return MAS_OK;
}

L1Blocks l1_blocks(const MasFaceFeats* f, long long rows, int per_block) {
    L1Blocks lb;
    lb.blk0[0] = 0;
    for (int i = 0; i < 5; ++i) lb.blk0[i + 1] = lb.blk0[i] + (int)((rows * f->chw[i] + per_block - 1) / per_block);
    return lb;
}

}  // namespace

extern "C" int mas_face_crop_fwd(const MasFaceImage* img, const MasFaceImage* rec, const MasFaceRow* rows, int n_rows, void* out, int out_dtype,
                                 void* stream) {
    MAS_ENTER();
    if (int rc = check_image(img, "face_crop_fwd")) return rc;
    if (int rc = check_image(rec, "face_crop_fwd")) return rc;
    if (!out) MAS_FAIL(MAS_EINVAL, "face_crop_fwd: null output");
    if (!dtype_ok(out_dtype)) MAS_FAIL(MAS_EINVAL, "face_crop_fwd: dtype %d", out_dtype);
    if (int rc = check_rows(rows, n_rows, "face_crop_fwd", img, rec)) return rc;
    RowTable t;
    memset(&t, 0, sizeof(t));
    memcpy(t.r, rows, sizeof(MasFaceRow) * n_rows);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(mas_cdiv(FS * FS, NT), n_rows);
    if (out_dtype == MAS_F32) hipLaunchKernelGGL(crop_fwd_kernel<float>, grid, dim3(NT), 0, s, *img, *rec, t, (float*)out);
    else hipLaunchKernelGGL(crop_fwd_kernel<bf16_t>, grid, dim3(NT), 0, s, *img, *rec, t, (bf16_t*)out);
    MAS_CHECK_LAUNCH("face_crop_fwd");
    return MAS_OK;
}

extern "C" int mas_face_crop_bwd(const float* dfaces, const MasFaceRow* rows, int n_rows, const MasFaceImage* drec, void* stream) {
    MAS_ENTER();
    if (!dfaces) MAS_FAIL(MAS_EINVAL, "face_crop_bwd: null gradient");
    if (int rc = check_image(drec, "face_crop_bwd")) return rc;
    if (int rc = check_rows(rows, n_rows, "face_crop_bwd", drec, drec)) return rc;
    RowTable t;
    memset(&t, 0, sizeof(t));
    memcpy(t.r, rows, sizeof(MasFaceRow) * n_rows);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long long px = (long long)drec->N * drec->H * drec->W;
    const dim3 grid((unsigned)((px + NT - 1) / NT));
    if (drec->dtype == MAS_F32) hipLaunchKernelGGL(crop_bwd_kernel<float>, grid, dim3(NT), 0, s, dfaces, t, n_rows, *drec);
    else hipLaunchKernelGGL(crop_bwd_kernel<bf16_t>, grid, dim3(NT), 0, s, dfaces, t, n_rows, *drec);
    MAS_CHECK_LAUNCH("face_crop_bwd");
    return MAS_OK;
}

extern "C" int mas_face_stem_fwd(const void* x, const float* w, void* y, int dtype, int R, void* stream) {
    MAS_ENTER();
    if (!x || !w || !y) MAS_FAIL(MAS_EINVAL, "face_stem_fwd: null argument");
    if (!dtype_ok(dtype) || R <= 0) MAS_FAIL(MAS_EINVAL, "face_stem_fwd: dtype %d, R %d", dtype, R);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(mas_cdiv(STEM_O * STEM_O, NT), R);
    if (dtype == MAS_F32) hipLaunchKernelGGL(stem_fwd_kernel<float>, grid, dim3(NT), 0, s, (const float*)x, w, (float*)y);
    else hipLaunchKernelGGL(stem_fwd_kernel<bf16_t>, grid, dim3(NT), 0, s, (const bf16_t*)x, w, (bf16_t*)y);
    MAS_CHECK_LAUNCH("face_stem_fwd");
    return MAS_OK;
}

extern "C" int mas_face_stem_dgrad(const void* dy, const float* w, float* dx, int dtype, int R, void* stream) {
    MAS_ENTER();
    if (!dy || !w || !dx) MAS_FAIL(MAS_EINVAL, "face_stem_dgrad: null argument");
    if (!dtype_ok(dtype) || R <= 0) MAS_FAIL(MAS_EINVAL, "face_stem_dgrad: dtype %d, R %d", dtype, R);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(mas_cdiv(FS * FS, NT), R);
    if (dtype == MAS_F32) hipLaunchKernelGGL(stem_dgrad_kernel<float>, grid, dim3(NT), 0, s, (const float*)dy, w, dx);
    else hipLaunchKernelGGL(stem_dgrad_kernel<bf16_t>, grid, dim3(NT), 0, s, (const bf16_t*)dy, w, dx);
    MAS_CHECK_LAUNCH("face_stem_dgrad");
    return MAS_OK;
}

extern "C" int mas_face_bn_fold(const MasFaceBnItem* items, int n_items, float* scale_shift, void* stream) {
    MAS_ENTER();
    if (!items || !scale_shift) MAS_FAIL(MAS_EINVAL, "face_bn_fold: null argument");
    if (n_items <= 0) MAS_FAIL(MAS_EINVAL, "face_bn_fold: %d items", n_items);
    hipLaunchKernelGGL(bn_fold_kernel, dim3(n_items), dim3(NT), 0, reinterpret_cast<hipStream_t>(stream), items, scale_shift);
    MAS_CHECK_LAUNCH("face_bn_fold");
    return MAS_OK;
}

extern "C" int mas_face_pool_fwd(const void* y, const float* scale_shift, void* z, unsigned char* idx, int dtype, int R, int H, int W, int C,
                                 void* stream) {
    MAS_ENTER();
    if (!y || !scale_shift || !z || !idx) MAS_FAIL(MAS_EINVAL, "face_pool_fwd: null argument");
    if (!dtype_ok(dtype) || R <= 0 || H < 3 || W < 3 || C <= 0 || C % 4) MAS_FAIL(MAS_EINVAL, "face_pool_fwd: bad shape or dtype");
    const int Ho = pool_out(H), Wo = pool_out(W);
    const long long total = (long long)R * Ho * Wo * (C / 4);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((total + NT - 1) / NT));
    if (dtype == MAS_F32)
        hipLaunchKernelGGL(pool_fwd_kernel<float>, grid, dim3(NT), 0, s, (const float*)y, scale_shift, (float*)z, (unsigned*)idx, R, H, W, C, Ho, Wo);
    else
        hipLaunchKernelGGL(pool_fwd_kernel<bf16_t>, grid, dim3(NT), 0, s, (const bf16_t*)y, scale_shift, (bf16_t*)z, (unsigned*)idx, R, H, W, C, Ho, Wo);
    MAS_CHECK_LAUNCH("face_pool_fwd");
    return MAS_OK;
}

extern "C" int mas_face_pool_bwd(const void* y, const float* scale_shift, const void* dz, const unsigned char* idx, const void* seed, void* dy,
                                 int dtype, int R, int H, int W, int C, void* stream) {
    MAS_ENTER();
    if (!y || !scale_shift || !dz || !idx || !dy) MAS_FAIL(MAS_EINVAL, "face_pool_bwd: null argument");
    if (!dtype_ok(dtype) || R <= 0 || H < 3 || W < 3 || C <= 0 || C % 4) MAS_FAIL(MAS_EINVAL, "face_pool_bwd: bad shape or dtype");
    const int Ho = pool_out(H), Wo = pool_out(W);
    const long long total = (long long)R * H * W * (C / 4);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((total + NT - 1) / NT));
    if (dtype == MAS_F32)
        hipLaunchKernelGGL(pool_bwd_kernel<float>, grid, dim3(NT), 0, s, (const float*)y, scale_shift, (const float*)dz, (const unsigned*)idx,
                           (const float*)seed, (float*)dy, R, H, W, C, Ho, Wo);
    else
        hipLaunchKernelGGL(pool_bwd_kernel<bf16_t>, grid, dim3(NT), 0, s, (const bf16_t*)y, scale_shift, (const bf16_t*)dz, (const unsigned*)idx,
                           (const bf16_t*)seed, (bf16_t*)dy, R, H, W, C, Ho, Wo);
    MAS_CHECK_LAUNCH("face_pool_bwd");
    return MAS_OK;
}

extern "C" int mas_face_join_fwd(const void* y3, const float* ss3, const void* r, const float* ssr, void* out, int dtype, int M, int C, void* stream) {
    MAS_ENTER();
    if (!y3 || !ss3 || !r || !out) MAS_FAIL(MAS_EINVAL, "face_join_fwd: null argument");
    if (!dtype_ok(dtype) || M <= 0 || C <= 0 || C % 4) MAS_FAIL(MAS_EINVAL, "face_join_fwd: bad shape or dtype");
    const long long n4 = (long long)M * C / 4;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == MAS_F32)
        hipLaunchKernelGGL(join_fwd_kernel<float>, dim3(ew_grid(n4)), dim3(NT), 0, s, (const float*)y3, ss3, (const float*)r, ssr, (float*)out, n4, C);
    else
        hipLaunchKernelGGL(join_fwd_kernel<bf16_t>, dim3(ew_grid(n4)), dim3(NT), 0, s, (const bf16_t*)y3, ss3, (const bf16_t*)r, ssr, (bf16_t*)out, n4, C);
    MAS_CHECK_LAUNCH("face_join_fwd");
    return MAS_OK;
}

static int mask_scale(const char* name, const void* dout, const void* dadd, const void* mask, const float* ssa, void* outa, const float* ssb,
                      void* outb, int dtype, int M, int C, void* stream) {
    if (!mask || !ssa || !outa) MAS_FAIL(MAS_EINVAL, "%s: null argument", name);
    if (!dtype_ok(dtype) || M <= 0 || C <= 0 || C % 4) MAS_FAIL(MAS_EINVAL, "%s: bad shape or dtype", name);
    const long long n4 = (long long)M * C / 4;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == MAS_F32)
        hipLaunchKernelGGL(mask_scale_kernel<float>, dim3(ew_grid(n4)), dim3(NT), 0, s, (const float*)dout, (const float*)dadd, (const float*)mask,
                           ssa, (float*)outa, ssb, (float*)outb, n4, C);
    else
        hipLaunchKernelGGL(mask_scale_kernel<bf16_t>, dim3(ew_grid(n4)), dim3(NT), 0, s, (const bf16_t*)dout, (const bf16_t*)dadd,
                           (const bf16_t*)mask, ssa, (bf16_t*)outa, ssb, (bf16_t*)outb, n4, C);
    MAS_CHECK_LAUNCH(name);
    return MAS_OK;
}

extern "C" int mas_face_join_bwd(const void* dout, const void* dadd, const void* out, const float* ss3, const float* ssr, void* dy3, void* dres,
                                 int dtype, int M, int C, void* stream) {
    MAS_ENTER();
    if (!dres) MAS_FAIL(MAS_EINVAL, "face_join_bwd: null argument");
    return mask_scale("face_join_bwd", dout, dadd, out, ss3, dy3, ssr, dres, dtype, M, C, stream);
}

extern "C" int mas_face_relu_bn_bwd(const void* da, const void* a, const float* scale_shift, void* dy, int dtype, int M, int C, void* stream) {
    MAS_ENTER();
    if (!da) MAS_FAIL(MAS_EINVAL, "face_relu_bn_bwd: null argument");
    return mask_scale("face_relu_bn_bwd", da, nullptr, a, scale_shift, dy, nullptr, nullptr, dtype, M, C, stream);
}

extern "C" int mas_face_subsample2x(const void* x, void* y, int dtype, int N, int H, int W, int C, void* stream) {
    MAS_ENTER();
    if (!x || !y) MAS_FAIL(MAS_EINVAL, "face_subsample2x: null argument");
    if (!dtype_ok(dtype) || N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % (dtype == MAS_BF16 ? 8 : 4))
        MAS_FAIL(MAS_EINVAL, "face_subsample2x: bad shape or dtype");
    const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
    const long long total = (long long)N * Ho * Wo * C / (dtype == MAS_BF16 ? 8 : 4);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == MAS_F32)
        hipLaunchKernelGGL(subsample2x_kernel<float>, dim3(ew_grid(total)), dim3(NT), 0, s, (const float*)x, (float*)y, N, H, W, C, Ho, Wo);
    else
        hipLaunchKernelGGL(subsample2x_kernel<bf16_t>, dim3(ew_grid(total)), dim3(NT), 0, s, (const bf16_t*)x, (bf16_t*)y, N, H, W, C, Ho, Wo);
    MAS_CHECK_LAUNCH("face_subsample2x");
    return MAS_OK;
}

extern "C" int mas_face_l1_workspace(const MasFaceFeats* f) {
    MAS_ENTER();
    if (int rc = check_feats(f, "face_l1_workspace")) return rc;
    return l1_blocks(f, f->half, L1_CHUNK).blk0[5];
}

extern "C" int mas_face_l1_fwd(const MasFaceFeats* f, float* workspace, float* out6, void* stream) {
    MAS_ENTER();
    if (int rc = check_feats(f, "face_l1_fwd")) return rc;
    if (!workspace || !out6) MAS_FAIL(MAS_EINVAL, "face_l1_fwd: null argument");
    const L1Blocks lb = l1_blocks(f, f->half, L1_CHUNK);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (f->dtype == MAS_F32) hipLaunchKernelGGL(l1_partial_kernel<float>, dim3(lb.blk0[5]), dim3(NT), 0, s, *f, lb, workspace);
    else hipLaunchKernelGGL(l1_partial_kernel<bf16_t>, dim3(lb.blk0[5]), dim3(NT), 0, s, *f, lb, workspace);
    MAS_CHECK_LAUNCH("face_l1_partial");
    hipLaunchKernelGGL(l1_final_kernel, dim3(1), dim3(NT), 0, s, *f, lb, (const float*)workspace, out6);
    MAS_CHECK_LAUNCH("face_l1_final");
    return MAS_OK;
}

extern "C" int mas_face_l1_bwd(const MasFaceFeats* f, int row0, int nb, const float* dl6, void* const* seeds, void* stream) {
    MAS_ENTER();
    if (int rc = check_feats(f, "face_l1_bwd")) return rc;
    if (!dl6 || !seeds) MAS_FAIL(MAS_EINVAL, "face_l1_bwd: null argument");
    if (nb <= 0 || row0 < f->half || row0 + nb > 2 * f->half) MAS_FAIL(MAS_EINVAL, "face_l1_bwd: rows [%d, %d) outside the second half", row0, row0 + nb);
    SeedPtrs sp;
    for (int i = 0; i < 5; ++i) {
        if (!seeds[i]) MAS_FAIL(MAS_EINVAL, "face_l1_bwd: null seed %d", i);
        sp.p[i] = seeds[i];
    }
    const L1Blocks lb = l1_blocks(f, nb, 4 * NT);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (f->dtype == MAS_F32) hipLaunchKernelGGL(l1_bwd_kernel<float>, dim3(lb.blk0[5]), dim3(NT), 0, s, *f, lb, row0, nb, dl6, sp);
    else hipLaunchKernelGGL(l1_bwd_kernel<bf16_t>, dim3(lb.blk0[5]), dim3(NT), 0, s, *f, lb, row0, nb, dl6, sp);
    MAS_CHECK_LAUNCH("face_l1_bwd");
    return MAS_OK;
}

// ---- the four passes on a device table of MAS_FACE_SLOTS slots (include/mas_hip.h): nothing below depends on the table's contents
static const FaceSlots* slots_of(const int32_t* table_dev) { return reinterpret_cast<const FaceSlots*>(table_dev); }

extern "C" int mas_face_crop_fwd_dev(const MasFaceImage* img, const MasFaceImage* rec, const int32_t* table_dev, void* out, int out_dtype,
                                     void* stream) {
    MAS_ENTER();
    if (int rc = check_image(img, "face_crop_fwd_dev")) return rc;
    if (int rc = check_image(rec, "face_crop_fwd_dev")) return rc;
    if (!table_dev || !out) MAS_FAIL(MAS_EINVAL, "face_crop_fwd_dev: null table or output");
    if (!dtype_ok(out_dtype)) MAS_FAIL(MAS_EINVAL, "face_crop_fwd_dev: dtype %d", out_dtype);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(mas_cdiv(FS * FS, NT), SLOTS);
    if (out_dtype == MAS_F32) hipLaunchKernelGGL(crop_fwd_dev_kernel<float>, grid, dim3(NT), 0, s, *img, *rec, slots_of(table_dev), (float*)out);
    else hipLaunchKernelGGL(crop_fwd_dev_kernel<bf16_t>, grid, dim3(NT), 0, s, *img, *rec, slots_of(table_dev), (bf16_t*)out);
    MAS_CHECK_LAUNCH("face_crop_fwd_dev");
    return MAS_OK;
}

extern "C" int mas_face_crop_bwd_dev(const float* dfaces, const int32_t* table_dev, const MasFaceImage* drec, void* stream) {
    MAS_ENTER();
    if (!dfaces || !table_dev) MAS_FAIL(MAS_EINVAL, "face_crop_bwd_dev: null gradient or table");
    if (int rc = check_image(drec, "face_crop_bwd_dev")) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const long long px = (long long)drec->N * drec->H * drec->W;
    const dim3 grid((unsigned)((px + NT - 1) / NT));
    if (drec->dtype == MAS_F32) hipLaunchKernelGGL(crop_bwd_dev_kernel<float>, grid, dim3(NT), 0, s, dfaces, slots_of(table_dev), *drec);
    else hipLaunchKernelGGL(crop_bwd_dev_kernel<bf16_t>, grid, dim3(NT), 0, s, dfaces, slots_of(table_dev), *drec);
    MAS_CHECK_LAUNCH("face_crop_bwd_dev");
    return MAS_OK;
}

static int check_feats_dev(const MasFaceFeats* f, const char* what) {
    if (int rc = check_feats(f, what)) return rc;
    if (f->half != PAIRS) MAS_FAIL(MAS_EINVAL, "%s: half = %d (the table's capacity is %d pairs)", what, f->half, PAIRS);
    return MAS_OK;
}

extern "C" int mas_face_l1_fwd_dev(const MasFaceFeats* f, const int32_t* table_dev, float* workspace, float* out6, void* stream) {
    MAS_ENTER();
    if (int rc = check_feats_dev(f, "face_l1_fwd_dev")) return rc;
    if (!table_dev || !workspace || !out6) MAS_FAIL(MAS_EINVAL, "face_l1_fwd_dev: null argument");
    const L1Blocks lb = l1_blocks(f, PAIRS, L1_CHUNK);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (f->dtype == MAS_F32) hipLaunchKernelGGL(l1_partial_dev_kernel<float>, dim3(lb.blk0[5]), dim3(NT), 0, s, *f, lb, slots_of(table_dev), workspace);
    else hipLaunchKernelGGL(l1_partial_dev_kernel<bf16_t>, dim3(lb.blk0[5]), dim3(NT), 0, s, *f, lb, slots_of(table_dev), workspace);
    MAS_CHECK_LAUNCH("face_l1_partial_dev");
    hipLaunchKernelGGL(l1_final_kernel, dim3(1), dim3(NT), 0, s, *f, lb, (const float*)workspace, out6);
    MAS_CHECK_LAUNCH("face_l1_final");
    return MAS_OK;
}

extern "C" int mas_face_l1_bwd_dev(const MasFaceFeats* f, const int32_t* table_dev, const float* dl6, void* const* seeds, void* stream) {
    MAS_ENTER();
    if (int rc = check_feats_dev(f, "face_l1_bwd_dev")) return rc;
    if (!table_dev || !dl6 || !seeds) MAS_FAIL(MAS_EINVAL, "face_l1_bwd_dev: null argument");
    SeedPtrs sp;
    for (int i = 0; i < 5; ++i) {
        if (!seeds[i]) MAS_FAIL(MAS_EINVAL, "face_l1_bwd_dev: null seed %d", i);
        sp.p[i] = seeds[i];
    }
    const L1Blocks lb = l1_blocks(f, PAIRS, 4 * NT);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (f->dtype == MAS_F32) hipLaunchKernelGGL(l1_bwd_dev_kernel<float>, dim3(lb.blk0[5]), dim3(NT), 0, s, *f, lb, slots_of(table_dev), dl6, sp);
    else hipLaunchKernelGGL(l1_bwd_dev_kernel<bf16_t>, dim3(lb.blk0[5]), dim3(NT), 0, s, *f, lb, slots_of(table_dev), dl6, sp);
    MAS_CHECK_LAUNCH("face_l1_bwd_dev");
    return MAS_OK;
}
