// Multi-tensor Adam for gfx950: ONE launch updates every parameter of a model (reference train.py:99-103: torch.optim.Adam on the
// VQ model's ~400 parameters, 95 M fp32 elements).  The step is a stream of 7 fp32 passes (read p, g, m, v; write p, m, v = 28 bytes per
// element, 2.67 GB for VQ-IMG: 0.42 ms at 6.3 TB/s); torch's fused multi-tensor path takes 10 launches and 0.75 ms for it
// (profiles/r04_kernel_trace_vq_final.txt).  A block owns 4096 consecutive elements of one tensor; the (tensor, offset) of a block comes
// from a table in device memory (binary search over first_block, as in misc.hip's tiled pack), so tiny tensors (biases, norm
// weights) cost one block each and no launch of their own.
// Arithmetic and its ORDER follow torch's fused kernel (torch/csrc ... FusedAdamMathFunctor, non-amsgrad, maximize = false):
//   g' = g + wd * p;  m = b1 m + (1 - b1) g';  v = b2 v + (1 - b2) g' g';  p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)
// with bc1 = 1 - b1^t, bc2 = 1 - b2^t computed by the caller in double precision.
// mas_adam_multi_ema keeps an exponential moving average of the weights in the same launch: e += (1 - decay) (p_new - e), one more read and
// one more write of 4 bytes per element (36 bytes: 3.43 GB for VQ-IMG, 0.54 ms at 6.3 TB/s; as a pass of its own after the step it is 40
// bytes and a launch per tensor), and returns before its first store when the gradient norm it is handed is not finite.
// mas_swap_multi exchanges p with another tensor per item over the same table (the EMA weights in front of the kernels, and back).
#include "mas_common.h"
#include "../../include/mas_hip.h"
#include <math.h>

namespace {

constexpr int ADAM_NT = 256, ADAM_PER_BLOCK = 4096;     // 4 x float4 per thread and tensor

// the index of the item that owns work-group b (items in ascending first_block order); the EMA instantiations and the swap look their
// second table up with it
__device__ __forceinline__ int item_index_of_block(const MasAdamItem* __restrict__ items, int n_items, int b) {
    int lo = 0, hi = n_items - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (items[mid].first_block <= b) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ MasAdamItem item_of_block(const MasAdamItem* __restrict__ items, int n_items, int b) {
    return items[item_index_of_block(items, n_items, b)];
}

// NaN or +-inf, from the bits (holds under any floating-point option the file is built with)
__device__ __forceinline__ bool not_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }

// SCALE: every gradient is multiplied by *grad_scale as it is loaded (the clip coefficient of mas_grad_clip_coef; g itself is not written).
// DECOUPLED: AdamW -- p -= lr wd p ahead of the moments, no wd p term in g (torch's fused functor in its ADAMW mode).
// <false, false, false> is the plain Adam step: neither `grad_scale` nor `lr` is read.
// EMA: the instantiations behind mas_adam_multi_ema; without it the three trailing arguments are not read and the code is what it was.
//   guard: `grad_norm` non-null and *grad_norm NaN or +-inf (one uniform read per work-group): return before anything is stored.
//   average: ema[i] non-null (`ema` itself may be null): e = fma(ema_w, p_new - e, e) after the update of an element, ema_w = 1 - decay; e is
//   loaded with p, g, m, v and stored with p, m, v.  Five 4 x float4 arrays are 80 data registers: 120 / 122 VGPRs and four waves per SIMD
//   (the other instantiations: 94 and five).  EMA_GROUPS = 2 (two halves of 2 x float4 per tensor) is 96 VGPRs and five waves with half
//   the loads in flight per lane.
// DEV: the instantiations behind mas_adam_multi_dev (always with EMA).  step_size, sqrt(bc2), lr and ema_w come from item idx's record of
//   four floats in `dev` (written by adam_dev_scalars_kernel in front of this launch) instead of the arguments: one uniform 16-byte load per
//   work-group.  Everything below that load is the code of the other instantiations.
constexpr int EMA_GROUPS = 4;
template <bool SCALE, bool DECOUPLED, bool EMA, bool DEV = false>
__global__ __launch_bounds__(ADAM_NT) void adam_multi_kernel(const MasAdamItem* __restrict__ items, int n_items, float step_size, float inv_bc2_sqrt,
                                                             float b1, float b2, float eps, float wd,     // (inv_bc2_sqrt: sqrt(bias_correction2) itself)
                                                             const float* __restrict__ grad_scale, float lr, float* const* __restrict__ ema,
                                                             float ema_w, const float* __restrict__ grad_norm, const float* __restrict__ dev) {
    const int b = blockIdx.x;
    if constexpr (EMA) {
        if (grad_norm != nullptr && not_finite(*grad_norm)) return;
    }
    const int idx = item_index_of_block(items, n_items, b);
    const MasAdamItem it = items[idx];
    const long long base = (long long)(b - it.first_block) * ADAM_PER_BLOCK;
    if constexpr (DEV) {
        const f32x4 s = *reinterpret_cast<const f32x4*>(dev + 4 * (long long)idx);
        step_size = s[0]; inv_bc2_sqrt = s[1]; lr = s[2]; ema_w = s[3];
    }
    const float omb1 = 1.0f - b1, omb2 = 1.0f - b2;
    float gs = 1.0f;
    if constexpr (SCALE) gs = *grad_scale;
    auto upd = [&](float& p, float g, float& m, float& v) {
        if constexpr (SCALE) g *= gs;
        if constexpr (DECOUPLED) { if (wd != 0.0f) p -= lr * wd * p; }
        else if (wd != 0.0f) g += p * wd;
        m = fmaf(omb1, g - m, m);                    // torch: lerp(exp_avg, grad, 1 - beta1)
        v = b2 * v + omb2 * g * g;
        const float denom = sqrtf(v) / inv_bc2_sqrt + eps;
        p -= step_size * m / denom;
    };
    const bool vec = ((reinterpret_cast<uintptr_t>(it.p) | reinterpret_cast<uintptr_t>(it.g) | reinterpret_cast<uintptr_t>(it.m) |
                       reinterpret_cast<uintptr_t>(it.v)) & 15) == 0;
    if constexpr (EMA) {
        float* const ema_t = ema != nullptr ? ema[idx] : nullptr;
        if (ema_t != nullptr) {
            if (vec && (reinterpret_cast<uintptr_t>(ema_t) & 15) == 0 && base + ADAM_PER_BLOCK <= it.n) {
                for (int h = 0; h < 4; h += EMA_GROUPS) {
                    f32x4 p[EMA_GROUPS], g[EMA_GROUPS], m[EMA_GROUPS], v[EMA_GROUPS], a[EMA_GROUPS];
#pragma unroll
                    for (int k = 0; k < EMA_GROUPS; ++k) {
                        const long long i = base + (long long)((h + k) * ADAM_NT + threadIdx.x) * 4;
                        p[k] = *reinterpret_cast<const f32x4*>(it.p + i); g[k] = *reinterpret_cast<const f32x4*>(it.g + i);
                        m[k] = *reinterpret_cast<const f32x4*>(it.m + i); v[k] = *reinterpret_cast<const f32x4*>(it.v + i);
                        a[k] = *reinterpret_cast<const f32x4*>(ema_t + i);
                    }
#pragma unroll
                    for (int k = 0; k < EMA_GROUPS; ++k) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) {
                            float pp = p[k][e], mm = m[k][e], vv = v[k][e];
                            upd(pp, g[k][e], mm, vv);
                            p[k][e] = pp; m[k][e] = mm; v[k][e] = vv; a[k][e] = fmaf(ema_w, pp - a[k][e], a[k][e]);
                        }
                        const long long i = base + (long long)((h + k) * ADAM_NT + threadIdx.x) * 4;
                        *reinterpret_cast<f32x4*>(it.p + i) = p[k]; *reinterpret_cast<f32x4*>(it.m + i) = m[k];
                        *reinterpret_cast<f32x4*>(it.v + i) = v[k]; *reinterpret_cast<f32x4*>(ema_t + i) = a[k];
                    }
                }
            } else {                                 // a tensor's last block, or unaligned storage: element by element
                for (int k = threadIdx.x; k < ADAM_PER_BLOCK; k += ADAM_NT) {
                    const long long i = base + k;
                    if (i < it.n) {
                        float pp = it.p[i], mm = it.m[i], vv = it.v[i];
                        const float aa = ema_t[i];
                        upd(pp, it.g[i], mm, vv);
                        it.p[i] = pp; it.m[i] = mm; it.v[i] = vv; ema_t[i] = fmaf(ema_w, pp - aa, aa);
                    }
                }
            }
            return;
        }
    }
    if (vec && base + ADAM_PER_BLOCK <= it.n) {
        f32x4 p[4], g[4], m[4], v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long i = base + (long long)(k * ADAM_NT + threadIdx.x) * 4;
            p[k] = *reinterpret_cast<const f32x4*>(it.p + i); g[k] = *reinterpret_cast<const f32x4*>(it.g + i);
            m[k] = *reinterpret_cast<const f32x4*>(it.m + i); v[k] = *reinterpret_cast<const f32x4*>(it.v + i);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { float pp = p[k][e], mm = m[k][e], vv = v[k][e]; upd(pp, g[k][e], mm, vv); p[k][e] = pp; m[k][e] = mm; v[k][e] = vv; }
            const long long i = base + (long long)(k * ADAM_NT + threadIdx.x) * 4;
            *reinterpret_cast<f32x4*>(it.p + i) = p[k]; *reinterpret_cast<f32x4*>(it.m + i) = m[k]; *reinterpret_cast<f32x4*>(it.v + i) = v[k];
        }
    } else {                                         // a tensor's last block, or unaligned storage: element by element
        for (int k = threadIdx.x; k < ADAM_PER_BLOCK; k += ADAM_NT) {
            const long long i = base + k;
            if (i < it.n) { float pp = it.p[i], mm = it.m[i], vv = it.v[i]; upd(pp, it.g[i], mm, vv); it.p[i] = pp; it.m[i] = mm; it.v[i] = vv; }
        }
    }
}

// ---- global-norm gradient clipping over the same table -----------------------------------------------------------------------------
// sum of the 256 lanes' fp64 values, valid in thread 0: wave shuffles (offsets 32 ... 1), then the four wave sums through LDS in wave order.
// The order is fixed, so the same data gives the same bits on every call.
__device__ __forceinline__ double block_sum_f64(double a) {
    __shared__ double wsum[ADAM_NT / 64];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a += __shfl_down(a, off, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = a;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 0; w < ADAM_NT / 64; ++w) t += wsum[w];
    }
    return t;
}

// partials[b] = sum of g^2 over block b's elements, squared and added in fp64 from the first addition (the square of an fp32 value is exact
// in fp64; gradients of 1e20 or 1e-30 neither overflow nor vanish).  One store per work-group, no atomics, nothing between work-groups.
__global__ __launch_bounds__(ADAM_NT) void grad_sqnorm_multi_kernel(const MasAdamItem* __restrict__ items, int n_items, double* __restrict__ partials) {
    const int b = blockIdx.x;
    const MasAdamItem it = item_of_block(items, n_items, b);
    const long long base = (long long)(b - it.first_block) * ADAM_PER_BLOCK;
    double acc = 0.0;
    if ((reinterpret_cast<uintptr_t>(it.g) & 15) == 0 && base + ADAM_PER_BLOCK <= it.n) {
        f32x4 g[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) g[k] = *reinterpret_cast<const f32x4*>(it.g + base + (long long)(k * ADAM_NT + threadIdx.x) * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { const double d = (double)g[k][e]; acc += d * d; }
        }
    } else {                                         // a tensor's last block, or unaligned storage: element by element
        for (int k = threadIdx.x; k < ADAM_PER_BLOCK; k += ADAM_NT) {
            const long long i = base + k;
            if (i < it.n) { const double d = (double)it.g[i]; acc += d * d; }
        }
    }
    acc = block_sum_f64(acc);
    if (threadIdx.x == 0) partials[b] = acc;
}

// One work-group: thread t adds partials[t], partials[t + 256], ... and then extra[t], extra[t + 256], ... in fp64; block sum; then
// out[0] = (float)sqrt(sum), out[1] = min(max_norm / (out[0] + 1e-6f), 1) in fp32 -- torch.nn.utils.clip_grad_norm_'s coefficient.
// The clamp is a comparison that a NaN fails, so a NaN norm gives a NaN coefficient (fminf would return 1).
__global__ __launch_bounds__(ADAM_NT) void grad_clip_coef_kernel(const double* __restrict__ partials, int n_partials, const double* __restrict__ extra,
                                                                 int n_extra, float max_norm, float* __restrict__ out) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < n_partials; i += ADAM_NT) acc += partials[i];
    for (int i = threadIdx.x; i < n_extra; i += ADAM_NT) acc += extra[i];
    acc = block_sum_f64(acc);
    if (threadIdx.x == 0) {
        const float norm = (float)sqrt(acc);
        const float c = max_norm / (norm + 1e-6f);
        out[0] = norm;
        out[1] = c > 1.0f ? 1.0f : c;
    }
}

// g *= *scale in place (the standalone clip_grad_norm_: the caller's optimizer reads the gradients afterwards)
__global__ __launch_bounds__(ADAM_NT) void grad_scale_multi_kernel(const MasAdamItem* __restrict__ items, int n_items, const float* __restrict__ scale) {
    const int b = blockIdx.x;
    const MasAdamItem it = item_of_block(items, n_items, b);
    const long long base = (long long)(b - it.first_block) * ADAM_PER_BLOCK;
    float* g = const_cast<float*>(it.g);
    const float s = *scale;
    if ((reinterpret_cast<uintptr_t>(g) & 15) == 0 && base + ADAM_PER_BLOCK <= it.n) {
        f32x4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = *reinterpret_cast<const f32x4*>(g + base + (long long)(k * ADAM_NT + threadIdx.x) * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) *reinterpret_cast<f32x4*>(g + base + (long long)(k * ADAM_NT + threadIdx.x) * 4) = v[k] * s;
    } else {
        for (int k = threadIdx.x; k < ADAM_PER_BLOCK; k += ADAM_NT) {
            const long long i = base + k;
            if (i < it.n) g[i] *= s;
        }
    }
}

// p <-> other[i], element for element, for every item whose `other` entry is not null
__global__ __launch_bounds__(ADAM_NT) void swap_multi_kernel(const MasAdamItem* __restrict__ items, float* const* __restrict__ other, int n_items) {
    const int b = blockIdx.x;
    const int idx = item_index_of_block(items, n_items, b);
    const MasAdamItem it = items[idx];
    float* const q = other[idx];
    if (q == nullptr) return;
    const long long base = (long long)(b - it.first_block) * ADAM_PER_BLOCK;
    if (((reinterpret_cast<uintptr_t>(it.p) | reinterpret_cast<uintptr_t>(q)) & 15) == 0 && base + ADAM_PER_BLOCK <= it.n) {
        f32x4 x[4], y[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long i = base + (long long)(k * ADAM_NT + threadIdx.x) * 4;
            x[k] = *reinterpret_cast<const f32x4*>(it.p + i); y[k] = *reinterpret_cast<const f32x4*>(q + i);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long i = base + (long long)(k * ADAM_NT + threadIdx.x) * 4;
            *reinterpret_cast<f32x4*>(it.p + i) = y[k]; *reinterpret_cast<f32x4*>(q + i) = x[k];
        }
    } else {
        for (int k = threadIdx.x; k < ADAM_PER_BLOCK; k += ADAM_NT) {
            const long long i = base + k;
            if (i < it.n) { const float x = it.p[i], y = q[i]; it.p[i] = y; q[i] = x; }
        }
    }
}

// ---- the step on the device ---------------------------------------------------------------------------------------------------------
// One thread per item, in front of the Adam launch of mas_adam_multi_dev: rec[4 i ..] = {step_size, sqrt(bc2), lr, ema_w} of item i from its
// step count on the device (t = *step[i] + 1: the count is advanced AFTER the step), the learning rate on the device and the EMA counter k
// on the device.  The formulas and their precision are adam_launch's on the host: bc = 1 - beta^t in fp64 from the caller's fp64 betas,
// step_size = (float)(lr / bc1), (float)sqrt(bc2); ema_w = 1 - (float)min(d, (1 + k) / (10 + k)) with the minimum in fp64 and the
// subtraction in fp32 (mas_adam_multi_ema's 1.0f - ema_decay).  Two fp64 pow per parameter and step, not two per work-group: the Adam
// kernel keeps its registers, and a model of 150 tensors computes 300 powers instead of two in each of its tens of thousands of work-groups.
__global__ __launch_bounds__(ADAM_NT) void adam_dev_scalars_kernel(const float* const* __restrict__ step, int n_items, const float* __restrict__ lr_dev,
                                                                   double b1, double b2, double ema_decay, const float* __restrict__ ema_count,
                                                                   float* __restrict__ rec) {
    const int i = blockIdx.x * ADAM_NT + threadIdx.x;
    if (i >= n_items) return;
    const double t = (double)*step[i] + 1.0;
    const float lr = *lr_dev;
    double d = ema_decay;
    if (ema_count != nullptr) {
        const double k = (double)*ema_count, w = (1.0 + k) / (10.0 + k);
        d = w < d ? w : d;
    }
    f32x4 r;
    r[0] = (float)((double)lr / (1.0 - pow(b1, t)));
    r[1] = (float)sqrt(1.0 - pow(b2, t));
    r[2] = lr;
    r[3] = 1.0f - (float)d;
    *reinterpret_cast<f32x4*>(rec + 4 * (long long)i) = r;
}

// counters[i] += 1 (fp32: exact up to 2^24 steps, torch's own `step` tensors are fp32 too).  A launch of its own BEHIND the step's Adam
// launches: no work-group reads a counter that another one is writing (mas_decode_advance is the precedent).
__global__ __launch_bounds__(ADAM_NT) void adam_advance_dev_kernel(float* __restrict__ counters, int n) {
    const int i = blockIdx.x * ADAM_NT + threadIdx.x;
    if (i < n) counters[i] += 1.0f;
}

}  // namespace

extern "C" int mas_adam_blocks(long long numel) { return numel <= 0 ? 0 : (int)((numel + ADAM_PER_BLOCK - 1) / ADAM_PER_BLOCK); }

namespace {

// DEV: `dev_scalars` (4 floats per item, device) replaces lr / the bias corrections / ema_w, none of which is read; the caller has issued
// adam_dev_scalars_kernel on the same stream
template <bool SCALE, bool DECOUPLED, bool EMA = false, bool DEV = false>
int adam_launch(const char* name, const MasAdamItem* items_device, int n_items, int total_blocks, float lr, float beta1, float beta2, float eps,
                float weight_decay, double bias_correction1, double bias_correction2, const float* grad_scale_device, void* stream,
                float* const* ema_device = nullptr, float ema_w = 0.0f, const float* grad_norm_device = nullptr,
                const float* dev_scalars = nullptr) {
    MAS_ENTER();
    if (!items_device || n_items <= 0 || total_blocks <= 0) MAS_FAIL(MAS_EINVAL, "%s: empty batch", name);
    if (!(bias_correction1 > 0.0) || !(bias_correction2 > 0.0)) MAS_FAIL(MAS_EINVAL, "%s: bias corrections must be positive (step >= 1)", name);
    const float step_size = (float)((double)lr / bias_correction1);
    const float inv_bc2_sqrt = (float)sqrt(bias_correction2);      // (passed as the divisor, like torch's bias_correction2_sqrt)
    hipLaunchKernelGGL((adam_multi_kernel<SCALE, DECOUPLED, EMA, DEV>), dim3((unsigned)total_blocks), dim3(ADAM_NT), 0, reinterpret_cast<hipStream_t>(stream),
                       items_device, n_items, step_size, inv_bc2_sqrt, beta1, beta2, eps, weight_decay, grad_scale_device, lr, ema_device, ema_w,
                       grad_norm_device, dev_scalars);
    MAS_CHECK_LAUNCH(name);
    return MAS_OK;
}

}  // namespace

extern "C" int mas_adam_multi(const MasAdamItem* items_device, int n_items, int total_blocks, float lr, float beta1, float beta2, float eps,
                              float weight_decay, double bias_correction1, double bias_correction2, void* stream) {
    return adam_launch<false, false>("adam_multi", items_device, n_items, total_blocks, lr, beta1, beta2, eps, weight_decay, bias_correction1,
                                     bias_correction2, nullptr, stream);
}

extern "C" int mas_adam_multi_ex(const MasAdamItem* items_device, int n_items, int total_blocks, float lr, float beta1, float beta2, float eps,
                                 float weight_decay, double bias_correction1, double bias_correction2, const float* grad_scale_device,
                                 int decoupled_wd, void* stream) {
    const bool dec = decoupled_wd != 0;
    if (!grad_scale_device && !dec)
        return mas_adam_multi(items_device, n_items, total_blocks, lr, beta1, beta2, eps, weight_decay, bias_correction1, bias_correction2, stream);
#define MAS_ADAM_EX(S, D) adam_launch<S, D>("adam_multi_ex", items_device, n_items, total_blocks, lr, beta1, beta2, eps, weight_decay, \
                                            bias_correction1, bias_correction2, grad_scale_device, stream)
    if (grad_scale_device) return dec ? MAS_ADAM_EX(true, true) : MAS_ADAM_EX(true, false);
    return MAS_ADAM_EX(false, true);
#undef MAS_ADAM_EX
}

extern "C" int mas_adam_multi_ema(const MasAdamItem* items_device, float* const* ema_device, int n_items, int total_blocks, float lr, float beta1,
                                  float beta2, float eps, float weight_decay, double bias_correction1, double bias_correction2,
                                  const float* grad_scale_device, int decoupled_wd, float ema_decay, const float* grad_norm_device, void* stream) {
    MAS_ENTER();
    if (!items_device || n_items <= 0 || total_blocks <= 0) MAS_FAIL(MAS_EINVAL, "adam_multi_ema: empty batch");
    if (!(ema_decay >= 0.0f && ema_decay < 1.0f)) MAS_FAIL(MAS_EINVAL, "adam_multi_ema: ema_decay must be in [0, 1)");
    if (!ema_device && !grad_norm_device)
        return mas_adam_multi_ex(items_device, n_items, total_blocks, lr, beta1, beta2, eps, weight_decay, bias_correction1, bias_correction2,
                                 grad_scale_device, decoupled_wd, stream);
    const bool dec = decoupled_wd != 0;
    const float ema_w = 1.0f - ema_decay;
#define MAS_ADAM_EMA(S, D) adam_launch<S, D, true>("adam_multi_ema", items_device, n_items, total_blocks, lr, beta1, beta2, eps, weight_decay, \
                                                   bias_correction1, bias_correction2, grad_scale_device, stream, ema_device, ema_w, grad_norm_device)
    if (grad_scale_device) return dec ? MAS_ADAM_EMA(true, true) : MAS_ADAM_EMA(true, false);
    return dec ? MAS_ADAM_EMA(false, true) : MAS_ADAM_EMA(false, false);
#undef MAS_ADAM_EMA
}

extern "C" int mas_adam_multi_dev(const MasAdamItem* items_device, float* const* ema_device, const float* const* step_device, int n_items,
                                  int total_blocks, const float* lr_device, double beta1, double beta2, float eps, float weight_decay,
                                  const float* grad_scale_device, int decoupled_wd, double ema_decay, const float* ema_count_device,
                                  const float* grad_norm_device, float* scalars_device, void* stream) {
    MAS_ENTER();
    if (!items_device || !step_device || !lr_device || !scalars_device || n_items <= 0 || total_blocks <= 0)
        MAS_FAIL(MAS_EINVAL, "adam_multi_dev: null or empty arguments");
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) MAS_FAIL(MAS_EINVAL, "adam_multi_dev: betas must be in [0, 1)");
    if (!(ema_decay >= 0.0 && ema_decay < 1.0)) MAS_FAIL(MAS_EINVAL, "adam_multi_dev: ema_decay must be in [0, 1)");
    if ((reinterpret_cast<uintptr_t>(scalars_device) & 15) != 0) MAS_FAIL(MAS_EINVAL, "adam_multi_dev: scalars_device must be 16-byte aligned");
    hipLaunchKernelGGL(adam_dev_scalars_kernel, dim3((unsigned)((n_items + ADAM_NT - 1) / ADAM_NT)), dim3(ADAM_NT), 0, reinterpret_cast<hipStream_t>(stream),
                       step_device, n_items, lr_device, beta1, beta2, ema_decay, ema_count_device, scalars_device);
    MAS_CHECK_LAUNCH("adam_multi_dev (scalars)");
    const bool dec = decoupled_wd != 0;
    // (bias corrections of 1: only adam_launch's argument check reads them; the kernel takes its scalars from scalars_device)
#define MAS_ADAM_DEV(S, D) adam_launch<S, D, true, true>("adam_multi_dev", items_device, n_items, total_blocks, 0.0f, (float)beta1, (float)beta2, eps, \
                                                         weight_decay, 1.0, 1.0, grad_scale_device, stream, ema_device, 0.0f, grad_norm_device, scalars_device)
    if (grad_scale_device) return dec ? MAS_ADAM_DEV(true, true) : MAS_ADAM_DEV(true, false);
    return dec ? MAS_ADAM_DEV(false, true) : MAS_ADAM_DEV(false, false);
#undef MAS_ADAM_DEV
}

extern "C" int mas_adam_advance_dev(float* counters, int n, void* stream) {
    MAS_ENTER();
    if (!counters || n <= 0) MAS_FAIL(MAS_EINVAL, "adam_advance_dev: null or empty arguments");
    hipLaunchKernelGGL(adam_advance_dev_kernel, dim3((unsigned)((n + ADAM_NT - 1) / ADAM_NT)), dim3(ADAM_NT), 0, reinterpret_cast<hipStream_t>(stream),
                       counters, n);
    MAS_CHECK_LAUNCH("adam_advance_dev");
    return MAS_OK;
}

extern "C" int mas_swap_multi(const MasAdamItem* items_device, float* const* other_device, int n_items, int total_blocks, void* stream) {
    MAS_ENTER();
    if (!items_device || !other_device || n_items <= 0 || total_blocks <= 0) MAS_FAIL(MAS_EINVAL, "swap_multi: null or empty arguments");
    hipLaunchKernelGGL(swap_multi_kernel, dim3((unsigned)total_blocks), dim3(ADAM_NT), 0, reinterpret_cast<hipStream_t>(stream), items_device,
                       other_device, n_items);
    MAS_CHECK_LAUNCH("swap_multi");
    return MAS_OK;
}

extern "C" int mas_grad_sqnorm_multi(const MasAdamItem* items_device, int n_items, int total_blocks, double* partials, void* stream) {
    MAS_ENTER();
    if (!items_device || !partials || n_items <= 0 || total_blocks <= 0) MAS_FAIL(MAS_EINVAL, "grad_sqnorm_multi: null or empty arguments");
    hipLaunchKernelGGL(grad_sqnorm_multi_kernel, dim3((unsigned)total_blocks), dim3(ADAM_NT), 0, reinterpret_cast<hipStream_t>(stream), items_device,
                       n_items, partials);
    MAS_CHECK_LAUNCH("grad_sqnorm_multi");
    return MAS_OK;
}

extern "C" int mas_grad_clip_coef(const double* partials, int n_partials, const double* extra, int n_extra, float max_norm, float* out,
                                  void* stream) {
    MAS_ENTER();
    if (!out || n_partials < 0 || n_extra < 0 || n_partials + n_extra <= 0 || (n_partials > 0 && !partials) || (n_extra > 0 && !extra))
        MAS_FAIL(MAS_EINVAL, "grad_clip_coef: null or empty arguments");
    if (!(max_norm > 0.0f) || isinf(max_norm)) MAS_FAIL(MAS_EINVAL, "grad_clip_coef: max_norm must be positive and finite");
    hipLaunchKernelGGL(grad_clip_coef_kernel, dim3(1), dim3(ADAM_NT), 0, reinterpret_cast<hipStream_t>(stream), partials, n_partials, extra, n_extra,
                       max_norm, out);
    MAS_CHECK_LAUNCH("grad_clip_coef");
    return MAS_OK;
}

extern "C" int mas_grad_scale_multi(const MasAdamItem* items_device, int n_items, int total_blocks, const float* scale_device, void* stream) {
    MAS_ENTER();
    if (!items_device || !scale_device || n_items <= 0 || total_blocks <= 0) MAS_FAIL(MAS_EINVAL, "grad_scale_multi: null or empty arguments");
    hipLaunchKernelGGL(grad_scale_multi_kernel, dim3((unsigned)total_blocks), dim3(ADAM_NT), 0, reinterpret_cast<hipStream_t>(stream), items_device,
                       n_items, scale_device);
    MAS_CHECK_LAUNCH("grad_scale_multi");
    return MAS_OK;
}
