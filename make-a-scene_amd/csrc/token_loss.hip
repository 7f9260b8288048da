// Stage-2 token cross-entropy for gfx950 (reference train.py:152: F.cross_entropy(pred_logit.view(-1, V), img_token.view(-1))):
//   * token_ce_fwd    : ONE read of the logits -> per row m = max_j x_j, log l = log sum_j exp(x_j - m), the target logit x_t and (with
//                       label smoothing) sum_j (x_j - m); the row loss and {m, log l} for the backward
//   * token_ce_reduce : one work-group, fp64 from the first addition, fixed order, no atomics -> {loss, count of rows not ignored}
//   * token_ce_bwd    : one read of the logits + one write  dx_j = w_r (exp((x_j - m) - log l) - (1 - eps) [j = t] - eps / V)
// Logits are read IN PLACE through (outer_stride, ld): row r starts at base + (r / inner) * outer_stride + (r % inner) * ld, so the
// [B, L, V] slice of a [B, S, V] tensor needs no copy and no fp32 cast.  One work-group of 256 lanes per row: a row of 8192 bf16 is 16 KB
// = 4 16-byte units per lane, which stay in registers between the exact maximum and the sum of exponentials (two passes over registers,
// one over memory); the two work-group reductions per row are hidden by the four or five work-groups resident per CU.  Longer rows, and rows
// that are not 16-byte aligned, stream with a per-lane online (m, l) merged in a fixed order, so V is bounded by neither registers nor LDS.
// The target logit is picked by comparing the running column index with t -- there is no load indexed by a target value.
#include "token_row_core.h"

namespace {

template <typename T>
__global__ __launch_bounds__(NT) void token_ce_fwd_kernel(const T* __restrict__ x, long long rows, int V, long long inner,
                                                          long long outer_stride, long long ld, const long long* __restrict__ target,
                                                          long long ignore_index, float eps, float* __restrict__ row_loss,
                                                          float* __restrict__ stats) {
    constexpr int N = Unit<T>::N;
    __shared__ float s_max[NW];
    __shared__ float s_sum[3][NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
        const long long t = target[r];
        if (t == ignore_index) {                                 // (uniform over the work-group) the row is not read
            if (tid == 0) { row_loss[r] = 0.0f; stats[2 * r] = 0.0f; stats[2 * r + 1] = 0.0f; }
            continue;
        }
        const auto [xr, nfull, e0] = row_plan(x, r, V, inner, outer_stride, ld);
        const int tc = t >= 0 && t < (long long)V ? (int)t : -1; // the target's column, or no column at all
        float M, l = 0.0f, s = 0.0f, xt = 0.0f;                  // s = sum_j (x_j - M): m - mean_j x_j without the cancellation of sum_j x_j
        if (nfull <= KMAX * NT && V - e0 <= NT) {                // resident: token_readout.hip spells the same test (token_row_core.h)
            // the row fits in registers: exact maximum first, then the sums, from the same registers
            u32x4 raw[KMAX];                                    // as loaded: 4 VGPRs per unit, converted at each use
            float vt = 0.0f;
            float mx = -INFINITY;
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                const int u = k * NT + tid;
                if (u < nfull) {
                    raw[k] = *reinterpret_cast<const u32x4*>(xr + (size_t)u * N);
                    float v[N];
                    cvt_unit<T, N>(raw[k], v);
#pragma unroll
                    for (int e = 0; e < N; ++e) mx = fmaxf(mx, v[e]);
                }
            }
            const bool has_t = tid < V - e0;
            if (has_t) { vt = (float)xr[e0 + tid]; mx = fmaxf(mx, vt); }
            M = row_max(mx, s_max, lane, wave);
            const float ms = exp_shift(M);
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                const int u = k * NT + tid;
                if (u < nfull) {
                    float v[N];
                    cvt_unit<T, N>(raw[k], v);
#pragma unroll
                    for (int e = 0; e < N; ++e) {
                        const float d = v[e] - ms;
                        l += __expf(d);
                        s += d;
                        if (u * N + e == tc) xt = v[e];
                    }
                }
            }
            if (has_t) {
                const float d = vt - ms;
                l += __expf(d);
                s += d;
                if (e0 + tid == tc) xt = vt;
            }
        } else {
            // streaming: a lane keeps an online (m, l) and sum_j (x_j - c) against its own first element c; merged below in a fixed order
            float mi = -INFINITY, li = 0.0f, ci = 0.0f, si = 0.0f;
            int ni = 0;
#pragma unroll 1
            for (int u = tid; u < nfull; u += NT) {
                float v[N];
                ld_unit<T, N>(xr + (size_t)u * N, v);
                const float um = unit_max(v);
                if (ni == 0) ci = v[0];
                if (um > mi) { li *= __expf(mi - um); mi = um; }   // the online step: token_readout.hip has the same one, with its a
                const float ms = exp_shift(mi);
#pragma unroll
                for (int e = 0; e < N; ++e) {
                    li += __expf(v[e] - ms);
                    si += v[e] - ci;
                    if (u * N + e == tc) xt = v[e];
                }
                ni += N;
            }
#pragma unroll 1
            for (int j = e0 + tid; j < V; j += NT) {
                const float a = (float)xr[j];
                if (ni == 0) ci = a;
                if (a > mi) { li *= __expf(mi - a); mi = a; }
                const float ms = exp_shift(mi);
                li += __expf(a - ms);
                si += a - ci;
                if (j == tc) xt = a;
                ni += 1;
            }
            M = row_max(mi, s_max, lane, wave);
            const float ms = exp_shift(M);
            l = ni ? li * __expf(mi - ms) : 0.0f;                // (mi == M: exp(0) = 1 exactly)
            s = ni ? si - (float)ni * (ms - ci) : 0.0f;
        }
        l = wave_sum(l); s = wave_sum(s); xt = wave_sum(xt);     // xt: one lane holds it, the others add exact zeros
        if (lane == 0) { s_sum[0][wave] = l; s_sum[1][wave] = s; s_sum[2][wave] = xt; }
        __syncthreads();
        if (tid == 0) {
            const float L = (s_sum[0][0] + s_sum[0][1]) + (s_sum[0][2] + s_sum[0][3]);
            const float S = (s_sum[1][0] + s_sum[1][1]) + (s_sum[1][2] + s_sum[1][3]);
            const float XT = (s_sum[2][0] + s_sum[2][1]) + (s_sum[2][2] + s_sum[2][3]);
            const float logl = logf(L);
            // {m, log l} stay apart: at |x| = 1e4 the sum m + log l would round to 1e-3 and the loss with it
            float loss = (1.0f - eps) * ((M - XT) + logl);
            if (eps > 0.0f) loss += eps * (-S / (float)V + logl);   // (m - mean_j x_j) + log l; skipped at eps = 0 (0 * inf on -inf logits)
            if (t < 0 || t >= (long long)V) loss = __builtin_nanf("");
            row_loss[r] = loss;
            stats[2 * r] = M;
            stats[2 * r + 1] = logl;
        }
        __syncthreads();                                          // s_max / s_sum are reused by the next row
    }
}

// One work-group: lane i adds rows i, i + 256, ... in fp64, then a fixed tree over the 256 partial sums.
__global__ __launch_bounds__(NT) void token_ce_reduce_kernel(const float* __restrict__ row_loss, const long long* __restrict__ target,
                                                             long long rows, long long ignore_index, int mean, float* __restrict__ out) {
    __shared__ double s_s[NT];
    __shared__ long long s_c[NT];
    const int tid = threadIdx.x;
    double s = 0.0;
    long long c = 0;
    for (long long i = tid; i < rows; i += NT) {
        s += (double)row_loss[i];
        c += target[i] != ignore_index;
    }
    s_s[tid] = s; s_c[tid] = c;
    __syncthreads();
    for (int o = NT / 2; o >= 1; o >>= 1) {
        if (tid < o) { s_s[tid] += s_s[tid + o]; s_c[tid] += s_c[tid + o]; }
        __syncthreads();
    }
    if (tid == 0) {
        out[0] = (float)(mean ? s_s[0] / (double)s_c[0] : s_s[0]);   // every row ignored: 0 / 0 = NaN, as torch
        out[1] = (float)s_c[0];
    }
}

template <typename T>
__global__ __launch_bounds__(NT) void token_ce_bwd_kernel(const T* __restrict__ x, long long rows, int V, long long inner,
                                                          long long outer_stride, long long ld, const long long* __restrict__ target,
                                                          long long ignore_index, float eps, const float* __restrict__ stats,
                                                          const float* __restrict__ grad, int grad_per_row,
                                                          const float* __restrict__ loss_count, T* __restrict__ dx) {
    constexpr int N = Unit<T>::N;
    const int tid = threadIdx.x;
    const float on = 1.0f - eps, sm = eps / (float)V;
    for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
        const long long t = target[r];
        T* dr = dx + r * (long long)V;
        const bool st16 = aligned16(dr);
        if (t == ignore_index || t < 0 || t >= (long long)V) {   // (uniform) ignored: a zero row; any other target outside [0, V): NaN
            const float f = t == ignore_index ? 0.0f : __builtin_nanf("");
            const int nf = st16 ? V / N : 0;
            float fv[N];
#pragma unroll
            for (int e = 0; e < N; ++e) fv[e] = f;
            for (int u = tid; u < nf; u += NT) st_unit<T, N>(dr + (size_t)u * N, fv);
            for (int j = nf * N + tid; j < V; j += NT) dr[j] = (T)f;
            continue;
        }
        float w = grad_per_row ? grad[r] : grad[0];
        if (loss_count) w = w / loss_count[1];                   // mean: the count the forward left on the device
        const float m = stats[2 * r], logl = stats[2 * r + 1];
        const auto [xr, nfull, e0] = row_plan(x, r, V, inner, outer_stride, ld);   // (e0: not needed here)
        for (int u0 = 0; u0 < nfull; u0 += KMAX * NT) {          // KMAX loads in flight per lane
            float v[KMAX][N];
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                const int u = u0 + k * NT + tid;
                if (u < nfull) ld_unit<T, N>(xr + (size_t)u * N, v[k]);
            }
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                const int u = u0 + k * NT + tid;
                if (u < nfull) {
#pragma unroll
                    for (int e = 0; e < N; ++e) {
                        const float p = __expf((v[k][e] - m) - logl);
                        v[k][e] = w * (p - ((long long)(u * N + e) == t ? on : 0.0f) - sm);
                    }
                    if (st16) st_unit<T, N>(dr + (size_t)u * N, v[k]);
                    else {
#pragma unroll
                        for (int e = 0; e < N; ++e) dr[(size_t)u * N + e] = (T)v[k][e];
                    }
                }
            }
        }
        for (int j = nfull * N + tid; j < V; j += NT) {
            const float p = __expf(((float)xr[j] - m) - logl);
            dr[j] = (T)(w * (p - ((long long)j == t ? on : 0.0f) - sm));
        }
    }
}

}  // namespace

extern "C" int mas_token_ce_fwd(const void* logits, int dtype, long long rows, int V, long long inner, long long outer_stride, long long ld,
                                const int64_t* target, long long ignore_index, float label_smoothing, float* row_loss, float* stats,
                                void* stream) {
    MAS_ENTER();
    if (int rc = row_check("token_ce_fwd", logits, dtype, rows, V, inner, outer_stride, ld, target, label_smoothing)) return rc;
    if (!row_loss || !stats) MAS_FAIL(MAS_EINVAL, "token_ce_fwd: null argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(row_grid(rows)), block(NT);
    const long long* tg = reinterpret_cast<const long long*>(target);
    if (dtype == MAS_BF16)
        hipLaunchKernelGGL((token_ce_fwd_kernel<bf16_t>), grid, block, 0, s, (const bf16_t*)logits, rows, V, inner, outer_stride, ld, tg,
                           ignore_index, label_smoothing, row_loss, stats);
    else
        hipLaunchKernelGGL((token_ce_fwd_kernel<float>), grid, block, 0, s, (const float*)logits, rows, V, inner, outer_stride, ld, tg,
                           ignore_index, label_smoothing, row_loss, stats);
    MAS_CHECK_LAUNCH("token_ce_fwd");
    return MAS_OK;
}

extern "C" int mas_token_ce_reduce(const float* row_loss, const int64_t* target, long long rows, long long ignore_index, int reduction,
                                   float* out, void* stream) {
    MAS_ENTER();
    if (!row_loss || !target || !out) MAS_FAIL(MAS_EINVAL, "token_ce_reduce: null argument");
    if (rows <= 0) MAS_FAIL(MAS_EINVAL, "token_ce_reduce: rows=%lld must be positive", rows);
    if (reduction != MAS_CE_MEAN && reduction != MAS_CE_SUM)
        MAS_FAIL(MAS_EINVAL, "token_ce_reduce: reduction %d (MAS_CE_MEAN or MAS_CE_SUM; MAS_CE_NONE has nothing to reduce)", reduction);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(token_ce_reduce_kernel, dim3(1), dim3(NT), 0, s, row_loss, reinterpret_cast<const long long*>(target), rows,
                       ignore_index, reduction == MAS_CE_MEAN ? 1 : 0, out);
    MAS_CHECK_LAUNCH("token_ce_reduce");
    return MAS_OK;
}

extern "C" int mas_token_ce_bwd(const void* logits, int dtype, long long rows, int V, long long inner, long long outer_stride, long long ld,
                                const int64_t* target, long long ignore_index, float label_smoothing, const float* stats,
                                const float* grad, const float* loss_count, int reduction, void* dx, void* stream) {
    MAS_ENTER();
    if (int rc = row_check("token_ce_bwd", logits, dtype, rows, V, inner, outer_stride, ld, target, label_smoothing)) return rc;
    if (!stats || !grad || !dx) MAS_FAIL(MAS_EINVAL, "token_ce_bwd: null argument");
    if (reduction != MAS_CE_NONE && reduction != MAS_CE_MEAN && reduction != MAS_CE_SUM)
        MAS_FAIL(MAS_EINVAL, "token_ce_bwd: reduction %d", reduction);
    if (reduction == MAS_CE_MEAN && !loss_count) MAS_FAIL(MAS_EINVAL, "token_ce_bwd: the mean needs the {loss, count} pair of token_ce_reduce");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(row_grid(rows)), block(NT);
    const long long* tg = reinterpret_cast<const long long*>(target);
    const float* lc = reduction == MAS_CE_MEAN ? loss_count : nullptr;
    const int per_row = reduction == MAS_CE_NONE ? 1 : 0;
    if (dtype == MAS_BF16)
        hipLaunchKernelGGL((token_ce_bwd_kernel<bf16_t>), grid, block, 0, s, (const bf16_t*)logits, rows, V, inner, outer_stride, ld, tg,
                           ignore_index, label_smoothing, stats, grad, per_row, lc, (bf16_t*)dx);
    else
        hipLaunchKernelGGL((token_ce_bwd_kernel<float>), grid, block, 0, s, (const float*)logits, rows, V, inner, outer_stride, ld, tg,
                           ignore_index, label_smoothing, stats, grad, per_row, lc, (float*)dx);
    MAS_CHECK_LAUNCH("token_ce_bwd");
    return MAS_OK;
}
