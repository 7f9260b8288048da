// K-means (Lloyd) for the codebook re-initialisation, wholly on the device (models/kmeans.py with on_device; reference
// models/modules.py:487-499 through fast_pytorch_kmeans; oracle/kmeans_oracle.py restates the rule).  C contract: include/mas_hip.h,
// "K-means re-initialisation".  A fit is a FIXED sequence of launches -- the host enqueues max_iter iterations and reads nothing -- and
// every sum is taken in an order the kernels fix, so a fit repeats bit for bit; there is no float atomic anywhere.
//
//   kmeans_init_kernel      centroid k = point row P(k), copied bit for bit; P the keyed bijection of mas_bijection.h, stream 2.
//   kmeans_reset_kernel     info = {0, 0}, shift = 0.
//   per iteration:
//     row_sqnorm            |c|^2 of the centroids                                     (vq_core.h; |x|^2 of the points: once per fit)
//     vq_partial<D>         the lookup's own split (min, argmin), lowest index on ties (vq_core.h, the one copy)
//     kmeans_finalize_kernel  merges the split partials and writes the index -- no z_q, no loss
//     kmeans_update_kernel  a work-group owns KM_CODES centroids (vq_bwd_codebook_kernel's geometry): its four waves scan a quarter of the
//                           assignments each, 64 per ballot, in position order, each wave adding the point rows into its OWN fp32 LDS
//                           accumulator; the four are folded in wave order.  new = sum / count, an empty cluster -> the zero vector.  The
//                           group reads only its own centroids' old rows, so it writes the new rows IN PLACE, and stores its partial of
//                           sum (new - old)^2: differences in fp32, squares and their sum in fp64, fixed order.
//     kmeans_advance_kernel ONE work-group: adds the partials in fixed order (fp64), then thread 0 stores info = {iterations + 1,
//                           shift <= tol} and shift.  Nobody else reads or writes them in that launch (mas_decode_advance is the precedent).
//   Every kernel of an iteration reads info[1] first and returns before any other load once it is set: after convergence the remaining
//   iterations are empty launches and nothing is written, so `assign` stays the assignment of the last executed iteration.
#include "vq_core.h"
#include "mas_bijection.h"

namespace {

constexpr int KM_CODES = 8;          // centroids per update work-group: 4 waves x 8 x 256 fp32 = 32 KB of LDS
constexpr int KM_MAX_ROWS = 1 << 30;

__global__ __launch_bounds__(NT) void kmeans_init_kernel(const float* __restrict__ x, int M, int K, int D, uint32_t k0, uint32_t k1,
                                                         uint32_t draw, float* __restrict__ cent, int32_t* __restrict__ init_idx) {
    const int k = blockIdx.x * (NT / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (k >= K) return;
    const uint32_t src = rsv_perm((uint32_t)k, (uint32_t)M, rsv_half_bits((uint32_t)M), 2u, draw, k0, k1);      // < M by construction
    const f32x4* from = reinterpret_cast<const f32x4*>(x + (size_t)src * D);
    f32x4* to = reinterpret_cast<f32x4*>(cent + (size_t)k * D);
    for (int q = lane; q < D / 4; q += 64) to[q] = from[q];
    if (init_idx && lane == 0) init_idx[k] = (int32_t)src;
}

__global__ void kmeans_reset_kernel(int32_t* __restrict__ info, double* __restrict__ shift) {
    if (threadIdx.x == 0) { info[0] = 0; info[1] = 0; shift[0] = 0.0; }
}

// one wave per point: merge the split partials (vq_finalize's merge), write the index
__global__ __launch_bounds__(NT) void kmeans_finalize_kernel(const float* __restrict__ pval, const int* __restrict__ pidx, int M, int ksplit,
                                                             int64_t* __restrict__ assign, const int32_t* __restrict__ info) {
    if (info[1]) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int row = blockIdx.x * (NT / 64) + wave;
    if (row >= M) return;
    float bv = INFINITY; int bi = 0x7fffffff;
    for (int sp = lane; sp < ksplit; sp += 64) take_min(bv, bi, pval[(size_t)row * ksplit + sp], pidx[(size_t)row * ksplit + sp]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const float ov = __shfl_xor(bv, o); const int oi = __shfl_xor(bi, o); take_min(bv, bi, ov, oi); }
    if (bi == 0x7fffffff) bi = 0;                // all-NaN row: stay in range
    if (lane == 0) assign[row] = (int64_t)bi;
}

__global__ __launch_bounds__(NT) void kmeans_update_kernel(const float* __restrict__ x, const int64_t* __restrict__ assign, float* cent,
                                                           int M, int K, int D, double* __restrict__ partial,
                                                           const int32_t* __restrict__ info) {
    __shared__ __attribute__((aligned(16))) float accs[NT / 64][KM_CODES][256];
    __shared__ int cnts[NT / 64][KM_CODES];
    __shared__ double red[NT];
    if (info[1]) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k0 = blockIdx.x * KM_CODES;
    for (int i = tid; i < (NT / 64) * KM_CODES * 256; i += NT) (&accs[0][0][0])[i] = 0.0f;
    if (tid < (NT / 64) * KM_CODES) (&cnts[0][0])[tid] = 0;
    __syncthreads();
    const int per = (M + NT / 64 - 1) / (NT / 64);
    const int lo = wave * per, hi = min(M, lo + per);
    const int d4 = lane * 4;
    for (int base = lo; base < hi; base += 64) {
        const int m_l = base + lane;
        const int k_l = m_l < hi ? (int)assign[m_l] - k0 : -1;
        unsigned long long mask = __builtin_amdgcn_ballot_w64(k_l >= 0 && k_l < KM_CODES);
        while (mask) {
            const int bit = __builtin_ctzll(mask);
            mask &= mask - 1;
            const int kk = __builtin_amdgcn_readlane(k_l, bit);
            const int m = base + bit;
            if (d4 < D) {
                const f32x4 xv = *reinterpret_cast<const f32x4*>(x + (size_t)m * D + d4);
                f32x4 a = *reinterpret_cast<f32x4*>(&accs[wave][kk][d4]);
#pragma unroll
                for (int e = 0; e < 4; ++e) a[e] += xv[e];
                *reinterpret_cast<f32x4*>(&accs[wave][kk][d4]) = a;
            }
            if (lane == 0) cnts[wave][kk] += 1;
        }
    }
    __syncthreads();
    double sq = 0.0;
    for (int i = tid; i < KM_CODES * D; i += NT) {
        const int code = i / D, d = i - code * D;
        if (k0 + code < K) {
            float t = accs[0][code][d];
            int n = cnts[0][code];
#pragma unroll
            for (int w = 1; w < NT / 64; ++w) { t += accs[w][code][d]; n += cnts[w][code]; }
            const float nw = n > 0 ? t / (float)n : 0.0f;
            float* p = cent + (size_t)(k0 + code) * D + d;
            const float df = nw - *p;
            sq += (double)df * (double)df;
            *p = nw;
        }
    }
    red[tid] = sq;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
    if (tid == 0) partial[blockIdx.x] = red[0];
}

__global__ __launch_bounds__(NT) void kmeans_advance_kernel(const double* __restrict__ partial, int n, float tol, int32_t* info, double* shift) {
    __shared__ double red[NT];
    if (info[1]) return;
    const int tid = threadIdx.x, iters = info[0];
    double s = 0.0;
    for (int i = tid; i < n; i += NT) s += partial[i];
    red[tid] = s;
    __syncthreads();
    for (int o = NT / 2; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
    // every read of info lies before the barriers above
    if (tid == 0) { shift[0] = red[0]; info[0] = iters + 1; info[1] = red[0] <= (double)tol ? 1 : 0; }
}

size_t km_float_words(int M, int K) { return (((size_t)M + K + (size_t)2 * M * MAX_KSPLIT) + 1) & ~(size_t)1; }

}  // namespace

// workspace: zz[M] | ee[K] | pval[M*MAX_KSPLIT] | pidx[M*MAX_KSPLIT] | (8-byte aligned) partial fp64[ceil(K/KM_CODES)]
extern "C" size_t mas_kmeans_workspace(int M, int K) {
    if (M <= 0 || K <= 0) return 0;
    return km_float_words(M, K) * sizeof(float) + (size_t)mas_cdiv(K, KM_CODES) * sizeof(double) + 64;
}

extern "C" int mas_kmeans_init(const float* points, int M, int K, int D, long long seed, int draw, float* centroids, int32_t* init_idx,
                               void* stream) {
    MAS_ENTER();
    if (D != 32 && D != 64 && D != 128 && D != 256) MAS_FAIL(MAS_EUNSUPPORTED, "kmeans_init: D=%d not in {32,64,128,256}", D);
    if (K < 1 || K > M) MAS_FAIL(MAS_EINVAL, "kmeans_init: needs 1 <= K <= M distinct rows, got K=%d, M=%d", K, M);
    if (M > KM_MAX_ROWS) MAS_FAIL(MAS_EUNSUPPORTED, "kmeans_init: M=%d beyond 2^30 rows", M);
    if (!points || !centroids) MAS_FAIL(MAS_EINVAL, "kmeans_init: null argument");
    if (((uintptr_t)points | (uintptr_t)centroids) & 15) MAS_FAIL(MAS_EINVAL, "kmeans_init: points and centroids must be 16-byte aligned");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(kmeans_init_kernel, dim3(mas_cdiv(K, NT / 64)), dim3(NT), 0, s, points, M, K, D,
                       (uint32_t)((unsigned long long)seed & 0xffffffffu), (uint32_t)((unsigned long long)seed >> 32), (uint32_t)draw, centroids,
                       init_idx);
    MAS_CHECK_LAUNCH("kmeans_init");
    return MAS_OK;
}

extern "C" int mas_kmeans_fit(const float* points, float* centroids, int M, int K, int D, int max_iter, float tol, int64_t* assign,
                              int32_t* info, double* shift, void* workspace, size_t ws_bytes, void* stream) {
    MAS_ENTER();
    if (D != 32 && D != 64 && D != 128 && D != 256) MAS_FAIL(MAS_EUNSUPPORTED, "kmeans_fit: D=%d not in {32,64,128,256}", D);
    if (K < 1 || K > M) MAS_FAIL(MAS_EINVAL, "kmeans_fit: needs 1 <= K <= M, got K=%d, M=%d", K, M);
    if (M > KM_MAX_ROWS) MAS_FAIL(MAS_EUNSUPPORTED, "kmeans_fit: M=%d beyond 2^30 rows", M);
    if (max_iter < 1) MAS_FAIL(MAS_EINVAL, "kmeans_fit: max_iter=%d, needs max_iter >= 1", max_iter);
    if (!points || !centroids || !assign || !info || !shift || !workspace) MAS_FAIL(MAS_EINVAL, "kmeans_fit: null argument");
    if (((uintptr_t)points | (uintptr_t)centroids | (uintptr_t)workspace) & 15)
        MAS_FAIL(MAS_EINVAL, "kmeans_fit: points, centroids and workspace must be 16-byte aligned");
    if (((uintptr_t)assign | (uintptr_t)shift) & 7 || (uintptr_t)info & 3) MAS_FAIL(MAS_EINVAL, "kmeans_fit: assign / shift / info misaligned");
    if (ws_bytes < mas_kmeans_workspace(M, K)) MAS_FAIL(MAS_EWORKSPACE, "kmeans_fit: workspace too small");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    float* zz = reinterpret_cast<float*>(workspace);
    float* ee = zz + M;
    float* pval = ee + K;
    int* pidx = reinterpret_cast<int*>(pval + (size_t)M * MAX_KSPLIT);
    double* partial = reinterpret_cast<double*>(zz + km_float_words(M, K));
    const int ksplit = pick_ksplit(M, K), nb = mas_cdiv(K, KM_CODES);
    const dim3 grid(mas_cdiv(M, ROWS_PER_BLOCK) * ksplit);
    hipLaunchKernelGGL(kmeans_reset_kernel, dim3(1), dim3(64), 0, s, info, shift);
    hipLaunchKernelGGL(row_sqnorm, dim3(mas_cdiv(M, NT / 64)), dim3(NT), 0, s, points, M, D, zz, (const int32_t*)nullptr);
    MAS_CHECK_LAUNCH("kmeans reset / row_sqnorm");
    for (int it = 0; it < max_iter; ++it) {
        hipLaunchKernelGGL(row_sqnorm, dim3(mas_cdiv(K, NT / 64)), dim3(NT), 0, s, (const float*)centroids, K, D, ee, (const int32_t*)info);
        launch_vq_partial(D, grid, s, points, centroids, zz, ee, M, K, ksplit, pval, pidx, info);
        hipLaunchKernelGGL(kmeans_finalize_kernel, dim3(mas_cdiv(M, NT / 64)), dim3(NT), 0, s, (const float*)pval, (const int*)pidx, M, ksplit,
                           assign, (const int32_t*)info);
        hipLaunchKernelGGL(kmeans_update_kernel, dim3(nb), dim3(NT), 0, s, points, (const int64_t*)assign, centroids, M, K, D, partial,
                           (const int32_t*)info);
        hipLaunchKernelGGL(kmeans_advance_kernel, dim3(1), dim3(NT), 0, s, (const double*)partial, nb, tol, info, shift);
        MAS_CHECK_LAUNCH("kmeans iteration");
    }
    return MAS_OK;
}
