// Whole-image LPIPS-VGG16 on gfx950 (losses/lpips.py:LPIPS.forward; mas_hip/lpips.py): everything but the thirteen convolutions,
// which run on the library's convolution kernels (mas_conv_fwd), on plain NHWC maps [2 B, H, W, C] -- the B real images first, then
// the B reconstructions:
//   pack: the ScalingLayer, the cat and the cast in one pass, NCHW / channels_last fp32 / bf16 images -> [2 B, H, W, 8] (RGB and
//     five zeros, the first convolution's input), and its adjoint into d fake;
//   ReLU in place; the 2x2 / stride-2 max-pool (floor) and its backward (first maximum of the window, torch's tie rule; the ReLU mask
//     of the level and the head's gradient seed folded in);
//   the LPIPS head per level (channel normalisation of both sides, difference, square, lin<k> weights; per-image fixed-order partial
//     sums), one finalize launch (a tree over the partial sums), and the head's backward for the rec side.
// These are object.hip's kernels without the atlas: no tile table, no cell record per pixel.  What the two files share lives in
// lpips_core.h, which also says what each keeps for itself and why.  Activations are bf16 or fp32; arithmetic in
// fp32; no float atomics anywhere (bitwise repeatable).
#include "lpips_core.h"

namespace {

constexpr int MAX_LEVELS = 8;
constexpr long long MAX_PIX = 1LL << 30;   // pixels per image
constexpr int MAX_BLOCKS = 1 << 18;        // partial sums per image and level: 256 chains of <= 1024 in the finalize

struct Levels { int n; int hw[MAX_LEVELS]; int blocks[MAX_LEVELS]; };

// one thread per canvas pixel: CP channels
template <typename T>
__global__ __launch_bounds__(NT) void pack_fwd_kernel(MasFaceImage real, MasFaceImage fake, const float* __restrict__ shift,
                                                      const float* __restrict__ scale, T* __restrict__ out) {
    const long long hw = (long long)real.H * real.W;
    const long long total = 2LL * real.N * hw;
    const float s0 = shift[0], s1 = shift[1], s2 = shift[2], k0 = scale[0], k1 = scale[1], k2 = scale[2];
    for (long long i = gtid(); i < total; i += gsize()) {
        const int n = (int)(i / hw);
        const bool rec = n >= real.N;
        const MasFaceImage& im = rec ? fake : real;
        const int b = rec ? n - real.N : n;
        const int y = (int)((i % hw) / real.W), x = (int)(i % real.W);
        const long long base = (long long)b * im.sn + (long long)y * im.sh + (long long)x * im.sw;
        V8<T> v = zero8<T>();
        v[0] = (T)((ld_img(im, base) - s0) / k0);
        v[1] = (T)((ld_img(im, base + im.sc) - s1) / k1);
        v[2] = (T)((ld_img(im, base + 2 * im.sc) - s2) / k2);
        st8(out + i * CP, v);
    }
}

// one thread per pixel of d fake
template <typename TD, typename TR>
__global__ __launch_bounds__(NT) void pack_bwd_kernel(const TD* __restrict__ dcan, const float* __restrict__ scale, MasFaceImage dfake) {
    const long long hw = (long long)dfake.H * dfake.W;
    const long long total = (long long)dfake.N * hw;
    const float k[3] = {scale[0], scale[1], scale[2]};
    TR* o = reinterpret_cast<TR*>(dfake.data);
    for (long long i = gtid(); i < total; i += gsize()) {
        const int b = (int)(i / hw);
        const int y = (int)((i % hw) / dfake.W), x = (int)(i % dfake.W);
        const TD* g = dcan + i * CP;
        const long long base = (long long)b * dfake.sn + (long long)y * dfake.sh + (long long)x * dfake.sw;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) o[base + ch * dfake.sc] = (TR)((float)g[ch] / k[ch]);
    }
}

// 8 channels per thread
template <typename T>
__global__ __launch_bounds__(NT) void relu_fwd_kernel(T* __restrict__ y, long long n8) {
    for (long long i = gtid(); i < n8; i += gsize()) {
        V8<T> v = ld8(y + i * 8);
#pragma unroll
        for (int k = 0; k < 8; ++k) v[k] = (float)v[k] < 0.0f ? (T)0.0f : v[k];      // a NaN stays a NaN, as in F.relu
        st8(y + i * 8, v);
    }
}

// x [N, H, W, C] -> y [N, H / 2, W / 2, C]; 8 channels of one output pixel per thread
template <typename T>
__global__ __launch_bounds__(NT) void pool_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, int N, int H, int W, int C) {
    const int ho = H >> 1, wo = W >> 1, c8 = C / 8;
    const long long total = (long long)N * ho * wo * c8;
    for (long long i = gtid(); i < total; i += gsize()) {
        const int cv = (int)(i % c8);
        const long long pix = i / c8;
        const int n = (int)(pix / ((long long)ho * wo));
        const int oy = (int)((pix / wo) % ho), ox = (int)(pix % wo);
        const T* src = x + (((long long)n * H + 2 * oy) * W + 2 * ox) * C + cv * 8;
        const V8<T> a = ld8(src), b = ld8(src + C), c = ld8(src + (long long)W * C), d = ld8(src + (long long)W * C + C);
        V8<T> v;
#pragma unroll
        for (int k = 0; k < 8; ++k) {                 // torch's scan: a larger value or a NaN replaces the maximum
            float m = (float)a[k];
            const float q[3] = {(float)b[k], (float)c[k], (float)d[k]};
#pragma unroll
            for (int t = 0; t < 3; ++t) m = (q[t] > m || q[t] != q[t]) ? q[t] : m;
            v[k] = (T)m;
        }
        st8(y + i * 8, v);
    }
}

// dy [N, H, W, C] (8 channels of one pixel per thread): a > 0 ? seed + routed dz : 0
template <typename T>
__global__ __launch_bounds__(NT) void pool_bwd_kernel(const T* __restrict__ a, const T* __restrict__ seed, const T* __restrict__ dz,
                                                      T* __restrict__ dy, int N, int H, int W, int C) {
    const int ho = H >> 1, wo = W >> 1, c8 = C / 8;
    const long long total = (long long)N * H * W * c8;
    for (long long i = gtid(); i < total; i += gsize()) {
        const int cv = (int)(i % c8);
        const long long pix = i / c8;
        const int n = (int)(pix / ((long long)H * W));
        const int yy = (int)((pix / W) % H), xx = (int)(pix % W);
        const V8<T> av = ld8(a + i * 8);
        float g[8];
        if (seed) {
            const V8<T> s = ld8(seed + i * 8);
#pragma unroll
            for (int k = 0; k < 8; ++k) g[k] = (float)s[k];
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) g[k] = 0.0f;
        }
        const int py = yy >> 1, px = xx >> 1;
        if (dz && py < ho && px < wo) {            // an odd last row / column is in no window
            const int me = (yy & 1) * 2 + (xx & 1);
            const T* w0 = a + (((long long)n * H + 2 * py) * W + 2 * px) * C + cv * 8;
            const V8<T> q0 = ld8(w0), q1 = ld8(w0 + C), q2 = ld8(w0 + (long long)W * C), q3 = ld8(w0 + (long long)W * C + C);
            const V8<T> dv = ld8(dz + (((long long)n * ho + py) * wo + px) * C + cv * 8);
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                int arg = 0;
                float m = (float)q0[k];
                if ((float)q1[k] > m) { m = (float)q1[k]; arg = 1; }
                if ((float)q2[k] > m) { m = (float)q2[k]; arg = 2; }
                if ((float)q3[k] > m) { arg = 3; }
                if (arg == me) g[k] += (float)dv[k];
            }
        }
        const V8<T> o = relu_mask<T>(av, g);
        st8(dy + i * 8, o);
    }
}

// block j of image b: 8192 / C pixels; G = C / 8 lanes per pixel, 8 channels each
template <typename T>
__global__ __launch_bounds__(NT) void head_fwd_kernel(const T* __restrict__ feat, const float* __restrict__ w, int B, int P, int C, int nblk,
                                                      float* __restrict__ partial) {
    __shared__ float red[NT];
    const int G = C / 8, NG = NT / G, ppb = HEAD_PASSES * NG;
    const int b = blockIdx.x / nblk, j = blockIdx.x % nblk;
    const int gi = threadIdx.x / G, li = threadIdx.x % G;
    const long long side = (long long)B * P * C;
    float wv[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) wv[k] = w[li * 8 + k];
    float acc = 0.0f;
    for (int pass = 0; pass < HEAD_PASSES; ++pass) {
        const long long q = (long long)j * ppb + pass * NG + gi;
        if (q >= P) break;                          // uniform per group
        const long long off = ((long long)b * P + q) * C + li * 8;
        const V8<T> fr = ld8(feat + off), ff = ld8(feat + side + off);
        float sr = 0.0f, sf = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) { sr += (float)fr[k] * (float)fr[k]; sf += (float)ff[k] * (float)ff[k]; }
        const float nr = sqrtf(group_sum(sr, G)) + 1e-10f, nf = sqrtf(group_sum(sf, G)) + 1e-10f;
        float d = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float e = (float)fr[k] / nr - (float)ff[k] / nf;
            d += e * e * wv[k];
        }
        acc += group_sum(d, G);
    }
    head_block_sum(acc, red, G, partial + blockIdx.x);
}

// one work-group per image
__global__ __launch_bounds__(NT) void finalize_kernel(const float* __restrict__ partial, Levels lv, int B, float* __restrict__ out) {
    __shared__ float red[NT];
    const int b = blockIdx.x, t = threadIdx.x;
    long long off = 0;
    float v = 0.0f;
    for (int l = 0; l < lv.n; ++l) {
        const int nb = lv.blocks[l];
        const float* p = partial + off + (long long)b * nb;
        float s = 0.0f;
        for (int j = t; j < nb; j += NT) s += p[j];
        red[t] = s;
        __syncthreads();
        for (int m = NT / 2; m > 0; m >>= 1) {
            if (t < m) red[t] += red[t + m];
            __syncthreads();
        }
        if (t == 0) v += red[0] / (float)lv.hw[l];
        __syncthreads();
        off += (long long)B * nb;
    }
    if (t == 0) out[b] = v;
}

// seed = d out / d (rec feature), every rec-side pixel of the level; G lanes per pixel
template <typename T>
__global__ __launch_bounds__(NT) void head_bwd_kernel(const T* __restrict__ feat, const float* __restrict__ w, int B, int P, int C,
                                                      const float* __restrict__ dout, T* __restrict__ seed) {
    const int G = C / 8, NG = NT / G;
    const long long npix = (long long)B * P;
    const long long side = npix * C;
    const int gi = threadIdx.x / G, li = threadIdx.x % G;
    float wv[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) wv[k] = w[li * 8 + k];
    for (long long pix = (long long)blockIdx.x * NG + gi; pix < npix; pix += (long long)gridDim.x * NG) {     // uniform per group
        const float coef = dout[pix / P] / (float)P;
        const long long off = pix * C + li * 8;
        const V8<T> fr = ld8(feat + off), ff = ld8(feat + side + off);
        float sr = 0.0f, sf = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) { sr += (float)fr[k] * (float)fr[k]; sf += (float)ff[k] * (float)ff[k]; }
        const float s = sqrtf(group_sum(sf, G));
        const float nr = sqrtf(group_sum(sr, G)) + 1e-10f, nf = s + 1e-10f;
        float g[8], gf = 0.0f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            g[k] = -2.0f * coef * wv[k] * ((float)fr[k] / nr - (float)ff[k] / nf);         // d / d (f_c / (|f| + eps))
            gf += g[k] * (float)ff[k];
        }
        gf = group_sum(gf, G);
        const float rad = s > 0.0f ? gf / (nf * nf * s) : 0.0f;      // |f| = 0: the 1 / |f| term is taken as 0 (torch: NaN)
        V8<T> o;
#pragma unroll
        for (int k = 0; k < 8; ++k) o[k] = (T)(g[k] / nf - (float)ff[k] * rad);
        st8(seed + off, o);
    }
}

bool head_c_ok(int C) { return C == 64 || C == 128 || C == 256 || C == 512; }

// check_img and this file's bound on the pixels of one image
int check_image(const MasFaceImage* im, const char* what) {
    if (int rc = check_img(im, what)) return rc;
    if ((long long)im->H * im->W > MAX_PIX) MAS_FAIL(MAS_EUNSUPPORTED, "%s: more than 2^30 pixels per image", what);
    return MAS_OK;
}

int check_map(int N, int H, int W, int C, int dtype, int min_side, const char* what) {
    if (N <= 0 || H < min_side || W < min_side || C <= 0 || C % 8 || !dt_ok(dtype))
        MAS_FAIL(MAS_EINVAL, "%s: N %d, H %d, W %d, C %d, dtype %d", what, N, H, W, C, dtype);
    if ((long long)H * W > MAX_PIX) MAS_FAIL(MAS_EUNSUPPORTED, "%s: more than 2^30 pixels per image", what);
    return MAS_OK;
}

int check_head(int B, int H, int W, int C, int dtype, const char* what) {
    if (int rc = check_map(B, H, W, 8, dtype, 1, what)) return rc;
    if (!head_c_ok(C)) MAS_FAIL(MAS_EINVAL, "%s: C %d is not one of 64, 128, 256, 512", what, C);
    return MAS_OK;
}

int head_blocks(int H, int W, int C) { return (int)(((long long)H * W + 8192 / C - 1) / (8192 / C)); }

}  // namespace

extern "C" int mas_lpips_pack_fwd(const MasFaceImage* real, const MasFaceImage* fake, const float* shift, const float* scale, void* canvas,
                                  int dtype, void* stream) {
    MAS_ENTER();
    if (int rc = check_image(real, "lpips_pack_fwd")) return rc;
    if (int rc = check_image(fake, "lpips_pack_fwd")) return rc;
    if (!shift || !scale || !canvas || !dt_ok(dtype)) MAS_FAIL(MAS_EINVAL, "lpips_pack_fwd: null argument or dtype %d", dtype);
    if (real->N != fake->N || real->H != fake->H || real->W != fake->W)
        MAS_FAIL(MAS_EINVAL, "lpips_pack_fwd: real [%d, 3, %d, %d] and fake [%d, 3, %d, %d] differ", real->N, real->H, real->W, fake->N, fake->H,
                 fake->W);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(grid_for(2LL * real->N * real->H * real->W));
    if (dtype == MAS_F32) hipLaunchKernelGGL(pack_fwd_kernel<float>, grid, dim3(NT), 0, s, *real, *fake, shift, scale, (float*)canvas);
    else hipLaunchKernelGGL(pack_fwd_kernel<bf16_t>, grid, dim3(NT), 0, s, *real, *fake, shift, scale, (bf16_t*)canvas);
    MAS_CHECK_LAUNCH("lpips_pack_fwd");
    return MAS_OK;
}

extern "C" int mas_lpips_pack_bwd(const void* dcanvas, int dtype, const float* scale, const MasFaceImage* dfake, void* stream) {
    MAS_ENTER();
    if (int rc = check_image(dfake, "lpips_pack_bwd")) return rc;
    if (!dcanvas || !scale || !dt_ok(dtype)) MAS_FAIL(MAS_EINVAL, "lpips_pack_bwd: null argument or dtype %d", dtype);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(grid_for((long long)dfake->N * dfake->H * dfake->W));
    if (dtype == MAS_F32) {
        if (dfake->dtype == MAS_F32) hipLaunchKernelGGL((pack_bwd_kernel<float, float>), grid, dim3(NT), 0, s, (const float*)dcanvas, scale, *dfake);
        else hipLaunchKernelGGL((pack_bwd_kernel<float, bf16_t>), grid, dim3(NT), 0, s, (const float*)dcanvas, scale, *dfake);
    } else {
        if (dfake->dtype == MAS_F32) hipLaunchKernelGGL((pack_bwd_kernel<bf16_t, float>), grid, dim3(NT), 0, s, (const bf16_t*)dcanvas, scale, *dfake);
        else hipLaunchKernelGGL((pack_bwd_kernel<bf16_t, bf16_t>), grid, dim3(NT), 0, s, (const bf16_t*)dcanvas, scale, *dfake);
    }
    MAS_CHECK_LAUNCH("lpips_pack_bwd");
    return MAS_OK;
}

extern "C" int mas_lpips_relu_fwd(void* y, long long n, int dtype, void* stream) {
    MAS_ENTER();
    if (!y || n <= 0 || n % 8 || !dt_ok(dtype)) MAS_FAIL(MAS_EINVAL, "lpips_relu_fwd: bad argument (n %lld, dtype %d)", n, dtype);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(grid_for(n / 8));
    if (dtype == MAS_F32) hipLaunchKernelGGL(relu_fwd_kernel<float>, grid, dim3(NT), 0, s, (float*)y, n / 8);
    else hipLaunchKernelGGL(relu_fwd_kernel<bf16_t>, grid, dim3(NT), 0, s, (bf16_t*)y, n / 8);
    MAS_CHECK_LAUNCH("lpips_relu_fwd");
    return MAS_OK;
}

extern "C" int mas_lpips_pool_fwd(const void* x, void* y, int N, int H, int W, int C, int dtype, void* stream) {
    MAS_ENTER();
    if (int rc = check_map(N, H, W, C, dtype, 2, "lpips_pool_fwd")) return rc;
    if (!x || !y) MAS_FAIL(MAS_EINVAL, "lpips_pool_fwd: null tensor");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(grid_for((long long)N * (H / 2) * (W / 2) * (C / 8)));
    if (dtype == MAS_F32) hipLaunchKernelGGL(pool_fwd_kernel<float>, grid, dim3(NT), 0, s, (const float*)x, (float*)y, N, H, W, C);
    else hipLaunchKernelGGL(pool_fwd_kernel<bf16_t>, grid, dim3(NT), 0, s, (const bf16_t*)x, (bf16_t*)y, N, H, W, C);
    MAS_CHECK_LAUNCH("lpips_pool_fwd");
    return MAS_OK;
}

extern "C" int mas_lpips_pool_bwd(const void* a, const void* seed, const void* dz, void* dy, int N, int H, int W, int C, int dtype,
                                  void* stream) {
    MAS_ENTER();
    if (int rc = check_map(N, H, W, C, dtype, 1, "lpips_pool_bwd")) return rc;
    if (!a || !dy) MAS_FAIL(MAS_EINVAL, "lpips_pool_bwd: null tensor");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(grid_for((long long)N * H * W * (C / 8)));
    if (dtype == MAS_F32)
        hipLaunchKernelGGL(pool_bwd_kernel<float>, grid, dim3(NT), 0, s, (const float*)a, (const float*)seed, (const float*)dz, (float*)dy, N, H, W, C);
    else
        hipLaunchKernelGGL(pool_bwd_kernel<bf16_t>, grid, dim3(NT), 0, s, (const bf16_t*)a, (const bf16_t*)seed, (const bf16_t*)dz, (bf16_t*)dy, N, H,
                           W, C);
    MAS_CHECK_LAUNCH("lpips_pool_bwd");
    return MAS_OK;
}

extern "C" int mas_lpips_head_blocks(int H, int W, int C) {
    if (int rc = check_head(1, H, W, C, MAS_F32, "lpips_head_blocks")) return rc;
    return head_blocks(H, W, C);
}

extern "C" int mas_lpips_head_fwd(const void* feat, const float* w, int B, int H, int W, int C, int dtype, float* partial, void* stream) {
    MAS_ENTER();
    if (int rc = check_head(B, H, W, C, dtype, "lpips_head_fwd")) return rc;
    if (!feat || !w || !partial) MAS_FAIL(MAS_EINVAL, "lpips_head_fwd: null argument");
    const int nblk = head_blocks(H, W, C);
    if (nblk > MAX_BLOCKS || (long long)B * nblk > 0x7fffffffLL) MAS_FAIL(MAS_EUNSUPPORTED, "lpips_head_fwd: %d images of %d blocks", B, nblk);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(B * nblk);
    if (dtype == MAS_F32) hipLaunchKernelGGL(head_fwd_kernel<float>, grid, dim3(NT), 0, s, (const float*)feat, w, B, H * W, C, nblk, partial);
    else hipLaunchKernelGGL(head_fwd_kernel<bf16_t>, grid, dim3(NT), 0, s, (const bf16_t*)feat, w, B, H * W, C, nblk, partial);
    MAS_CHECK_LAUNCH("lpips_head_fwd");
    return MAS_OK;
}

extern "C" int mas_lpips_finalize(const float* partial, int B, int n_levels, const int32_t* hw, const int32_t* blocks, float* out, void* stream) {
    MAS_ENTER();
    if (!partial || !hw || !blocks || !out || B <= 0 || n_levels < 1 || n_levels > MAX_LEVELS)
        MAS_FAIL(MAS_EINVAL, "lpips_finalize: null argument, B %d or %d levels", B, n_levels);
    Levels lv;
    memset(&lv, 0, sizeof(lv));
    lv.n = n_levels;
    for (int l = 0; l < n_levels; ++l) {
        if (hw[l] < 1 || blocks[l] < 1) MAS_FAIL(MAS_EINVAL, "lpips_finalize: level %d has %d pixels in %d blocks", l, hw[l], blocks[l]);
        if (blocks[l] > MAX_BLOCKS) MAS_FAIL(MAS_EUNSUPPORTED, "lpips_finalize: level %d has %d blocks (> 2^18)", l, blocks[l]);
        lv.hw[l] = hw[l];
        lv.blocks[l] = blocks[l];
    }
    hipLaunchKernelGGL(finalize_kernel, dim3(B), dim3(NT), 0, reinterpret_cast<hipStream_t>(stream), partial, lv, B, out);
    MAS_CHECK_LAUNCH("lpips_finalize");
    return MAS_OK;
}

extern "C" int mas_lpips_head_bwd(const void* feat, const float* w, int B, int H, int W, int C, int dtype, const float* dout, void* seed,
                                  void* stream) {
    MAS_ENTER();
    if (int rc = check_head(B, H, W, C, dtype, "lpips_head_bwd")) return rc;
    if (!feat || !w || !dout || !seed) MAS_FAIL(MAS_EINVAL, "lpips_head_bwd: null argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(grid_for((long long)B * H * W * (C / 8)));
    if (dtype == MAS_F32) hipLaunchKernelGGL(head_bwd_kernel<float>, grid, dim3(NT), 0, s, (const float*)feat, w, B, H * W, C, dout, (float*)seed);
    else hipLaunchKernelGGL(head_bwd_kernel<bf16_t>, grid, dim3(NT), 0, s, (const bf16_t*)feat, w, B, H * W, C, dout, (bf16_t*)seed);
    MAS_CHECK_LAUNCH("lpips_head_bwd");
    return MAS_OK;
}
