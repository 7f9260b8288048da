// The VQ-IMG read-out: float images to uint8 pictures, squared error and SSIM between two pictures, codebook usage counts.
//   * img_bytes: x [N, C, H, W] fp32 or bf16, dense NCHW or dense NHWC, read in place and once -> picture uint8 [N, H, W, C].  Per element,
//        in fp32 with every operation rounded on its own (no fused multiply-add):  t = (x - lo) * s,  s = float32(255 / (hi - lo));
//        t = fmin(fmax(t, 0), 255) (a NaN becomes 0);  byte = rint(t), half to even.  NHWC is one flat array: 16-byte units from the first
//        16-byte boundary of x, head and tail one by one.  NCHW: a lane owns V consecutive pixels (one 16-byte unit of every channel row
//        where the rows are 16-byte aligned, one pixel otherwise) and writes their V C interleaved bytes as dwords.
//   * img_agreement: two pictures -> sse[N] (integers: exact in any order) and one fp64 partial sum of the SSIM map per tile.  A tile is
//        T x T window positions of one image (T = MAS_IMG_SSIM_TILE); the work-group stages the tile and its 10-pixel halo of both
//        pictures in LDS as doubles, one channel at a time, runs the 11-tap window horizontally on {a, b, a a, b b, a b}, then vertically,
//        and every lane forms the map value of its position, all in fp64 (fp32 sums are wrong by up to 7e-5 on flat bright pictures:
//        the weights do not sum to 1, so the variance of a constant is not 0).  Every pixel belongs to exactly one tile (the last tile of
//        a row or column also owns its halo), which is where its squared error is counted: one 64-bit integer atomic per work-group and
//        image.  A tile's map sum is a tree over the lanes in a fixed order, and img_agreement_reduce adds an image's tiles in a fixed
//        order: the same pictures give the same bits, whatever the grid.  Nothing outside a picture is read: the halo is cut at the edge.
//   * code_usage: indices (int64 or int32) -> counts[K + 1] ADDED to the caller's buffer, counts[K] = the indices outside [0, K).  The
//        range check comes before any indexing.  A work-group histogram in LDS (32-bit bins, one 64-bit atomic per non-zero bin at the
//        end) while K + 1 <= MAS_CODE_USAGE_LDS_BINS, global 64-bit integer atomics beyond.
// Grids depend on the shape and the CU count only; 64-bit offsets; no float atomics; nothing allocates or synchronises with the host.
#include "mas_common.h"
#include "seg_elem.h"     // ld_n, aligned_to
#include <math.h>

namespace {

constexpr int NT = SEG_NT;
constexpr int T = MAS_IMG_SSIM_TILE;
constexpr int WIN = MAS_IMG_SSIM_WINDOW;
constexpr int R = T + WIN - 1;                          // edge of a tile with its halo, in pixels
constexpr int PITCH = 48;                               // doubles per staged row: two rows of a 32-lane ds_read_b64 group, 16 lanes each, are 96
                                                        // dwords apart = half the 64 banks, so the group covers every bank once
static_assert(PITCH >= R && PITCH % 32 == 16, "row pitch of the staged tile");
constexpr int MAXC = MAS_IMG_MAX_CHANNELS;
constexpr int LDS_BINS = MAS_CODE_USAGE_LDS_BINS;
static_assert(T * T == NT, "one window position per lane");
typedef unsigned char u8_t;

// ---- bytes ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned to_byte(float x, float lo, float s) {
#pragma clang fp contract(off)
    float t = (x - lo) * s;                             // two roundings: what the numpy restatement does
    t = fminf(fmaxf(t, 0.0f), 255.0f);                  // (fmaxf returns the operand that is not a NaN)
    return (unsigned)rintf(t);
}

struct BArgs {
    const void* x;
    u8_t* out;
    long long units;                                    // NCHW: lanes' work items; NHWC: elements
    unsigned HW, upi;                                   // NCHW: units per image
    float lo, s;
};

template <typename PT>
__global__ __launch_bounds__(NT) void img_bytes_flat_kernel(const BArgs A) {
    constexpr int U = 16 / (int)sizeof(PT);
    const PT* x = (const PT*)A.x;
    const long long n = A.units;
    long long head = (long long)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(x) & 15)) & 15) / sizeof(PT));
    if (head > n) head = n;
    const long long nunits = (n - head) / U, tail0 = head + nunits * U;
    const bool out_vec = aligned_to(A.out + head, U);   // the U bytes of a unit as one store
    const long long gtid = (long long)blockIdx.x * NT + threadIdx.x, gstride = (long long)gridDim.x * NT;
    if (gtid < head) A.out[gtid] = (u8_t)to_byte(to_f(x[gtid]), A.lo, A.s);
    if (gtid < n - tail0) A.out[tail0 + gtid] = (u8_t)to_byte(to_f(x[tail0 + gtid]), A.lo, A.s);
    for (long long q = gtid; q < nunits; q += gstride) {
        const long long e = head + q * U;
        float v[U];
        ld_n<PT, U>(x + e, true, v);
        unsigned w[U / 4];
#pragma unroll
        for (int k = 0; k < U / 4; ++k)
            w[k] = to_byte(v[4 * k], A.lo, A.s) | (to_byte(v[4 * k + 1], A.lo, A.s) << 8) | (to_byte(v[4 * k + 2], A.lo, A.s) << 16) |
                   (to_byte(v[4 * k + 3], A.lo, A.s) << 24);
        if (out_vec) {
            if constexpr (U == 8) *reinterpret_cast<u32x2*>(A.out + e) = u32x2{w[0], w[1]};
            else *reinterpret_cast<unsigned*>(A.out + e) = w[0];
        } else {
#pragma unroll
            for (int i = 0; i < U; ++i) A.out[e + i] = (u8_t)(w[i / 4] >> (8 * (i % 4)));
        }
    }
}

// V = pixels per lane: 16 / sizeof(PT) (HW % V == 0, x 16-byte and out 4-byte aligned: V C is a multiple of 4) or 1
template <typename PT, int V, int C>
__global__ __launch_bounds__(NT) void img_bytes_nchw_kernel(const BArgs A) {
    const unsigned HW = A.HW;
    for (long long u = (long long)blockIdx.x * NT + threadIdx.x; u < A.units; u += (long long)gridDim.x * NT) {
        const long long img = u / A.upi;
        const unsigned p0 = (unsigned)(u - img * A.upi) * V;
        const PT* xr = (const PT*)A.x + (img * C) * (long long)HW + p0;
        u8_t* ob = A.out + (img * HW + p0) * (long long)C;
        unsigned b[V * C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            float v[V];
            ld_n<PT, V>(xr + (long long)c * HW, true, v);
#pragma unroll
            for (int i = 0; i < V; ++i) b[i * C + c] = to_byte(v[i], A.lo, A.s);
        }
        if constexpr (V == 1) {
#pragma unroll
            for (int c = 0; c < C; ++c) ob[c] = (u8_t)b[c];
        } else {
#pragma unroll
            for (int k = 0; k < V * C / 4; ++k)
                reinterpret_cast<unsigned*>(ob)[k] = b[4 * k] | (b[4 * k + 1] << 8) | (b[4 * k + 2] << 16) | (b[4 * k + 3] << 24);
        }
    }
}

// ---- squared error and SSIM ---------------------------------------------------------------------------------------------------------
struct GArgs {
    const u8_t* a; const u8_t* b;
    unsigned long long* sse;                            // [N]
    double* partials;                                   // [N][ty][tx]
    double g[WIN];
    long long tiles;
    int C, H, W, ty, tx;                                // tiles of an image: ty x tx
};

__global__ __launch_bounds__(NT) void img_agreement_kernel(const GArgs A) {
    __shared__ double s_a[R][PITCH], s_b[R][PITCH];     // one channel of the tile and its halo, zero past the picture's edge
    __shared__ double s_h[5][R][T];                     // after the horizontal pass: {a, b, a a, b b, a b}
    __shared__ double s_red[NT];
    __shared__ unsigned s_sse;
    const int tid = threadIdx.x, lx = tid % T, ly = tid / T;
    const int C = A.C, H = A.H, W = A.W;
    const long long tpi = (long long)A.ty * A.tx;
    const double C1 = (0.01 * 255.0) * (0.01 * 255.0), C2 = (0.03 * 255.0) * (0.03 * 255.0);
    unsigned long long acc = 0;                         // lane 0: the squared error of image acc_img, not yet added to sse
    long long acc_img = -1;
    for (long long t = blockIdx.x; t < A.tiles; t += gridDim.x) {
        const long long img = t / tpi;
        const int tr = (int)(t - img * tpi), tyi = tr / A.tx, txi = tr - tyi * A.tx;
        const int y0 = tyi * T, x0 = txi * T;
        const int rh = H - y0 < R ? H - y0 : R, rw = W - x0 < R ? W - x0 : R;          // the staged region, cut at the picture's edge
        const int oh = tyi == A.ty - 1 ? rh : T, ow = txi == A.tx - 1 ? rw : T;        // the pixels this tile owns
        const bool valid = y0 + ly < H - (WIN - 1) && x0 + lx < W - (WIN - 1);         // this lane's window lies inside the picture
        const long long base = ((img * H + y0) * (long long)W + x0) * C;
        if (tid == 0) s_sse = 0;
        unsigned sq = 0;
        double map_sum = 0.0;
        for (int c = 0; c < C; ++c) {
            __syncthreads();                            // the previous channel (or tile) has been read
            for (int e = tid; e < R * R; e += NT) {
                const int r = e / R, q = e - r * R;
                int va = 0, vb = 0;
                if (r < rh && q < rw) {
                    const long long off = base + ((long long)r * W + q) * C + c;
                    va = A.a[off]; vb = A.b[off];
                    if (r < oh && q < ow) sq += (unsigned)((va - vb) * (va - vb));
                }
                s_a[r][q] = (double)va; s_b[r][q] = (double)vb;
            }
            __syncthreads();
            for (int e = tid; e < R * T; e += NT) {
                const int r = e / T, q = e - r * T;
                double ha = 0.0, hb = 0.0, haa = 0.0, hbb = 0.0, hab = 0.0;
#pragma unroll
                for (int i = 0; i < WIN; ++i) {
                    const double va = s_a[r][q + i], vb = s_b[r][q + i], w = A.g[i];
                    ha = fma(w, va, ha); hb = fma(w, vb, hb);
                    haa = fma(w, va * va, haa); hbb = fma(w, vb * vb, hbb); hab = fma(w, va * vb, hab);   // (byte products: exact)
                }
                s_h[0][r][q] = ha; s_h[1][r][q] = hb; s_h[2][r][q] = haa; s_h[3][r][q] = hbb; s_h[4][r][q] = hab;
            }
            __syncthreads();
            if (valid) {
                double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int j = 0; j < WIN; ++j) {
                    const double w = A.g[j];
#pragma unroll
                    for (int k = 0; k < 5; ++k) m[k] = fma(w, s_h[k][ly + j][lx], m[k]);
                }
                const double mab = m[0] * m[1], maa = m[0] * m[0], mbb = m[1] * m[1];
                const double va = m[2] - maa, vb = m[3] - mbb, vab = m[4] - mab;
                map_sum += ((2.0 * mab + C1) * (2.0 * vab + C2)) / ((maa + mbb + C1) * (va + vb + C2));
            }
        }
        s_red[tid] = map_sum;                           // (0 for a lane without a window)
        if (sq) atomicAdd(&s_sse, sq);                  // (a tile's sum: at most R R C 255^2 < 2^28)
        __syncthreads();
        for (int o = NT / 2; o >= 1; o >>= 1) {
            if (tid < o) s_red[tid] += s_red[tid + o];
            __syncthreads();
        }
        if (tid == 0) {
            A.partials[t] = s_red[0];
            if (img != acc_img) {
                if (acc) atomicAdd(A.sse + acc_img, acc);
                acc = 0; acc_img = img;
            }
            acc += s_sse;
        }
    }
    if (tid == 0 && acc) atomicAdd(A.sse + acc_img, acc);
}

// one work-group per image: its tiles in a fixed order, over the number of map values; NaN for a picture smaller than the window
__global__ __launch_bounds__(NT) void img_agreement_reduce_kernel(const double* __restrict__ partials, long long tpi, double inv_count,
                                                                  double* __restrict__ ssim) {
    __shared__ double s_red[NT];
    const int tid = threadIdx.x;
    const double* p = partials + (long long)blockIdx.x * tpi;
    double s = 0.0;
    for (long long i = tid; i < tpi; i += NT) s += p[i];
    s_red[tid] = s;
    __syncthreads();
    for (int o = NT / 2; o >= 1; o >>= 1) {
        if (tid < o) s_red[tid] += s_red[tid + o];
        __syncthreads();
    }
    if (tid == 0) ssim[blockIdx.x] = inv_count > 0.0 ? s_red[0] * inv_count : __builtin_nan("");
}

// ---- codebook usage -----------------------------------------------------------------------------------------------------------------
template <typename IT, bool LDS>
__global__ __launch_bounds__(NT) void code_usage_kernel(const IT* __restrict__ idx, long long n, int K, unsigned long long* __restrict__ counts) {
    extern __shared__ unsigned s_bins[];                // [K + 1] (LDS)
    const int tid = threadIdx.x;
    if constexpr (LDS) {
        for (int i = tid; i <= K; i += NT) s_bins[i] = 0;
        __syncthreads();
    }
    for (long long i = (long long)blockIdx.x * NT + tid; i < n; i += (long long)gridDim.x * NT) {
        const IT v = idx[i];
        const int bin = v >= 0 && v < (IT)K ? (int)v : K;            // the check first: nothing below indexes outside [0, K]
        if constexpr (LDS) atomicAdd(&s_bins[bin], 1u);
        else atomicAdd(counts + bin, 1ull);
    }
    if constexpr (LDS) {
        __syncthreads();
        for (int i = tid; i <= K; i += NT) {
            const unsigned v = s_bins[i];
            if (v) atomicAdd(counts + i, (unsigned long long)v);
        }
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
int img_shape(const char* what, int N, int C, int H, int W) {
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0) MAS_FAIL(MAS_EINVAL, "%s: empty shape [%d, %d, %d, %d]", what, N, C, H, W);
    if (C > MAXC) MAS_FAIL(MAS_EUNSUPPORTED, "%s: %d channels (1 .. %d)", what, C, MAXC);
    if ((long long)H * W > (1LL << 30)) MAS_FAIL(MAS_EUNSUPPORTED, "%s: H W = %lld > 2^30", what, (long long)H * W);
    if ((double)N * C * (double)H * (double)W > 4e18) MAS_FAIL(MAS_EUNSUPPORTED, "%s: more than 4e18 elements", what);
    return MAS_OK;
}

inline int tiles_of(int extent) { const int p = extent - (WIN - 1); return p <= 0 ? 1 : (p + T - 1) / T; }

template <typename PT, int V>
void bytes_nchw_go(int C, dim3 grid, hipStream_t s, const BArgs& A) {
    switch (C) {
        case 1: hipLaunchKernelGGL((img_bytes_nchw_kernel<PT, V, 1>), grid, dim3(NT), 0, s, A); break;
        case 2: hipLaunchKernelGGL((img_bytes_nchw_kernel<PT, V, 2>), grid, dim3(NT), 0, s, A); break;
        case 3: hipLaunchKernelGGL((img_bytes_nchw_kernel<PT, V, 3>), grid, dim3(NT), 0, s, A); break;
        default: hipLaunchKernelGGL((img_bytes_nchw_kernel<PT, V, 4>), grid, dim3(NT), 0, s, A); break;
    }
}

}  // namespace

extern "C" int mas_img_bytes(const void* x, int x_dtype, int x_layout, int N, int C, int H, int W, double lo, double hi, unsigned char* out,
                             void* stream) {
    MAS_ENTER();
    const char* what = "img_bytes";
    if (!x || !out) MAS_FAIL(MAS_EINVAL, "%s: null argument", what);
    if (int rc = img_shape(what, N, C, H, W)) return rc;
    if (x_dtype != MAS_F32 && x_dtype != MAS_BF16) MAS_FAIL(MAS_EUNSUPPORTED, "%s: dtype %d (fp32 / bf16)", what, x_dtype);
    if (x_layout != MAS_SEG_NCHW && x_layout != MAS_SEG_NHWC) MAS_FAIL(MAS_EINVAL, "%s: layout code %d (MAS_SEG_NCHW or MAS_SEG_NHWC)", what, x_layout);
    if (!isfinite(lo) || !isfinite(hi) || !(lo < hi)) MAS_FAIL(MAS_EINVAL, "%s: the range [%g, %g] must be finite with lo < hi", what, lo, hi);
    const size_t xe = mas_esize(x_dtype);
    if (reinterpret_cast<uintptr_t>(x) % xe) MAS_FAIL(MAS_EINVAL, "%s: the image is not aligned to its element size", what);
    BArgs A;
    memset(&A, 0, sizeof(A));
    const long long hw = (long long)H * W;
    A.x = x; A.out = out; A.HW = (unsigned)hw;
    A.lo = (float)lo; A.s = (float)(255.0 / (hi - lo));
    const long long cap = (long long)mas_num_cus() * 8;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (x_layout == MAS_SEG_NHWC || C == 1) {                        // (one channel: the two layouts are the same memory)
        A.units = (long long)N * C * hw;
        const long long need = (A.units / (16 / (long long)xe) + NT - 1) / NT + 1;
        const dim3 grid((unsigned)(need < cap ? need : cap)), block(NT);
        if (x_dtype == MAS_BF16) hipLaunchKernelGGL((img_bytes_flat_kernel<bf16_t>), grid, block, 0, s, A);
        else hipLaunchKernelGGL((img_bytes_flat_kernel<float>), grid, block, 0, s, A);
    } else {
        const int vu = 16 / (int)xe;
        const bool vec = hw % vu == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0;
        A.upi = (unsigned)(vec ? hw / vu : hw);
        A.units = (long long)N * A.upi;
        const long long need = (A.units + NT - 1) / NT;
        const dim3 grid((unsigned)(need < cap ? need : cap));
        if (x_dtype == MAS_BF16) { if (vec) bytes_nchw_go<bf16_t, 8>(C, grid, s, A); else bytes_nchw_go<bf16_t, 1>(C, grid, s, A); }
        else { if (vec) bytes_nchw_go<float, 4>(C, grid, s, A); else bytes_nchw_go<float, 1>(C, grid, s, A); }
    }
    MAS_CHECK_LAUNCH(what);
    return MAS_OK;
}

extern "C" int mas_img_agreement_blocks(int N, int C, int H, int W) {
    if (int rc = img_shape("img_agreement_blocks", N, C, H, W)) return rc;
    const long long tiles = (long long)N * tiles_of(H) * tiles_of(W);
    if (tiles > 0x7fffffffLL) MAS_FAIL(MAS_EUNSUPPORTED, "img_agreement_blocks: %lld tiles > 2^31 - 1", tiles);
    return (int)tiles;
}

extern "C" int mas_img_agreement(const unsigned char* a, const unsigned char* b, int N, int C, int H, int W, const double* window,
                                 long long* sse, double* partials, int n_partials, void* stream) {
    MAS_ENTER();
    const char* what = "img_agreement";
    if (!a || !b || !window || !sse || !partials) MAS_FAIL(MAS_EINVAL, "%s: null argument", what);
    const int tiles = mas_img_agreement_blocks(N, C, H, W);
    if (tiles < 0) return tiles;
    if (n_partials != tiles) MAS_FAIL(MAS_EWORKSPACE, "%s: partials holds %d sums, mas_img_agreement_blocks says %d", what, n_partials, tiles);
    if (reinterpret_cast<uintptr_t>(sse) % 8 || reinterpret_cast<uintptr_t>(partials) % 8)
        MAS_FAIL(MAS_EINVAL, "%s: sse / partials not aligned to 8 bytes", what);
    GArgs A;
    memset(&A, 0, sizeof(A));
    A.a = a; A.b = b; A.sse = reinterpret_cast<unsigned long long*>(sse); A.partials = partials;
    for (int i = 0; i < WIN; ++i) {
        if (!isfinite(window[i])) MAS_FAIL(MAS_EINVAL, "%s: window[%d] is not finite", what, i);
        A.g[i] = window[i];
    }
    A.tiles = tiles; A.C = C; A.H = H; A.W = W; A.ty = tiles_of(H); A.tx = tiles_of(W);
    const long long cap = (long long)mas_num_cus() * 8;
    const dim3 grid((unsigned)(tiles < cap ? tiles : cap)), block(NT);
    hipLaunchKernelGGL(img_agreement_kernel, grid, block, 0, reinterpret_cast<hipStream_t>(stream), A);
    MAS_CHECK_LAUNCH(what);
    return MAS_OK;
}

extern "C" int mas_img_agreement_reduce(const double* partials, int n_partials, int N, int C, int H, int W, double* ssim, void* stream) {
    MAS_ENTER();
    const char* what = "img_agreement_reduce";
    if (!partials || !ssim) MAS_FAIL(MAS_EINVAL, "%s: null argument", what);
    const int tiles = mas_img_agreement_blocks(N, C, H, W);
    if (tiles < 0) return tiles;
    if (n_partials != tiles) MAS_FAIL(MAS_EWORKSPACE, "%s: partials holds %d sums, mas_img_agreement_blocks says %d", what, n_partials, tiles);
    const bool any = H >= WIN && W >= WIN;
    const double inv_count = any ? 1.0 / ((double)C * (double)(H - (WIN - 1)) * (double)(W - (WIN - 1))) : 0.0;
    hipLaunchKernelGGL(img_agreement_reduce_kernel, dim3((unsigned)N), dim3(NT), 0, reinterpret_cast<hipStream_t>(stream), partials,
                       (long long)(tiles / N), inv_count, ssim);
    MAS_CHECK_LAUNCH(what);
    return MAS_OK;
}

extern "C" int mas_code_usage(const void* indices, int index_bytes, long long n, int K, long long* counts, void* stream) {
    MAS_ENTER();
    const char* what = "code_usage";
    if (!indices || !counts) MAS_FAIL(MAS_EINVAL, "%s: null argument", what);
    if (index_bytes != 4 && index_bytes != 8) MAS_FAIL(MAS_EINVAL, "%s: indices of %d bytes (int32: 4, int64: 8)", what, index_bytes);
    if (n <= 0 || K <= 0) MAS_FAIL(MAS_EINVAL, "%s: n = %lld indices, K = %d codes must be positive", what, n, K);
    if (K > 0x7ffffffe) MAS_FAIL(MAS_EUNSUPPORTED, "%s: K = %d > 2^31 - 2", what, K);
    if (n > 0xffffffffLL) MAS_FAIL(MAS_EUNSUPPORTED, "%s: n = %lld > 2^32 - 1 (a work-group's bins are 32 bits wide)", what, n);
    if (reinterpret_cast<uintptr_t>(indices) % index_bytes || reinterpret_cast<uintptr_t>(counts) % 8)
        MAS_FAIL(MAS_EINVAL, "%s: indices / counts not aligned to their element size", what);
    const bool lds = K + 1 <= LDS_BINS;
    // a work-group zeroes and flushes K + 1 bins: give it at least 16 indices per lane before another one starts
    const long long cap = (long long)mas_num_cus() * 4, need = (n + 16 * NT - 1) / (16 * NT);
    const dim3 grid((unsigned)(need < cap ? need : cap)), block(NT);
    const size_t smem = lds ? (size_t)(K + 1) * sizeof(unsigned) : 0;
    unsigned long long* c = reinterpret_cast<unsigned long long*>(counts);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (index_bytes == 8) {
        if (lds) hipLaunchKernelGGL((code_usage_kernel<long long, true>), grid, block, smem, s, (const long long*)indices, n, K, c);
        else hipLaunchKernelGGL((code_usage_kernel<long long, false>), grid, block, 0, s, (const long long*)indices, n, K, c);
    } else {
        if (lds) hipLaunchKernelGGL((code_usage_kernel<int, true>), grid, block, smem, s, (const int*)indices, n, K, c);
        else hipLaunchKernelGGL((code_usage_kernel<int, false>), grid, block, 0, s, (const int*)indices, n, K, c);
    }
    MAS_CHECK_LAUNCH(what);
    return MAS_OK;
}
