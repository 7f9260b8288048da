// The object-aware term of the VQ-IMG loss (Make-A-Scene section 3.2) on gfx950: LPIPS-VGG16 on every object crop of the batch at
// once, laid out as an "atlas".
//
// Every used crop sits at a 16-aligned origin of an NHWC canvas with a zero gutter of >= 16 px after it; real and rec crops take the
// same places in two canvas images.  Each 3x3 convolution of VGG16 then runs ONCE per layer for the whole batch on the library's
// convolution kernels (mas_conv_fwd); this file holds everything else:
//   crop -> canvas with the ScalingLayer applied (a box pixel outside the image is (0 - shift) / scale, as torchvision's zero-padding
//     crop feeds it to the ScalingLayer), and its adjoint as a gather into d rec (overlapping boxes summed in box order);
//   the ReLU + mask pass after every convolution: outside the valid rectangle of each crop at level l (origin >> l, size h >> l) the
//     map is 0, so the gutter supplies exactly the zero padding an isolated crop would see and the extra pooled row / column of odd
//     sizes disappears (16-alignment keeps every 2x2 window of a valid output inside one crop); its backward;
//   the masked 2x2 / stride-2 max-pool and its backward (first maximum of the window, torch's tie rule; the ReLU mask of the level
//     below and the head's gradient seed folded in);
//   the LPIPS head per level (channel normalisation of both sides, squared difference, lin<k> weights, per-crop fixed-order partial
//     sums), one finalize launch for the crops' values and the loss, and the head's backward for the rec side.
// Activations are bf16 or fp32; arithmetic in fp32; no float atomics anywhere (bitwise repeatable).
#include "lpips_core.h"

namespace {

constexpr int LEVELS = 5;

// the cell whose level-l valid rectangle holds pixel (y, x) of canvas n, or -1
__device__ __forceinline__ int cell_at(const MasObjPlan& p, int n, int y, int x, int l) {
    const int sh = 4 - l;
    const int t = p.tiles[((long long)n * (p.H >> 4) + (y >> sh)) * (p.W >> 4) + (x >> sh)];
    if (t < 0) return -1;
    const MasObjCell c = p.cells[t];
    const int cy = y - (c.oy >> l), cx = x - (c.ox >> l);
    return (cy >= 0 && cy < (c.h >> l) && cx >= 0 && cx < (c.w >> l)) ? t : -1;
}

// What a kernel is told about the atlas -- every kernel body below is written once, over either:
//   ListTab: the plan of one call, as the host made it: n_cells by value, blk0 rows of n_cells + 1, a grid cut to the boxes;
//   DevTab : a table of FIXED capacity that the host rewrites between calls (mas_obj_*_dev): n_cells is read from the table's header, blk0
//     rows are max_cells + 1 apart, the head runs on a grid that bounds every table, partial has fixed per-level offsets, and a header
//     outside [0, max_cells] makes every work-group return.  Its p holds the pointers into the table and the canvas geometry.
struct ListTab {
    static constexpr bool FIXED_GRID = false;
    MasObjPlan p;
    __device__ __forceinline__ bool ok() const { return true; }
    __device__ __forceinline__ int n_cells() const { return p.n_cells; }
    __device__ __forceinline__ int blk_stride() const { return p.n_cells + 1; }
    __device__ __forceinline__ int out_cells() const { return p.n_cells; }
    __device__ __forceinline__ int part_off(int) const { return 0; }
};

struct DevTab {
    static constexpr bool FIXED_GRID = true;
    MasObjPlan p;                              // (p.n_cells is not used: the table's header says it)
    const int32_t* header;
    int max_cells;
    int off[LEVELS];                           // first partial of every level: the prefix sums of the fixed grids
    __device__ __forceinline__ bool ok() const { const int n = header[0]; return n >= 0 && n <= max_cells; }
    __device__ __forceinline__ int n_cells() const { return header[0]; }
    __device__ __forceinline__ int blk_stride() const { return max_cells + 1; }
    __device__ __forceinline__ int out_cells() const { return max_cells; }
    __device__ __forceinline__ int part_off(int l) const { return off[l]; }
};

// one thread per canvas pixel: CP channels
template <typename T, typename Tab>
__global__ __launch_bounds__(NT) void canvas_fwd_kernel(MasFaceImage img, MasFaceImage rec, Tab tab, const float* __restrict__ shift,
                                                        const float* __restrict__ scale, T* __restrict__ out) {
    if (!tab.ok()) return;
    const MasObjPlan& p = tab.p;
    const long long hw = (long long)p.H * p.W;
    const long long total = 2LL * p.n_canvas * hw;
    const float s0 = shift[0], s1 = shift[1], s2 = shift[2], k0 = scale[0], k1 = scale[1], k2 = scale[2];
    for (long long i = gtid(); i < total; i += gsize()) {
        const int n = (int)(i / hw);
        const int side = n >= p.n_canvas ? 1 : 0;
        const int y = (int)((i % hw) / p.W), x = (int)(i % p.W);
        V8<T> v = zero8<T>();
        const int t = cell_at(p, n - side * p.n_canvas, y, x, 0);
        if (t >= 0) {
            const MasObjCell c = p.cells[t];
            const MasFaceImage& im = side ? rec : img;
            const int iy = c.top + y - c.oy, ix = c.left + x - c.ox;
            float px[3] = {0.0f, 0.0f, 0.0f};
            if (c.b < im.N && iy >= 0 && iy < im.H && ix >= 0 && ix < im.W) {
                const long long base = (long long)c.b * im.sn + (long long)iy * im.sh + (long long)ix * im.sw;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) px[ch] = ld_img(im, base + ch * im.sc);
            }
            v[0] = (T)((px[0] - s0) / k0);
            v[1] = (T)((px[1] - s1) / k1);
            v[2] = (T)((px[2] - s2) / k2);
        }
        st8(out + i * CP, v);
    }
}

// one thread per pixel of d rec: the cells of its image in table order
template <typename TD, typename TR, typename Tab>
__global__ __launch_bounds__(NT) void canvas_bwd_kernel(const TD* __restrict__ dcan, Tab tab, const float* __restrict__ scale,
                                                        MasFaceImage drec) {
    if (!tab.ok()) return;
    const MasObjPlan& p = tab.p;
    const long long hw = (long long)drec.H * drec.W;
    const long long total = (long long)drec.N * hw;
    const float k[3] = {scale[0], scale[1], scale[2]};
    for (long long i = gtid(); i < total; i += gsize()) {
        const int b = (int)(i / hw);
        const int y = (int)((i % hw) / drec.W), x = (int)(i % drec.W);
        float acc[3] = {0.0f, 0.0f, 0.0f};
        if (b < p.n_images) {
            for (int t = p.img_cell0[b]; t < p.img_cell0[b + 1]; ++t) {
                const MasObjCell c = p.cells[t];
                const int cy = y - c.top, cx = x - c.left;
                if (cy < 0 || cy >= c.h || cx < 0 || cx >= c.w) continue;
                const int py = c.oy + cy, px = c.ox + cx;
                if (c.n < 0 || c.n >= p.n_canvas || py >= p.H || px >= p.W) continue;       // a malformed table reads nothing
                const TD* g = dcan + (((long long)c.n * p.H + py) * p.W + px) * CP;
#pragma unroll
                for (int ch = 0; ch < 3; ++ch) acc[ch] += (float)g[ch] / k[ch];
            }
        }
        TR* o = reinterpret_cast<TR*>(drec.data);
        const long long base = (long long)b * drec.sn + (long long)y * drec.sh + (long long)x * drec.sw;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) o[base + ch * drec.sc] = (TR)acc[ch];
    }
}

// 8 channels per thread
template <typename T, typename Tab>
__global__ __launch_bounds__(NT) void relu_fwd_kernel(T* __restrict__ y, Tab tab, int l, int N, int C) {
    if (!tab.ok()) return;
    const MasObjPlan& p = tab.p;
    const int hl = p.H >> l, wl = p.W >> l, c8 = C / 8;
    const long long total = (long long)N * hl * wl * c8;
    for (long long i = gtid(); i < total; i += gsize()) {
        const long long pix = i / c8;
        const int n = (int)(pix / ((long long)hl * wl));
        const int yy = (int)((pix / wl) % hl), xx = (int)(pix % wl);
        const bool in = cell_at(p, n % p.n_canvas, yy, xx, l) >= 0;
        V8<T> v = ld8(y + i * 8);
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float f = (float)v[k];
            v[k] = (T)(in && f > 0.0f ? f : 0.0f);
        }
        st8(y + i * 8, v);
    }
}

template <typename T>
__global__ __launch_bounds__(NT) void relu_bwd_kernel(const T* da, const T* __restrict__ a, T* dy, long long n8) {
    for (long long i = gtid(); i < n8; i += gsize()) {
        const V8<T> av = ld8(a + i * 8);
        V8<T> g = ld8(da + i * 8);
#pragma unroll
        for (int k = 0; k < 8; ++k) g[k] = (float)av[k] > 0.0f ? g[k] : (T)0.0f;
        st8(dy + i * 8, g);
    }
}

// x at level l -> y at level l + 1; 8 channels of one output pixel per thread
template <typename T, typename Tab>
__global__ __launch_bounds__(NT) void pool_fwd_kernel(const T* __restrict__ x, T* __restrict__ y, Tab tab, int l, int N, int C) {
    if (!tab.ok()) return;
    const MasObjPlan& p = tab.p;
    const int hi = p.H >> l, wi = p.W >> l, ho = hi >> 1, wo = wi >> 1, c8 = C / 8;
    const long long total = (long long)N * ho * wo * c8;
    for (long long i = gtid(); i < total; i += gsize()) {
        const int cv = (int)(i % c8);
        const long long pix = i / c8;
        const int n = (int)(pix / ((long long)ho * wo));
        const int oy = (int)((pix / wo) % ho), ox = (int)(pix % wo);
        V8<T> v = zero8<T>();
        if (cell_at(p, n % p.n_canvas, oy, ox, l + 1) >= 0) {
            const T* src = x + (((long long)n * hi + 2 * oy) * wi + 2 * ox) * C + cv * 8;
            const V8<T> a = ld8(src), b = ld8(src + C), c = ld8(src + (long long)wi * C), d = ld8(src + (long long)wi * C + C);
#pragma unroll
            for (int k = 0; k < 8; ++k) v[k] = (T)fmaxf(fmaxf((float)a[k], (float)b[k]), fmaxf((float)c[k], (float)d[k]));
        }
        st8(y + i * 8, v);
    }
}

// dy at level l (8 channels of one pixel per thread): a > 0 ? seed + routed dz : 0
template <typename T, typename Tab>
__global__ __launch_bounds__(NT) void pool_bwd_kernel(const T* __restrict__ a, const T* __restrict__ seed, const T* __restrict__ dz,
                                                      T* __restrict__ dy, Tab tab, int l, int N, int C) {
    if (!tab.ok()) return;
    const MasObjPlan& p = tab.p;
    const int hi = p.H >> l, wi = p.W >> l, ho = hi >> 1, wo = wi >> 1, c8 = C / 8;
    const long long total = (long long)N * hi * wi * c8;
    for (long long i = gtid(); i < total; i += gsize()) {
        const int cv = (int)(i % c8);
        const long long pix = i / c8;
        const int n = (int)(pix / ((long long)hi * wi));
        const int yy = (int)((pix / wi) % hi), xx = (int)(pix % wi);
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
        if (dz && py < ho && px < wo && cell_at(p, n % p.n_canvas, py, px, l + 1) >= 0) {
            const int me = (yy & 1) * 2 + (xx & 1);
            const T* w0 = a + (((long long)n * hi + 2 * py) * wi + 2 * px) * C + cv * 8;
            const V8<T> q0 = ld8(w0), q1 = ld8(w0 + C), q2 = ld8(w0 + (long long)wi * C), q3 = ld8(w0 + (long long)wi * C + C);
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

// per pixel of one cell: the LPIPS head's value; G = C / 8 lanes per pixel, 8 channels each
template <typename T, typename Tab>
__global__ __launch_bounds__(NT) void head_fwd_kernel(const T* __restrict__ feat, const float* __restrict__ w, Tab tab, int l, int C,
                                                      float* __restrict__ partial) {
    __shared__ float red[NT];
    if (!tab.ok()) return;
    const MasObjPlan& p = tab.p;
    const int G = C / 8, NG = NT / G, ppb = HEAD_PASSES * NG;
    const int nc = tab.n_cells();
    const int* blk = p.blk0 + l * tab.blk_stride();
    const int bid = blockIdx.x;
    if (Tab::FIXED_GRID && bid >= blk[nc]) return;  // a block of the fixed grid beyond the table's last one (every one when nc == 0)
    int lo = 0, hi = nc - 1;                        // the cell k with blk[k] <= bid < blk[k + 1]
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (blk[mid] <= bid) lo = mid; else hi = mid - 1;
    }
    const MasObjCell c = p.cells[lo];
    const int hl = p.H >> l, wl = p.W >> l;
    const int ch = c.h >> l, cw = c.w >> l, P = ch * cw;
    const int gi = threadIdx.x / G, li = threadIdx.x % G;
    const long long side = (long long)p.n_canvas * hl * wl * C;
    float wv[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) wv[k] = w[li * 8 + k];
    float acc = 0.0f;
    for (int pass = 0; pass < HEAD_PASSES; ++pass) {
        const int q = (bid - blk[lo]) * ppb + pass * NG + gi;
        if (q >= P) break;                          // uniform per group
        const int yy = (c.oy >> l) + q / cw, xx = (c.ox >> l) + q % cw;
        if (yy >= hl || xx >= wl || c.n < 0 || c.n >= p.n_canvas) break;
        const long long off = (((long long)c.n * hl + yy) * wl + xx) * C + li * 8;
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
    head_block_sum(acc, red, G, partial + bid);
}

template <typename Tab>
__global__ __launch_bounds__(NT) void finalize_kernel(const float* __restrict__ partial, Tab tab, float* __restrict__ out) {
    __shared__ int off[LEVELS];
    if (!tab.ok()) return;
    const MasObjPlan& p = tab.p;
    const int nc = tab.n_cells(), stride = tab.blk_stride();
    if (threadIdx.x == 0) {
        int o = 0;
        for (int l = 0; l < LEVELS; ++l) { off[l] = Tab::FIXED_GRID ? tab.part_off(l) : o; o += p.blk0[l * stride + nc]; }
    }
    __syncthreads();
    for (int k = nc + threadIdx.x; k < tab.out_cells(); k += NT) out[1 + k] = 0.0f;      // (fixed capacity: the unused slots)
    for (int k = threadIdx.x; k < nc; k += NT) {
        const MasObjCell c = p.cells[k];
        float v = 0.0f;
        for (int l = 0; l < LEVELS; ++l) {
            const int* blk = p.blk0 + l * stride;
            float s = 0.0f;
            for (int j = blk[k]; j < blk[k + 1]; ++j) s += partial[off[l] + j];
            v += s / (float)((c.h >> l) * (c.w >> l));
        }
        out[1 + k] = v;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float loss = 0.0f;
        for (int b = 0; b < p.n_images; ++b) {
            float s = 0.0f;
            const int k0 = p.img_cell0[b], k1 = p.img_cell0[b + 1];
            for (int k = k0; k < k1; ++k) s += out[1 + k];
            loss += s / (float)(k1 - k0 + 1);
        }
        out[0] = loss;
    }
}

// seed = d out / d (rec feature) at level l, every rec-side pixel of the level (0 outside the cells); G lanes per pixel
template <typename T, typename Tab>
__global__ __launch_bounds__(NT) void head_bwd_kernel(const T* __restrict__ feat, const float* __restrict__ w, Tab tab, int l, int C,
                                                      const float* __restrict__ dout, T* __restrict__ seed) {
    if (!tab.ok()) return;
    const MasObjPlan& p = tab.p;
    const int G = C / 8, NG = NT / G;
    const int hl = p.H >> l, wl = p.W >> l;
    const long long npix = (long long)p.n_canvas * hl * wl;
    const long long side = npix * C;
    const int gi = threadIdx.x / G, li = threadIdx.x % G;
    float wv[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) wv[k] = w[li * 8 + k];
    const float d0 = dout[0];
    for (long long pix = (long long)blockIdx.x * NG + gi; pix < npix; pix += (long long)gridDim.x * NG) {
        const int n = (int)(pix / ((long long)hl * wl));
        const int yy = (int)((pix / wl) % hl), xx = (int)(pix % wl);
        const long long off = pix * C + li * 8;
        const int t = cell_at(p, n, yy, xx, l);
        V8<T> o = zero8<T>();
        if (t >= 0) {
            const MasObjCell c = p.cells[t];
            const int nb = p.img_cell0[c.b + 1] - p.img_cell0[c.b];
            const float coef = (d0 / (float)(nb + 1) + dout[1 + t]) / (float)((c.h >> l) * (c.w >> l));
            const V8<T> fr = ld8(feat + off), ff = ld8(feat + side + off);
            float sr = 0.0f, sf = 0.0f;
#pragma unroll
            for (int k = 0; k < 8; ++k) { sr += (float)fr[k] * (float)fr[k]; sf += (float)ff[k] * (float)ff[k]; }
            const float s = sqrtf(group_sum(sf, G));
            const float nr = sqrtf(group_sum(sr, G)) + 1e-10f, nf = s + 1e-10f;
            float g[8], gf = 0.0f;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                g[k] = -2.0f * coef * wv[k] * ((float)fr[k] / nr - (float)ff[k] / nf);         // d / d (g_c / (|g| + eps))
                gf += g[k] * (float)ff[k];
            }
            gf = group_sum(gf, G);
            const float rad = s > 0.0f ? gf / (nf * nf * s) : 0.0f;
#pragma unroll
            for (int k = 0; k < 8; ++k) o[k] = (T)(g[k] / nf - (float)ff[k] * rad);
        }
        st8(seed + off, o);
    }
}

int check_plan(const MasObjPlan* p, const char* what) {
    if (!p || !p->cells || !p->img_cell0 || !p->tiles || !p->blk0) MAS_FAIL(MAS_EINVAL, "%s: null plan table", what);
    if (p->n_cells <= 0 || p->n_images <= 0 || p->n_canvas <= 0 || p->H <= 0 || p->W <= 0 || p->H % MAS_OBJ_ALIGN || p->W % MAS_OBJ_ALIGN)
        MAS_FAIL(MAS_EINVAL, "%s: bad plan (%d cells, %d images, %d canvases of %d x %d)", what, p->n_cells, p->n_images, p->n_canvas, p->H, p->W);
    return MAS_OK;
}

int check_level(int level, int N, int C, int dtype, int max_level, const char* what) {
    if (level < 0 || level > max_level || N <= 0 || C <= 0 || C % 8 || !dt_ok(dtype))
        MAS_FAIL(MAS_EINVAL, "%s: level %d, N %d, C %d, dtype %d", what, level, N, C, dtype);
    return MAS_OK;
}

int check_map(const MasObjPlan* p, int level, int N, int C, int dtype, int max_level, const char* what) {
    if (int rc = check_plan(p, what)) return rc;
    return check_level(level, N, C, dtype, max_level, what);
}

// ---- the fixed-capacity table (mas_obj_*_dev): its geometry comes by value, everything about the boxes is in the table --------------------
constexpr int HEAD_C[LEVELS] = {64, 128, 256, 512, 512};       // VGG16's channels at the five LPIPS levels
constexpr int MAX_ATLAS_CELLS = 4096;

struct Atlas { const int32_t* table; int max_cells, n_images, n_canvas, H, W; };

bool atlas_geometry_ok(const Atlas& a) {
    return a.max_cells >= 1 && a.max_cells <= MAX_ATLAS_CELLS && a.n_images >= 1 && a.n_canvas >= 1 && a.H >= MAS_OBJ_ALIGN && a.W >= MAS_OBJ_ALIGN &&
           a.H % MAS_OBJ_ALIGN == 0 && a.W % MAS_OBJ_ALIGN == 0 && (long long)a.n_canvas * a.H * a.W <= (1LL << 28) && a.n_images <= (1 << 20);
}

int check_atlas(const Atlas& a, const char* what) {
    if (!a.table) MAS_FAIL(MAS_EINVAL, "%s: null atlas table", what);
    if (!atlas_geometry_ok(a))
        MAS_FAIL(MAS_EINVAL, "%s: bad atlas (%d cells at most, %d images, %d canvases of %d x %d)", what, a.max_cells, a.n_images, a.n_canvas, a.H, a.W);
    return MAS_OK;
}

// the head's grid at level l, whatever the table holds: the cells' level-l rectangles are disjoint and inside the canvases, and every cell
// rounds its pixels up to whole blocks once
int head_grid(const Atlas& a, int l) {
    const long long pix = (long long)a.n_canvas * (a.H >> l) * (a.W >> l);
    const int ppb = MAS_OBJ_HEAD_PIX(HEAD_C[l]);
    return (int)((pix + ppb - 1) / ppb) + a.max_cells;
}

DevTab dev_tab(const Atlas& a) {
    DevTab t;
    const int32_t* cells = a.table + MAS_OBJ_ATLAS_HEADER;
    const int32_t* img0 = cells + 8LL * a.max_cells;
    const int32_t* blk0 = img0 + a.n_images + 1;
    t.p.cells = reinterpret_cast<const MasObjCell*>(cells);
    t.p.img_cell0 = img0;
    t.p.blk0 = blk0;
    t.p.tiles = blk0 + LEVELS * (a.max_cells + 1);
    t.p.n_cells = 0; t.p.n_images = a.n_images; t.p.n_canvas = a.n_canvas; t.p.H = a.H; t.p.W = a.W; t.p.pad_ = 0;
    t.header = a.table;
    t.max_cells = a.max_cells;
    int o = 0;
    for (int l = 0; l < LEVELS; ++l) { t.off[l] = o; o += head_grid(a, l); }
    return t;
}

// ---- the launches, once for both kinds of table ---------------------------------------------------------------------------------------
template <typename Tab>
void launch_canvas_fwd(const Tab& t, const MasFaceImage* img, const MasFaceImage* rec, const float* shift, const float* scale, void* canvas, int dtype,
                       hipStream_t s) {
    const dim3 grid(grid_for(2LL * t.p.n_canvas * t.p.H * t.p.W));
    if (dtype == MAS_F32) hipLaunchKernelGGL((canvas_fwd_kernel<float, Tab>), grid, dim3(NT), 0, s, *img, *rec, t, shift, scale, (float*)canvas);
    else hipLaunchKernelGGL((canvas_fwd_kernel<bf16_t, Tab>), grid, dim3(NT), 0, s, *img, *rec, t, shift, scale, (bf16_t*)canvas);
}

template <typename Tab>
void launch_canvas_bwd(const Tab& t, const void* dcanvas, int dtype, const float* scale, const MasFaceImage* drec, hipStream_t s) {
    const dim3 grid(grid_for((long long)drec->N * drec->H * drec->W));
    if (dtype == MAS_F32) {
        if (drec->dtype == MAS_F32) hipLaunchKernelGGL((canvas_bwd_kernel<float, float, Tab>), grid, dim3(NT), 0, s, (const float*)dcanvas, t, scale, *drec);
        else hipLaunchKernelGGL((canvas_bwd_kernel<float, bf16_t, Tab>), grid, dim3(NT), 0, s, (const float*)dcanvas, t, scale, *drec);
    } else {
        if (drec->dtype == MAS_F32) hipLaunchKernelGGL((canvas_bwd_kernel<bf16_t, float, Tab>), grid, dim3(NT), 0, s, (const bf16_t*)dcanvas, t, scale, *drec);
        else hipLaunchKernelGGL((canvas_bwd_kernel<bf16_t, bf16_t, Tab>), grid, dim3(NT), 0, s, (const bf16_t*)dcanvas, t, scale, *drec);
    }
}

template <typename Tab>
void launch_relu_fwd(const Tab& t, void* y, int level, int N, int C, int dtype, hipStream_t s) {
    const dim3 grid(grid_for((long long)N * (t.p.H >> level) * (t.p.W >> level) * (C / 8)));
    if (dtype == MAS_F32) hipLaunchKernelGGL((relu_fwd_kernel<float, Tab>), grid, dim3(NT), 0, s, (float*)y, t, level, N, C);
    else hipLaunchKernelGGL((relu_fwd_kernel<bf16_t, Tab>), grid, dim3(NT), 0, s, (bf16_t*)y, t, level, N, C);
}

template <typename Tab>
void launch_pool_fwd(const Tab& t, const void* x, void* y, int level, int N, int C, int dtype, hipStream_t s) {
    const dim3 grid(grid_for((long long)N * (t.p.H >> (level + 1)) * (t.p.W >> (level + 1)) * (C / 8)));
    if (dtype == MAS_F32) hipLaunchKernelGGL((pool_fwd_kernel<float, Tab>), grid, dim3(NT), 0, s, (const float*)x, (float*)y, t, level, N, C);
    else hipLaunchKernelGGL((pool_fwd_kernel<bf16_t, Tab>), grid, dim3(NT), 0, s, (const bf16_t*)x, (bf16_t*)y, t, level, N, C);
}

template <typename Tab>
void launch_pool_bwd(const Tab& t, const void* a, const void* seed, const void* dz, void* dy, int level, int N, int C, int dtype, hipStream_t s) {
    const dim3 grid(grid_for((long long)N * (t.p.H >> level) * (t.p.W >> level) * (C / 8)));
    if (dtype == MAS_F32)
        hipLaunchKernelGGL((pool_bwd_kernel<float, Tab>), grid, dim3(NT), 0, s, (const float*)a, (const float*)seed, (const float*)dz, (float*)dy, t, level, N, C);
    else
        hipLaunchKernelGGL((pool_bwd_kernel<bf16_t, Tab>), grid, dim3(NT), 0, s, (const bf16_t*)a, (const bf16_t*)seed, (const bf16_t*)dz, (bf16_t*)dy, t,
                           level, N, C);
}

template <typename Tab>
void launch_head_fwd(const Tab& t, const void* feat, const float* w, int level, int C, int dtype, int n_blocks, float* partial, hipStream_t s) {
    if (dtype == MAS_F32) hipLaunchKernelGGL((head_fwd_kernel<float, Tab>), dim3(n_blocks), dim3(NT), 0, s, (const float*)feat, w, t, level, C, partial);
    else hipLaunchKernelGGL((head_fwd_kernel<bf16_t, Tab>), dim3(n_blocks), dim3(NT), 0, s, (const bf16_t*)feat, w, t, level, C, partial);
}

template <typename Tab>
void launch_head_bwd(const Tab& t, const void* feat, const float* w, int level, int C, int dtype, const float* dout, void* seed, hipStream_t s) {
    const long long npix = (long long)t.p.n_canvas * (t.p.H >> level) * (t.p.W >> level);
    const dim3 grid(grid_for(npix * (C / 8)));
    if (dtype == MAS_F32) hipLaunchKernelGGL((head_bwd_kernel<float, Tab>), grid, dim3(NT), 0, s, (const float*)feat, w, t, level, C, dout, (float*)seed);
    else hipLaunchKernelGGL((head_bwd_kernel<bf16_t, Tab>), grid, dim3(NT), 0, s, (const bf16_t*)feat, w, t, level, C, dout, (bf16_t*)seed);
}

bool head_c_ok(int C) { return C >= 64 && C <= 512 && !(C & (C - 1)); }

}  // namespace

extern "C" int mas_obj_canvas_fwd(const MasFaceImage* img, const MasFaceImage* rec, const MasObjPlan* p, const float* shift, const float* scale,
                                  void* canvas, int dtype, void* stream) {
    MAS_ENTER();
    if (int rc = check_img(img, "obj_canvas_fwd")) return rc;
    if (int rc = check_img(rec, "obj_canvas_fwd")) return rc;
    if (int rc = check_plan(p, "obj_canvas_fwd")) return rc;
    if (!shift || !scale || !canvas || !dt_ok(dtype)) MAS_FAIL(MAS_EINVAL, "obj_canvas_fwd: null argument or dtype %d", dtype);
    launch_canvas_fwd(ListTab{*p}, img, rec, shift, scale, canvas, dtype, reinterpret_cast<hipStream_t>(stream));
    MAS_CHECK_LAUNCH("obj_canvas_fwd");
    return MAS_OK;
}

extern "C" int mas_obj_canvas_bwd(const void* dcanvas, int dtype, const MasObjPlan* p, const float* scale, const MasFaceImage* drec, void* stream) {
    MAS_ENTER();
    if (int rc = check_img(drec, "obj_canvas_bwd")) return rc;
    if (int rc = check_plan(p, "obj_canvas_bwd")) return rc;
    if (!dcanvas || !scale || !dt_ok(dtype)) MAS_FAIL(MAS_EINVAL, "obj_canvas_bwd: null argument or dtype %d", dtype);
    launch_canvas_bwd(ListTab{*p}, dcanvas, dtype, scale, drec, reinterpret_cast<hipStream_t>(stream));
    MAS_CHECK_LAUNCH("obj_canvas_bwd");
    return MAS_OK;
}

extern "C" int mas_obj_relu_fwd(void* y, const MasObjPlan* p, int level, int N, int C, int dtype, void* stream) {
    MAS_ENTER();
    if (int rc = check_map(p, level, N, C, dtype, LEVELS - 1, "obj_relu_fwd")) return rc;
    if (!y) MAS_FAIL(MAS_EINVAL, "obj_relu_fwd: null tensor");
    launch_relu_fwd(ListTab{*p}, y, level, N, C, dtype, reinterpret_cast<hipStream_t>(stream));
    MAS_CHECK_LAUNCH("obj_relu_fwd");
    return MAS_OK;
}

extern "C" int mas_obj_relu_bwd(const void* da, const void* a, void* dy, long long n, int dtype, void* stream) {
    MAS_ENTER();
    if (!da || !a || !dy || n <= 0 || n % 8 || !dt_ok(dtype)) MAS_FAIL(MAS_EINVAL, "obj_relu_bwd: bad argument (n %lld, dtype %d)", n, dtype);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(grid_for(n / 8));
    if (dtype == MAS_F32) hipLaunchKernelGGL(relu_bwd_kernel<float>, grid, dim3(NT), 0, s, (const float*)da, (const float*)a, (float*)dy, n / 8);
    else hipLaunchKernelGGL(relu_bwd_kernel<bf16_t>, grid, dim3(NT), 0, s, (const bf16_t*)da, (const bf16_t*)a, (bf16_t*)dy, n / 8);
    MAS_CHECK_LAUNCH("obj_relu_bwd");
    return MAS_OK;
}

extern "C" int mas_obj_pool_fwd(const void* x, void* y, const MasObjPlan* p, int level, int N, int C, int dtype, void* stream) {
    MAS_ENTER();
    if (int rc = check_map(p, level, N, C, dtype, LEVELS - 2, "obj_pool_fwd")) return rc;
    if (!x || !y) MAS_FAIL(MAS_EINVAL, "obj_pool_fwd: null tensor");
    launch_pool_fwd(ListTab{*p}, x, y, level, N, C, dtype, reinterpret_cast<hipStream_t>(stream));
    MAS_CHECK_LAUNCH("obj_pool_fwd");
    return MAS_OK;
}

extern "C" int mas_obj_pool_bwd(const void* a, const void* seed, const void* dz, void* dy, const MasObjPlan* p, int level, int N, int C, int dtype,
                                void* stream) {
    MAS_ENTER();
    if (int rc = check_map(p, level, N, C, dtype, LEVELS - 1, "obj_pool_bwd")) return rc;
    if (!a || !dy || (dz && level == LEVELS - 1)) MAS_FAIL(MAS_EINVAL, "obj_pool_bwd: null tensor, or a pooled gradient at the top level");
    launch_pool_bwd(ListTab{*p}, a, seed, dz, dy, level, N, C, dtype, reinterpret_cast<hipStream_t>(stream));
    MAS_CHECK_LAUNCH("obj_pool_bwd");
    return MAS_OK;
}

extern "C" int mas_obj_head_fwd(const void* feat, const float* w, const MasObjPlan* p, int level, int C, int dtype, int n_blocks, float* partial,
                                void* stream) {
    MAS_ENTER();
    if (int rc = check_map(p, level, 1, C, dtype, LEVELS - 1, "obj_head_fwd")) return rc;
    if (!feat || !w || !partial || !head_c_ok(C) || n_blocks < p->n_cells)
        MAS_FAIL(MAS_EINVAL, "obj_head_fwd: null argument, C %d or %d blocks for %d cells", C, n_blocks, p->n_cells);
    launch_head_fwd(ListTab{*p}, feat, w, level, C, dtype, n_blocks, partial, reinterpret_cast<hipStream_t>(stream));
    MAS_CHECK_LAUNCH("obj_head_fwd");
    return MAS_OK;
}

extern "C" int mas_obj_finalize(const float* partial, const MasObjPlan* p, float* out, void* stream) {
    MAS_ENTER();
    if (int rc = check_plan(p, "obj_finalize")) return rc;
    if (!partial || !out) MAS_FAIL(MAS_EINVAL, "obj_finalize: null argument");
    hipLaunchKernelGGL(finalize_kernel<ListTab>, dim3(1), dim3(NT), 0, reinterpret_cast<hipStream_t>(stream), partial, ListTab{*p}, out);
    MAS_CHECK_LAUNCH("obj_finalize");
    return MAS_OK;
}

extern "C" int mas_obj_head_bwd(const void* feat, const float* w, const MasObjPlan* p, int level, int C, int dtype, const float* dout, void* seed,
                                void* stream) {
    MAS_ENTER();
    if (int rc = check_map(p, level, 1, C, dtype, LEVELS - 1, "obj_head_bwd")) return rc;
    if (!feat || !w || !dout || !seed || !head_c_ok(C)) MAS_FAIL(MAS_EINVAL, "obj_head_bwd: null argument or C %d", C);
    launch_head_bwd(ListTab{*p}, feat, w, level, C, dtype, dout, seed, reinterpret_cast<hipStream_t>(stream));
    MAS_CHECK_LAUNCH("obj_head_bwd");
    return MAS_OK;
}

// ---- the same passes on a table of fixed capacity: nothing about the boxes comes from the host ---------------------------------------
extern "C" int mas_obj_atlas_ints(int max_cells, int n_images, int n_canvas, int H, int W) {
    MAS_ENTER();
    const Atlas a{nullptr, max_cells, n_images, n_canvas, H, W};
    if (!atlas_geometry_ok(a)) MAS_FAIL(MAS_EINVAL, "obj_atlas_ints: bad atlas (%d cells at most, %d images, %d canvases of %d x %d)", max_cells, n_images, n_canvas, H, W);
    return MAS_OBJ_ATLAS_HEADER + 8 * max_cells + (n_images + 1) + LEVELS * (max_cells + 1) + n_canvas * (H / MAS_OBJ_ALIGN) * (W / MAS_OBJ_ALIGN);
}

extern "C" int mas_obj_head_grid_dev(int level, int max_cells, int n_canvas, int H, int W) {
    MAS_ENTER();
    const Atlas a{nullptr, max_cells, 1, n_canvas, H, W};
    if (!atlas_geometry_ok(a) || level < 0 || level >= LEVELS) MAS_FAIL(MAS_EINVAL, "obj_head_grid_dev: level %d or a bad atlas (%d cells at most, %d canvases of %d x %d)", level, max_cells, n_canvas, H, W);
    return head_grid(a, level);
}

extern "C" int mas_obj_canvas_fwd_dev(const MasFaceImage* img, const MasFaceImage* rec, const int32_t* table_dev, int max_cells, int n_images,
                                      int n_canvas, int H, int W, const float* shift, const float* scale, void* canvas, int dtype, void* stream) {
    MAS_ENTER();
    const Atlas a{table_dev, max_cells, n_images, n_canvas, H, W};
    if (int rc = check_img(img, "obj_canvas_fwd_dev")) return rc;
    if (int rc = check_img(rec, "obj_canvas_fwd_dev")) return rc;
    if (int rc = check_atlas(a, "obj_canvas_fwd_dev")) return rc;
    if (!shift || !scale || !canvas || !dt_ok(dtype)) MAS_FAIL(MAS_EINVAL, "obj_canvas_fwd_dev: null argument or dtype %d", dtype);
    launch_canvas_fwd(dev_tab(a), img, rec, shift, scale, canvas, dtype, reinterpret_cast<hipStream_t>(stream));
    MAS_CHECK_LAUNCH("obj_canvas_fwd_dev");
    return MAS_OK;
}

extern "C" int mas_obj_canvas_bwd_dev(const void* dcanvas, int dtype, const int32_t* table_dev, int max_cells, int n_images, int n_canvas, int H, int W,
                                      const float* scale, const MasFaceImage* drec, void* stream) {
    MAS_ENTER();
    const Atlas a{table_dev, max_cells, n_images, n_canvas, H, W};
    if (int rc = check_img(drec, "obj_canvas_bwd_dev")) return rc;
    if (int rc = check_atlas(a, "obj_canvas_bwd_dev")) return rc;
    if (!dcanvas || !scale || !dt_ok(dtype)) MAS_FAIL(MAS_EINVAL, "obj_canvas_bwd_dev: null argument or dtype %d", dtype);
    launch_canvas_bwd(dev_tab(a), dcanvas, dtype, scale, drec, reinterpret_cast<hipStream_t>(stream));
    MAS_CHECK_LAUNCH("obj_canvas_bwd_dev");
    return MAS_OK;
}

extern "C" int mas_obj_relu_fwd_dev(void* y, const int32_t* table_dev, int max_cells, int n_images, int n_canvas, int H, int W, int level, int N, int C,
                                    int dtype, void* stream) {
    MAS_ENTER();
    const Atlas a{table_dev, max_cells, n_images, n_canvas, H, W};
    if (int rc = check_atlas(a, "obj_relu_fwd_dev")) return rc;
    if (int rc = check_level(level, N, C, dtype, LEVELS - 1, "obj_relu_fwd_dev")) return rc;
    if (!y) MAS_FAIL(MAS_EINVAL, "obj_relu_fwd_dev: null tensor");
    launch_relu_fwd(dev_tab(a), y, level, N, C, dtype, reinterpret_cast<hipStream_t>(stream));
    MAS_CHECK_LAUNCH("obj_relu_fwd_dev");
    return MAS_OK;
}

extern "C" int mas_obj_pool_fwd_dev(const void* x, void* y, const int32_t* table_dev, int max_cells, int n_images, int n_canvas, int H, int W, int level,
                                    int N, int C, int dtype, void* stream) {
    MAS_ENTER();
    const Atlas a{table_dev, max_cells, n_images, n_canvas, H, W};
    if (int rc = check_atlas(a, "obj_pool_fwd_dev")) return rc;
    if (int rc = check_level(level, N, C, dtype, LEVELS - 2, "obj_pool_fwd_dev")) return rc;
    if (!x || !y) MAS_FAIL(MAS_EINVAL, "obj_pool_fwd_dev: null tensor");
    launch_pool_fwd(dev_tab(a), x, y, level, N, C, dtype, reinterpret_cast<hipStream_t>(stream));
    MAS_CHECK_LAUNCH("obj_pool_fwd_dev");
    return MAS_OK;
}

extern "C" int mas_obj_pool_bwd_dev(const void* a_, const void* seed, const void* dz, void* dy, const int32_t* table_dev, int max_cells, int n_images,
                                    int n_canvas, int H, int W, int level, int N, int C, int dtype, void* stream) {
    MAS_ENTER();
    const Atlas a{table_dev, max_cells, n_images, n_canvas, H, W};
    if (int rc = check_atlas(a, "obj_pool_bwd_dev")) return rc;
    if (int rc = check_level(level, N, C, dtype, LEVELS - 1, "obj_pool_bwd_dev")) return rc;
    if (!a_ || !dy || (dz && level == LEVELS - 1)) MAS_FAIL(MAS_EINVAL, "obj_pool_bwd_dev: null tensor, or a pooled gradient at the top level");
    launch_pool_bwd(dev_tab(a), a_, seed, dz, dy, level, N, C, dtype, reinterpret_cast<hipStream_t>(stream));
    MAS_CHECK_LAUNCH("obj_pool_bwd_dev");
    return MAS_OK;
}

extern "C" int mas_obj_head_fwd_dev(const void* feat, const float* w, const int32_t* table_dev, int max_cells, int n_images, int n_canvas, int H, int W,
                                    int level, int dtype, float* partial, void* stream) {
    MAS_ENTER();
    const Atlas a{table_dev, max_cells, n_images, n_canvas, H, W};
    if (int rc = check_atlas(a, "obj_head_fwd_dev")) return rc;
    if (int rc = check_level(level, 1, 8, dtype, LEVELS - 1, "obj_head_fwd_dev")) return rc;
    if (!feat || !w || !partial) MAS_FAIL(MAS_EINVAL, "obj_head_fwd_dev: null argument");
    const DevTab t = dev_tab(a);
    launch_head_fwd(t, feat, w, level, HEAD_C[level], dtype, head_grid(a, level), partial + t.off[level], reinterpret_cast<hipStream_t>(stream));
    MAS_CHECK_LAUNCH("obj_head_fwd_dev");
    return MAS_OK;
}

extern "C" int mas_obj_finalize_dev(const float* partial, const int32_t* table_dev, int max_cells, int n_images, int n_canvas, int H, int W, float* out,
                                    void* stream) {
    MAS_ENTER();
    const Atlas a{table_dev, max_cells, n_images, n_canvas, H, W};
    if (int rc = check_atlas(a, "obj_finalize_dev")) return rc;
    if (!partial || !out) MAS_FAIL(MAS_EINVAL, "obj_finalize_dev: null argument");
    hipLaunchKernelGGL(finalize_kernel<DevTab>, dim3(1), dim3(NT), 0, reinterpret_cast<hipStream_t>(stream), partial, dev_tab(a), out);
    MAS_CHECK_LAUNCH("obj_finalize_dev");
    return MAS_OK;
}

extern "C" int mas_obj_head_bwd_dev(const void* feat, const float* w, const int32_t* table_dev, int max_cells, int n_images, int n_canvas, int H, int W,
                                    int level, int dtype, const float* dout, void* seed, void* stream) {
    MAS_ENTER();
    const Atlas a{table_dev, max_cells, n_images, n_canvas, H, W};
    if (int rc = check_atlas(a, "obj_head_bwd_dev")) return rc;
    if (int rc = check_level(level, 1, 8, dtype, LEVELS - 1, "obj_head_bwd_dev")) return rc;
    if (!feat || !w || !dout || !seed) MAS_FAIL(MAS_EINVAL, "obj_head_bwd_dev: null argument");
    launch_head_bwd(dev_tab(a), feat, w, level, HEAD_C[level], dtype, dout, seed, reinterpret_cast<hipStream_t>(stream));
    MAS_CHECK_LAUNCH("obj_head_bwd_dev");
    return MAS_OK;
}
