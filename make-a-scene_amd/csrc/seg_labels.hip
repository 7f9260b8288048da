// The VQ-SEG map as label planes (reference Data/dataset_preprocessor.py:62-86 builds it as a [H, W, 159] one-hot tensor: 636 bytes per
// pixel for 4 bytes of information).  planes [N, P, H, W] uint8: a class-label plane per group (0 = none, v sets channel base + v - 1), then
// planes that hold a channel's value (the edge channel: 0, 1 or 2).  Two things are made from them, and neither ever holds a dense target:
//   * seg_expand            : the dense map the encoder's first convolution reads, written ONCE in that convolution's layout (NHWC, channel
//                             axis zero-padded to a 16-byte multiple) or as NCHW: a write-bound stream
//   * seg_loss_labels_fwd/bwd: the objective of seg_loss.hip (the per-element code is seg_elem.h, shared) with t derived in registers
// A work-group takes tiles of TP = 256 pixels of one image x all channels.  Per tile, lane i reads the P label bytes of pixel i -- the only
// read of them -- and leaves the pixel's ENTRIES in LDS: PS (4 or 8) dwords {channel | value << 16}, 0xffff = none.  After that a channel
// c of that pixel has the value of the entry whose channel equals c, or 0: PS compares, and no address ever depends on a label.
//   NHWC output / prediction: the tile is one contiguous block of pw C elements, walked in 16-byte units; a lane reads the entries of its
//        unit's pixel from LDS (one or two ds_read_b128) and moves on to the next pixel's where the unit crosses into it.  The loss walks
//        the block from its first 16-byte boundary in memory, head and tail elements one by one (the flat kernel of seg_loss.hip).
//   NCHW output / prediction: C rows of pw consecutive pixels.  A lane keeps V pixels (one 16-byte unit where the rows are 16-byte aligned,
//        one pixel otherwise) for the whole tile, their entries in registers, and walks the channels: a wave reads 1 KB of one row at a time.
// Forward sums: a lane adds in fp32 over at most 4 units, then in fp64; work-group tree and reduce kernel are seg_loss.hip's.
// The grid depends on the shape and the CU count only; no atomics; 64-bit offsets.
#include "mas_common.h"
#include "seg_elem.h"

namespace {

constexpr int NT = SEG_NT;
constexpr int TP = MAS_SEG_LABELS_TILE;
static_assert(TP == NT, "one lane stages one pixel of a tile");
constexpr unsigned NONE = 0xffffu;
typedef unsigned char u8_t;

struct Layout {
    int P;
    unsigned C;
    unsigned base[MAS_SEG_MAX_PLANES], size[MAS_SEG_MAX_PLANES];      // size 0: a value plane, its byte is the value of channel `base`
};

struct Args {
    Layout L;
    const u8_t* planes;
    const void* x; void* out;            // expand: out = the map; loss: x = prediction, out = dx
    const float* w;
    long long tiles;
    unsigned HW, tiles_per_img, Cout;    // Cout: channels of the output (C_pad) or of the prediction (C)
    float invC;                          // 1 / Cout (NHWC loss), 1 / units per pixel (NHWC expand)
    int mse_on;
    const float* g; double inv_n;
    double* partials;
};

// the tile's labels -> entries in LDS [TP + 1][PS]; slot TP is `none`: a unit that ends on the tile's last element looks one pixel ahead
template <int PS>
__device__ __forceinline__ void stage(const Layout& L, const u8_t* __restrict__ pl, unsigned HW, unsigned pw, unsigned* s_e) {
    const unsigned tid = threadIdx.x;
    unsigned e[PS];
#pragma unroll
    for (int k = 0; k < PS; ++k) {
        e[k] = NONE;
        if (k < L.P && tid < pw) {
            const unsigned v = pl[(long long)k * HW + tid];
            const unsigned size = L.size[k], base = L.base[k];
            if (size == 0) e[k] = base | (v << 16);
            else if (v >= 1 && v <= size) e[k] = (base + v - 1) | (1u << 16);
        }
    }
#pragma unroll
    for (int k = 0; k < PS; k += 4) *reinterpret_cast<u32x4*>(s_e + tid * PS + k) = u32x4{e[k], e[k + 1], e[k + 2], e[k + 3]};
    if (tid < PS) s_e[TP * PS + tid] = NONE;
}
template <int PS>
__device__ __forceinline__ void entries(const unsigned* s_e, unsigned p, unsigned (&e)[PS]) {
#pragma unroll
    for (int k = 0; k < PS; k += 4) {
        const u32x4 q = *reinterpret_cast<const u32x4*>(s_e + p * PS + k);
        e[k] = q[0]; e[k + 1] = q[1]; e[k + 2] = q[2]; e[k + 3] = q[3];
    }
}
template <int PS>
__device__ __forceinline__ float value_of(const unsigned (&e)[PS], unsigned c) {
    float t = 0.0f;
#pragma unroll
    for (int k = 0; k < PS; ++k) t = (e[k] & 0xffffu) == c ? (float)(e[k] >> 16) : t;
    return t;
}

struct Tile { long long img; unsigned p0, pw; };
__device__ __forceinline__ Tile tile_of(long long tile, unsigned tiles_per_img, unsigned HW) {
    Tile t;
    t.img = tile / tiles_per_img;
    t.p0 = (unsigned)(tile - t.img * tiles_per_img) * TP;
    t.pw = HW - t.p0 < (unsigned)TP ? HW - t.p0 : (unsigned)TP;
    return t;
}

// ---- expand -----------------------------------------------------------------------------------------------------------------------
// U = elements per store: one 16-byte unit (Cout % U == 0 and out 16-byte aligned, so every pixel is) or 1
template <typename OT, int PS, int U>
__global__ __launch_bounds__(NT) void seg_expand_nhwc_kernel(const Args A) {
    __shared__ __attribute__((aligned(16))) unsigned s_e[(TP + 1) * PS];
    const unsigned upp = A.Cout / U;                             // units per pixel
    for (long long tile = blockIdx.x; tile < A.tiles; tile += gridDim.x) {
        const Tile T = tile_of(tile, A.tiles_per_img, A.HW);
        __syncthreads();
        stage<PS>(A.L, A.planes + (T.img * A.L.P) * (long long)A.HW + T.p0, A.HW, T.pw, s_e);
        __syncthreads();
        OT* ob = (OT*)A.out + (T.img * A.HW + T.p0) * (long long)A.Cout;
        const unsigned nunits = T.pw * upp;
#pragma unroll 2
        for (unsigned q = threadIdx.x; q < nunits; q += NT) {
            unsigned p, u;
            divmod(q, upp, A.invC, p, u);
            unsigned e[PS];
            entries<PS>(s_e, p, e);
            float v[U];
#pragma unroll
            for (int i = 0; i < U; ++i) v[i] = value_of<PS>(e, u * U + i);       // channels C .. Cout - 1 match no entry: exact zeros
            st_n<OT, U>(ob + (size_t)q * U, true, v);
        }
    }
}

// V = pixels per store: one 16-byte unit (HW % V == 0 and out 16-byte aligned, so every row of every tile is) or 1
template <typename OT, int PS, int V>
__global__ __launch_bounds__(NT) void seg_expand_nchw_kernel(const Args A) {
    __shared__ __attribute__((aligned(16))) unsigned s_e[(TP + 1) * PS];
    constexpr int UPR = TP / V, ROWS = NT / UPR;
    const unsigned lu = threadIdx.x % UPR, lrow = threadIdx.x / UPR;
    for (long long tile = blockIdx.x; tile < A.tiles; tile += gridDim.x) {
        const Tile T = tile_of(tile, A.tiles_per_img, A.HW);
        __syncthreads();
        stage<PS>(A.L, A.planes + (T.img * A.L.P) * (long long)A.HW + T.p0, A.HW, T.pw, s_e);
        __syncthreads();
        if (lu * V < T.pw) {
            unsigned e[V][PS];
#pragma unroll
            for (int i = 0; i < V; ++i) entries<PS>(s_e, lu * V + i, e[i]);
            OT* ob = (OT*)A.out + (T.img * A.Cout) * (long long)A.HW + T.p0 + lu * V;
#pragma unroll 4
            for (unsigned c = lrow; c < A.Cout; c += ROWS) {
                float v[V];
#pragma unroll
                for (int i = 0; i < V; ++i) v[i] = value_of<PS>(e[i], c);
                st_n<OT, V>(ob + (long long)c * A.HW, true, v);
            }
        }
    }
}

// ---- loss -------------------------------------------------------------------------------------------------------------------------
template <typename PT, int PS, bool BWD>
struct Block {                            // one tile of an NHWC prediction: pw C contiguous elements
    static constexpr int U = 16 / (int)sizeof(PT);
    const PT* x; PT* dx; const unsigned* s_e; const float* s_w;
    unsigned C; float invC, scale; bool mse_on;
    double bce, sq;

    template <int N>
    __device__ __forceinline__ void proc(int j, bool dvec) {
        float xv[N], out[N];
        ld_n<PT, N>(x + j, true, xv);
        unsigned p, c;
        divmod((unsigned)j, C, invC, p, c);
        unsigned e[PS];
        entries<PS>(s_e, p, e);
        float fb = 0.0f, fs = 0.0f;
#pragma unroll
        for (int i = 0; i < N; ++i) {
            const float t = value_of<PS>(e, c), wm1 = s_w[c];
            if constexpr (BWD) out[i] = elem_bwd(xv[i], t, wm1, mse_on, scale);
            else elem_fwd(xv[i], t, wm1, mse_on, fb, fs);
            if (N > 1 && ++c == C) { c = 0; ++p; entries<PS>(s_e, p, e); }       // (p <= pw <= TP: slot TP exists)
        }
        if constexpr (BWD) st_n<PT, N>(dx + j, dvec, out);
        else { bce += (double)fb; sq += (double)fs; }
    }

    __device__ __forceinline__ void run(int len) {
        const int tid = threadIdx.x;
        int head = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(x) & 15)) & 15) / sizeof(PT));   // elements ahead of the first 16-byte unit
        if (head > len) head = len;
        const int nunits = (len - head) / U, tail0 = head + nunits * U;
        const bool dvec = BWD ? aligned_to(dx + head, 16) : false;
        if (tid < head) proc<1>(tid, false);
        if (tid >= 64 && tid - 64 < len - tail0) proc<1>(tail0 + tid - 64, false);                      // (head, tail < U <= 8)
#pragma unroll 2
        for (int u = tid; u < nunits; u += NT) proc<U>(head + u * U, dvec);
    }
};

template <typename PT, int PS, bool BWD>
__global__ __launch_bounds__(NT) void seg_labels_nhwc_kernel(const Args A) {
    __shared__ __attribute__((aligned(16))) unsigned s_e[(TP + 1) * PS];
    extern __shared__ float s_w[];                               // [C]: w[c] - 1
    const unsigned C = A.L.C;
    for (unsigned c = threadIdx.x; c < C; c += NT) s_w[c] = A.w[c] - 1.0f;
    Block<PT, PS, BWD> B;
    B.s_e = s_e; B.s_w = s_w; B.C = C; B.invC = A.invC; B.mse_on = A.mse_on != 0;
    B.scale = BWD ? (float)((double)A.g[0] * A.inv_n) : 0.0f;
    B.bce = 0.0; B.sq = 0.0;
    for (long long tile = blockIdx.x; tile < A.tiles; tile += gridDim.x) {
        const Tile T = tile_of(tile, A.tiles_per_img, A.HW);
        __syncthreads();                                         // the previous tile has been read (and s_w is written)
        stage<PS>(A.L, A.planes + (T.img * A.L.P) * (long long)A.HW + T.p0, A.HW, T.pw, s_e);
        __syncthreads();
        const long long blk = (T.img * A.HW + T.p0) * (long long)C;
        B.x = (const PT*)A.x + blk; B.dx = BWD ? (PT*)A.out + blk : nullptr;
        B.run((int)(T.pw * C));
    }
    if constexpr (!BWD) block_sums(B.bce, B.sq, A.partials);
}

// V = pixels per load: one 16-byte unit (HW % V == 0, x and dx 16-byte aligned) or 1
template <typename PT, int PS, int V, bool BWD>
__global__ __launch_bounds__(NT) void seg_labels_nchw_kernel(const Args A) {
    __shared__ __attribute__((aligned(16))) unsigned s_e[(TP + 1) * PS];
    extern __shared__ float s_w[];
    constexpr int UPR = TP / V, ROWS = NT / UPR, KC = 4;         // KC channels of a lane between two fp64 additions
    const unsigned C = A.L.C, HW = A.HW;
    for (unsigned c = threadIdx.x; c < C; c += NT) s_w[c] = A.w[c] - 1.0f;
    const bool mse_on = A.mse_on != 0;
    const float scale = BWD ? (float)((double)A.g[0] * A.inv_n) : 0.0f;
    const unsigned lu = threadIdx.x % UPR, lrow = threadIdx.x / UPR;
    double bce = 0.0, sq = 0.0;
    for (long long tile = blockIdx.x; tile < A.tiles; tile += gridDim.x) {
        const Tile T = tile_of(tile, A.tiles_per_img, HW);
        __syncthreads();
        stage<PS>(A.L, A.planes + (T.img * A.L.P) * (long long)HW + T.p0, HW, T.pw, s_e);
        __syncthreads();
        if (lu * V < T.pw) {
            unsigned e[V][PS];
#pragma unroll
            for (int i = 0; i < V; ++i) entries<PS>(s_e, lu * V + i, e[i]);
            const long long row0 = (T.img * C) * (long long)HW + T.p0 + lu * V;
            const PT* xr = (const PT*)A.x + row0;
            PT* dr = BWD ? (PT*)A.out + row0 : nullptr;
            for (unsigned cb = lrow; cb < C; cb += KC * ROWS) {
                float fb = 0.0f, fs = 0.0f;
#pragma unroll
                for (int k = 0; k < KC; ++k) {
                    const unsigned c = cb + k * ROWS;
                    if (c < C) {
                        const long long o = (long long)c * HW;
                        float xv[V], out[V];
                        ld_n<PT, V>(xr + o, true, xv);
                        const float wm1 = s_w[c];
#pragma unroll
                        for (int i = 0; i < V; ++i) {
                            const float t = value_of<PS>(e[i], c);
                            if constexpr (BWD) out[i] = elem_bwd(xv[i], t, wm1, mse_on, scale);
                            else elem_fwd(xv[i], t, wm1, mse_on, fb, fs);
                        }
                        if constexpr (BWD) st_n<PT, V>(dr + o, true, out);
                    }
                }
                bce += (double)fb; sq += (double)fs;
            }
        }
    }
    if constexpr (!BWD) block_sums(bce, sq, A.partials);
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
struct Plan { Layout L; long long tiles, n; unsigned tiles_per_img; int blocks; };

int lab_plan(const char* what, const int* groups, int n_groups, int value_channels, int N, int H, int W, Plan* pl) {
    if (N <= 0 || H <= 0 || W <= 0) MAS_FAIL(MAS_EINVAL, "%s: empty shape [%d, %d, %d]", what, N, H, W);
    if (n_groups < 0 || value_channels < 0 || n_groups + value_channels < 1 || n_groups + value_channels > MAS_SEG_MAX_PLANES)
        MAS_FAIL(MAS_EINVAL, "%s: %d groups + %d value channels (1 .. %d planes)", what, n_groups, value_channels, MAS_SEG_MAX_PLANES);
    if (n_groups > 0 && !groups) MAS_FAIL(MAS_EINVAL, "%s: null argument (groups)", what);
    memset(&pl->L, 0, sizeof(pl->L));
    unsigned c = 0;
    for (int g = 0; g < n_groups; ++g) {
        if (groups[g] < 1 || groups[g] > 255) MAS_FAIL(MAS_EINVAL, "%s: group %d has %d classes (1 .. 255)", what, g, groups[g]);
        pl->L.base[g] = c; pl->L.size[g] = (unsigned)groups[g];
        c += (unsigned)groups[g];
    }
    for (int k = 0; k < value_channels; ++k) { pl->L.base[n_groups + k] = c++; pl->L.size[n_groups + k] = 0; }
    pl->L.P = n_groups + value_channels;
    pl->L.C = c;
    const long long hw = (long long)H * W;
    if (hw > (1LL << 30)) MAS_FAIL(MAS_EUNSUPPORTED, "%s: H W = %lld > 2^30", what, hw);
    pl->tiles_per_img = (unsigned)((hw + TP - 1) / TP);
    pl->tiles = (long long)N * pl->tiles_per_img;
    const long long cap = (long long)mas_num_cus() * 8;
    pl->blocks = (int)(pl->tiles < cap ? pl->tiles : cap);
    return MAS_OK;
}

int check_x(const char* what, int x_dtype, int x_layout, int N, int C_out, long long hw, Plan* pl) {
    if (x_dtype != MAS_F32 && x_dtype != MAS_BF16) MAS_FAIL(MAS_EUNSUPPORTED, "%s: dtype %d (fp32 / bf16)", what, x_dtype);
    if (x_layout != MAS_SEG_NCHW && x_layout != MAS_SEG_NHWC) MAS_FAIL(MAS_EINVAL, "%s: layout code %d (MAS_SEG_NCHW or MAS_SEG_NHWC)", what, x_layout);
    if ((double)N * C_out * (double)hw > 4e18) MAS_FAIL(MAS_EUNSUPPORTED, "%s: more than 4e18 elements", what);
    pl->n = (long long)N * C_out * hw;
    return MAS_OK;
}

template <bool BWD>
int lab_run(const char* what, const void* x, int x_dtype, int x_layout, const u8_t* planes, const int* groups, int n_groups, int value_channels,
            const float* w, int N, int H, int W, int mse_on, double* partials, int partial_pairs, const float* g, void* dx, void* stream) {
    MAS_ENTER();
    Plan pl;
    if (int rc = lab_plan(what, groups, n_groups, value_channels, N, H, W, &pl)) return rc;
    const long long hw = (long long)H * W;
    if (int rc = check_x(what, x_dtype, x_layout, N, (int)pl.L.C, hw, &pl)) return rc;
    if (!x || !planes || !w || (BWD ? (!g || !dx) : !partials)) MAS_FAIL(MAS_EINVAL, "%s: null argument", what);
    const size_t xe = mas_esize(x_dtype);
    if (reinterpret_cast<uintptr_t>(x) % xe || (BWD && reinterpret_cast<uintptr_t>(dx) % xe))
        MAS_FAIL(MAS_EINVAL, "%s: a tensor is not aligned to its element size", what);
    if (!BWD && partial_pairs < pl.blocks)
        MAS_FAIL(MAS_EWORKSPACE, "%s: %d {bce, mse} pairs of workspace, mas_seg_loss_labels_blocks says %d", what, partial_pairs, pl.blocks);
    Args A;
    memset(&A, 0, sizeof(A));
    A.L = pl.L; A.planes = planes; A.x = x; A.out = dx; A.w = w; A.tiles = pl.tiles; A.HW = (unsigned)hw; A.tiles_per_img = pl.tiles_per_img;
    A.Cout = pl.L.C; A.invC = 1.0f / (float)pl.L.C; A.mse_on = mse_on != 0; A.g = g; A.inv_n = 1.0 / (double)pl.n; A.partials = partials;
    const dim3 grid((unsigned)pl.blocks), block(NT);
    const size_t lds = (size_t)pl.L.C * sizeof(float);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool wide = pl.L.P > 4;
    const int vu = 16 / (int)xe;
    const bool vec = hw % vu == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0 && (!BWD || reinterpret_cast<uintptr_t>(dx) % 16 == 0);
#define LAB_GO(PT, PS) do { \
        if (x_layout == MAS_SEG_NHWC) hipLaunchKernelGGL((seg_labels_nhwc_kernel<PT, PS, BWD>), grid, block, lds, s, A); \
        else if (vec) hipLaunchKernelGGL((seg_labels_nchw_kernel<PT, PS, 16 / (int)sizeof(PT), BWD>), grid, block, lds, s, A); \
        else hipLaunchKernelGGL((seg_labels_nchw_kernel<PT, PS, 1, BWD>), grid, block, lds, s, A); } while (0)
    if (x_dtype == MAS_BF16) { if (wide) LAB_GO(bf16_t, 8); else LAB_GO(bf16_t, 4); }
    else { if (wide) LAB_GO(float, 8); else LAB_GO(float, 4); }
#undef LAB_GO
    MAS_CHECK_LAUNCH(what);
    return MAS_OK;
}

}  // namespace

extern "C" int mas_seg_expand(const unsigned char* planes, const int* groups, int n_groups, int value_channels, int N, int H, int W, void* out,
                              int out_dtype, int out_layout, int C_pad, void* stream) {
    MAS_ENTER();
    const char* what = "seg_expand";
    Plan pl;
    if (int rc = lab_plan(what, groups, n_groups, value_channels, N, H, W, &pl)) return rc;
    const long long hw = (long long)H * W;
    if (C_pad < (int)pl.L.C || C_pad > 65535) MAS_FAIL(MAS_EINVAL, "%s: C_pad = %d for C = %u channels (C .. 65535)", what, C_pad, pl.L.C);
    if (int rc = check_x(what, out_dtype, out_layout, N, C_pad, hw, &pl)) return rc;
    if (!planes || !out) MAS_FAIL(MAS_EINVAL, "%s: null argument", what);
    const size_t oe = mas_esize(out_dtype);
    if (reinterpret_cast<uintptr_t>(out) % oe) MAS_FAIL(MAS_EINVAL, "%s: the output is not aligned to its element size", what);
    Args A;
    memset(&A, 0, sizeof(A));
    A.L = pl.L; A.planes = planes; A.out = out; A.tiles = pl.tiles; A.HW = (unsigned)hw; A.tiles_per_img = pl.tiles_per_img;
    A.Cout = (unsigned)C_pad;
    const dim3 grid((unsigned)pl.blocks), block(NT);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool wide = pl.L.P > 4, al16 = reinterpret_cast<uintptr_t>(out) % 16 == 0;
    const int vu = 16 / (int)oe;
    const bool vec = al16 && (out_layout == MAS_SEG_NHWC ? C_pad % vu == 0 : hw % vu == 0);
    if (out_layout == MAS_SEG_NHWC) A.invC = 1.0f / (float)(vec ? C_pad / vu : C_pad);
#define EXP_GO(OT, PS) do { \
        constexpr int VU = 16 / (int)sizeof(OT); \
        if (out_layout == MAS_SEG_NHWC) { \
            if (vec) hipLaunchKernelGGL((seg_expand_nhwc_kernel<OT, PS, VU>), grid, block, 0, s, A); \
            else hipLaunchKernelGGL((seg_expand_nhwc_kernel<OT, PS, 1>), grid, block, 0, s, A); \
        } else { \
            if (vec) hipLaunchKernelGGL((seg_expand_nchw_kernel<OT, PS, VU>), grid, block, 0, s, A); \
            else hipLaunchKernelGGL((seg_expand_nchw_kernel<OT, PS, 1>), grid, block, 0, s, A); \
        } } while (0)
    if (out_dtype == MAS_BF16) { if (wide) EXP_GO(bf16_t, 8); else EXP_GO(bf16_t, 4); }
    else { if (wide) EXP_GO(float, 8); else EXP_GO(float, 4); }
#undef EXP_GO
    MAS_CHECK_LAUNCH(what);
    return MAS_OK;
}

extern "C" int mas_seg_loss_labels_blocks(const int* groups, int n_groups, int value_channels, int N, int H, int W, int x_dtype, int x_layout) {
    Plan pl;
    if (int rc = lab_plan("seg_loss_labels_blocks", groups, n_groups, value_channels, N, H, W, &pl)) return rc;
    if (int rc = check_x("seg_loss_labels_blocks", x_dtype, x_layout, N, (int)pl.L.C, (long long)H * W, &pl)) return rc;
    return pl.blocks;
}

extern "C" int mas_seg_loss_labels_fwd(const void* x, int x_dtype, int x_layout, const unsigned char* planes, const int* groups, int n_groups,
                                       int value_channels, const float* pos_weight, int N, int H, int W, int mse_on, double* partials,
                                       int partial_pairs, void* stream) {
    return lab_run<false>("seg_loss_labels_fwd", x, x_dtype, x_layout, planes, groups, n_groups, value_channels, pos_weight, N, H, W, mse_on,
                          partials, partial_pairs, nullptr, nullptr, stream);
}

extern "C" int mas_seg_loss_labels_bwd(const void* x, int x_dtype, int x_layout, const unsigned char* planes, const int* groups, int n_groups,
                                       int value_channels, const float* pos_weight, int N, int H, int W, int mse_on, const float* grad, void* dx,
                                       void* stream) {
    return lab_run<true>("seg_loss_labels_bwd", x, x_dtype, x_layout, planes, groups, n_groups, value_channels, pos_weight, N, H, W, mse_on,
                         nullptr, 0, grad, dx, stream);
}
