// The VQ-SEG objective for gfx950 (reference losses/loss_seg.py:6-41: binary_cross_entropy_with_logits(pos_weight) over the 159-channel map,
// plus mse_loss(sigmoid) in VQVAEWithBCELoss), for x = prediction logits, t = target, w[c] = positive weight of channel c, n = N C H W:
//   lw = 1 + (w[c] - 1) t       bce = (1 - t) x + lw softplus(-x)       mse = (sigma(x) - t)^2       loss = mean(bce) + mse_on mean(mse)
//   dx = g / n [ (1 - t) - lw (1 - sigma) + mse_on 2 (sigma - t) sigma (1 - sigma) ]
// with e = exp(-|x|), softplus(-x) = max(-x, 0) + log(1 + e), sigma = (x >= 0 ? 1 : e) / (1 + e), 1 - sigma = (x >= 0 ? e : 1) / (1 + e): one
// exponential whose argument is never positive, so nothing overflows at either end and 1 - sigma never cancels.
//   * seg_loss_fwd    : ONE read of x and t -> one {bce_sum, mse_sum} pair per work-group in fp64 (a lane adds in fp32 within one tile only)
//   * seg_loss_reduce : one work-group, fixed order, no atomics -> {loss, bce_mean, mse_mean} fp32, each rounded once from fp64
//   * seg_loss_bwd    : one read of x and t, one write of dx in x's dtype AND x's memory layout; g from a device scalar
// Each tensor is dense NCHW or dense NHWC on its own, and neither is copied.  Two shapes of kernel:
//   flat  (same layout): the tensor is one array of n elements, cut into tiles of 256 lanes x 4 units x 16 bytes; the 16-byte units start
//         at the first 16-byte boundary of the ARRAY (a 159-channel pixel is 636 bytes: no pixel is aligned, the array is), the few
//         elements before and after go one by one.  The channel is i mod C (NHWC) or (i / HW) mod C (NCHW), carried from tile to tile
//         as a remainder, so the loop holds no 64-bit division.
//   mixed (layouts differ): a tile is P consecutive pixels of one image x all C channels.  The TARGET goes through LDS as fp32, written
//         in its own memory order and read in the prediction's, image [pixel][channel] with a row pitch of C | 1 dwords: the side whose
//         lanes run over pixels at a fixed channel then strides by an odd number of banks.  x is read, and dx written, straight in the
//         prediction's layout: as one contiguous block of P C elements in 16-byte units (NHWC), or as C rows of P elements (NCHW).
//         P = 32 at C = 159 (21 KB, six work-groups per CU); with an odd C the image is the NHWC block in its own order, shifted so that
//         the 16-byte units of x are 16-byte aligned in LDS too and a lane reads its targets with ds_read_b128.
// The weights sit in LDS as w[c] - 1; no load is indexed by a data value.  The grid depends on the shape and the CU count only.
#include "mas_common.h"
#include "seg_elem.h"     // ld_n / st_n, divmod, Pre, elem_fwd, elem_bwd, block_sums: shared with seg_labels.hip
#include <math.h>

namespace {

constexpr int NT = SEG_NT;
constexpr int KU = 4;                    // 16-byte units of x per lane and tile (flat kernel)
constexpr int LDS_TILE_BUDGET = 24 * 1024;   // bytes of LDS per work-group of the mixed kernel: six work-groups per CU (48 KB / three: 1.6x slower)
typedef unsigned char u8_t;

enum { L_NCHW = MAS_SEG_NCHW, L_NHWC = MAS_SEG_NHWC };

// One contiguous span of x (and of dx) walked by the whole work-group.  XL says how the channel follows from the offset j in the span:
// L_NHWC: channel (c0 + j) mod C (and, with the target in LDS, pixel (c0 + j) / C of the tile, c0 = 0); L_NCHW: the span starts r0 elements
// into a plane of channel c0, and a plane is HW elements.  The target comes from global memory at the same offsets or from the LDS tile.
template <typename PT, typename TT, int XL, bool LDS_T, bool BWD>
struct Span {
    static constexpr int U = 16 / (int)sizeof(PT);
    const PT* x; PT* dx; const TT* t; const float* s_t; const float* s_w;
    unsigned C, HW, c0, r0, pad;
    float invC, invHW, scale;
    bool mse_on;
    float bce, sq;

    template <int N>
    __device__ __forceinline__ void proc(int j, bool tvec, bool dvec) {
        float xv[N], tv[N], out[N];
        ld_n<PT, N>(x + j, true, xv);
        if constexpr (!LDS_T) ld_n<TT, N>(t + j, tvec, tv);
        constexpr bool LDS_VEC = LDS_T && N >= 4;                // pad == 0: the tile is the block's own order, and run() made the units 16-byte aligned in LDS
        unsigned c, r = 0, a = 0;
        if constexpr (XL == L_NHWC) {
            unsigned p;
            divmod(c0 + (unsigned)j, C, invC, p, c);
            a = (unsigned)j + p * pad;
            if constexpr (LDS_VEC) {
                if (pad == 0) {
#pragma unroll
                    for (int k = 0; k < N / 4; ++k) {
                        const f32x4 q4 = *reinterpret_cast<const f32x4*>(s_t + a + 4 * k);
                        tv[4 * k] = q4[0]; tv[4 * k + 1] = q4[1]; tv[4 * k + 2] = q4[2]; tv[4 * k + 3] = q4[3];
                    }
                }
            }
        } else {
            unsigned q;
            divmod(r0 + (unsigned)j, HW, invHW, q, r);
            divmod(c0 + q, C, invC, q, c);
        }
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const float tt = (LDS_T && !(LDS_VEC && pad == 0)) ? s_t[a] : tv[e];
            const float wm1 = s_w[c];
            if constexpr (BWD) out[e] = elem_bwd(xv[e], tt, wm1, mse_on, scale);
            else elem_fwd(xv[e], tt, wm1, mse_on, bce, sq);
            if constexpr (XL == L_NHWC) {
                a += 1;
                if (++c == C) { c = 0; a += pad; }
            } else {
                if (++r == HW) { r = 0; if (++c == C) c = 0; }
            }
        }
        if constexpr (BWD) st_n<PT, N>(dx + j, dvec, out);
    }

    __device__ __forceinline__ void run(int len) {
        const int tid = threadIdx.x;
        int head = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(x) & 15)) & 15) / sizeof(PT));   // elements ahead of the first 16-byte unit
        if (head > len) head = len;
        const int nunits = (len - head) / U, tail0 = head + nunits * U;
        const bool tvec = LDS_T ? false : aligned_to(t + head, Chunk<TT, U>::BYTES);
        const bool dvec = BWD ? aligned_to(dx + head, 16) : false;
        if (tid < head) proc<1>(tid, false, false);
        if (tid >= 64 && tid - 64 < len - tail0) proc<1>(tail0 + tid - 64, false, false);                // (head, tail < U <= 8)
#pragma unroll 2
        for (int u = tid; u < nunits; u += NT) proc<U>(head + u * U, tvec, dvec);
    }
};

struct Args {
    const void* x; void* dx; const void* t; const float* w;
    long long n, tiles;                  // elements; tiles in all
    unsigned C, HW;
    unsigned step_c, step_r;             // flat: how (c0, r0) move when a work-group goes on by gridDim tiles
    unsigned P, Cp, tiles_per_img;       // mixed
    float invC, invHW;
    int mse_on;
    const float* g; double inv_n;        // backward
    double* partials;                    // forward
};

template <typename PT, typename TT, int XL, bool BWD>
__global__ __launch_bounds__(NT) void seg_flat_kernel(const Args A) {
    extern __shared__ float s_w[];                               // [C]: w[c] - 1
    constexpr int TE = NT * KU * (16 / (int)sizeof(PT));
    for (unsigned c = threadIdx.x; c < A.C; c += NT) s_w[c] = A.w[c] - 1.0f;
    __syncthreads();
    Span<PT, TT, XL, false, BWD> sp;
    sp.s_t = nullptr; sp.s_w = s_w; sp.C = A.C; sp.HW = A.HW; sp.pad = 0; sp.invC = A.invC; sp.invHW = A.invHW; sp.mse_on = A.mse_on != 0;
    sp.scale = BWD ? (float)((double)A.g[0] * A.inv_n) : 0.0f;
    const long long first = (long long)blockIdx.x * TE;          // the one 64-bit division: where this work-group's first tile starts
    unsigned c0, r0 = 0;
    if (XL == L_NHWC) c0 = (unsigned)(first % A.C);
    else { r0 = (unsigned)(first % A.HW); c0 = (unsigned)((first / A.HW) % A.C); }
    double bce = 0.0, sq = 0.0;
    for (long long tile = blockIdx.x; tile < A.tiles; tile += gridDim.x) {
        const long long i0 = tile * TE;
        const long long left = A.n - i0;
        sp.x = (const PT*)A.x + i0; sp.dx = BWD ? (PT*)A.dx + i0 : nullptr; sp.t = (const TT*)A.t + i0;
        sp.c0 = c0; sp.r0 = r0; sp.bce = 0.0f; sp.sq = 0.0f;
        sp.run(left < TE ? (int)left : TE);
        bce += (double)sp.bce; sq += (double)sp.sq;
        if (XL == L_NHWC) { c0 += A.step_c; if (c0 >= A.C) c0 -= A.C; }
        else {
            r0 += A.step_r;
            unsigned carry = 0;
            if (r0 >= A.HW) { r0 -= A.HW; carry = 1; }
            c0 += A.step_c + carry;
            if (c0 >= A.C) c0 -= A.C;
        }
    }
    if constexpr (!BWD) block_sums(bce, sq, A.partials);
}

// XL = the prediction's layout; the target has the other one
template <typename PT, typename TT, int XL, bool BWD>
__global__ __launch_bounds__(NT) void seg_mixed_kernel(const Args A) {
    extern __shared__ __attribute__((aligned(16))) float s_all[];
    float* s_t = s_all;                                          // [P][Cp] the target tile as fp32
    float* s_w = s_all + (size_t)A.P * A.Cp + 4;                 // [C] (4: room for the shift below)
    const int tid = threadIdx.x;
    const unsigned C = A.C, HW = A.HW, P = A.P, Cp = A.Cp, pad = Cp - C;
    for (unsigned c = tid; c < C; c += NT) s_w[c] = A.w[c] - 1.0f;
    const bool mse_on = A.mse_on != 0;
    const float scale = BWD ? (float)((double)A.g[0] * A.inv_n) : 0.0f;
    const unsigned lp = tid & (P - 1), lrow = tid / P, rows = NT / P;   // P is a power of two <= 64
    double bce = 0.0, sq = 0.0;
    for (long long tile = blockIdx.x; tile < A.tiles; tile += gridDim.x) {
        const long long img = tile / A.tiles_per_img;
        const unsigned p0 = (unsigned)(tile - img * A.tiles_per_img) * P;
        const unsigned pw = HW - p0 < P ? HW - p0 : P;
        const long long ibase = img * (long long)C * HW;
        const long long blk = ibase + (long long)p0 * C;         // the NHWC side: pw C contiguous elements
        const long long row0 = ibase + p0;                       // the NCHW side: row c at row0 + c HW, pw elements
        __syncthreads();                                         // the previous tile has been read (and s_w is written)
        if constexpr (XL == L_NHWC) {
            // target rows -> LDS [pixel][channel]: lanes run over pixels, pitch Cp is odd
            // With an odd C the pitch is C itself and the image is the block in its own order; it is shifted by up to 3 dwords so that
            // the 16-byte units of x, which start at the block's first 16-byte boundary in MEMORY, are 16-byte aligned in LDS as well:
            // the span then reads its four (eight) targets as one (two) ds_read_b128 instead of conflicting dword reads.
            const TT* tr = (const TT*)A.t + row0;
            const PT* xb = (const PT*)A.x + blk;
            const unsigned xhead = ((16u - (unsigned)(reinterpret_cast<uintptr_t>(xb) & 15)) & 15) / (unsigned)sizeof(PT);
            float* s_img = s_t + (pad == 0 ? (4u - (xhead & 3)) & 3 : 0u);
            if (lp < pw) {
#pragma unroll 8
                for (unsigned c = lrow; c < C; c += rows) s_img[lp * Cp + c] = to_f(tr[(long long)c * HW + lp]);
            }
            __syncthreads();
            Span<PT, TT, L_NHWC, true, BWD> sp;
            sp.x = xb; sp.dx = BWD ? (PT*)A.dx + blk : nullptr; sp.t = nullptr; sp.s_t = s_img; sp.s_w = s_w;
            sp.C = C; sp.HW = HW; sp.c0 = 0; sp.r0 = 0; sp.pad = pad; sp.invC = A.invC; sp.invHW = A.invHW; sp.scale = scale;
            sp.mse_on = mse_on; sp.bce = 0.0f; sp.sq = 0.0f;
            sp.run((int)(pw * C));
            bce += (double)sp.bce; sq += (double)sp.sq;
        } else {
            // target block -> LDS in its own order (element j of the block at j + (j / C) pad), four elements at a time where aligned
            const TT* tb = (const TT*)A.t + blk;
            const int len = (int)(pw * C);
            constexpr unsigned QB = 4 * sizeof(TT);
            int head = (int)(((QB - (unsigned)(reinterpret_cast<uintptr_t>(tb) & (QB - 1))) & (QB - 1)) / sizeof(TT));
            if (head > len) head = len;
            const int nq = (len - head) / 4, tail0 = head + nq * 4;
            if (tid < head) { unsigned p, c; divmod((unsigned)tid, C, A.invC, p, c); s_t[tid + p * pad] = to_f(tb[tid]); }
            if (tid >= 64 && tid - 64 < len - tail0) {
                const unsigned j = (unsigned)(tail0 + tid - 64);
                unsigned p, c; divmod(j, C, A.invC, p, c);
                s_t[j + p * pad] = to_f(tb[j]);
            }
#pragma unroll 2
            for (int q = tid; q < nq; q += NT) {
                const unsigned j = (unsigned)(head + q * 4);
                float v[4];
                ld_n<TT, 4>(tb + j, true, v);
                unsigned p, c; divmod(j, C, A.invC, p, c);
                unsigned a = j + p * pad;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    s_t[a] = v[e];
                    a += 1;
                    if (++c == C) { c = 0; a += pad; }
                }
            }
            __syncthreads();
            // x rows: lanes run over pixels at a fixed channel
            const PT* xr = (const PT*)A.x + row0;
            PT* dr = BWD ? (PT*)A.dx + row0 : nullptr;
            float fb = 0.0f, fs = 0.0f;
            if (lp < pw) {
#pragma unroll 4
                for (unsigned c = lrow; c < C; c += rows) {
                    const long long o = (long long)c * HW + lp;
                    const float xv = to_f(xr[o]), tt = s_t[lp * Cp + c], wm1 = s_w[c];
                    if constexpr (BWD) dr[o] = (PT)elem_bwd(xv, tt, wm1, mse_on, scale);
                    else elem_fwd(xv, tt, wm1, mse_on, fb, fs);
                }
            }
            bce += (double)fb; sq += (double)fs;
        }
    }
    if constexpr (!BWD) block_sums(bce, sq, A.partials);
}

// One work-group: lane i adds pairs i, i + 256, ... in fp64, then a fixed tree; the three results are each rounded once.
__global__ __launch_bounds__(NT) void seg_reduce_kernel(const double* __restrict__ partials, int blocks, double inv_n, int mse_on,
                                                        float* __restrict__ out) {
    __shared__ double s_b[NT], s_s[NT];
    const int tid = threadIdx.x;
    double b = 0.0, s = 0.0;
    for (int i = tid; i < blocks; i += NT) { b += partials[2 * (size_t)i]; s += partials[2 * (size_t)i + 1]; }
    s_b[tid] = b; s_s[tid] = s;
    __syncthreads();
    for (int o = NT / 2; o >= 1; o >>= 1) {
        if (tid < o) { s_b[tid] += s_b[tid + o]; s_s[tid] += s_s[tid + o]; }
        __syncthreads();
    }
    if (tid == 0) {
        const double bm = s_b[0] * inv_n, sm = mse_on ? s_s[0] * inv_n : 0.0;
        out[0] = (float)(bm + sm);
        out[1] = (float)bm;
        out[2] = (float)sm;
    }
}

struct Plan {
    bool mixed;
    long long n, tiles;
    int blocks;
    unsigned P, Cp, tiles_per_img, te;
    size_t lds;
};

int seg_plan(const char* what, int N, int C, int H, int W, int x_dtype, int x_layout, int t_layout, Plan* pl) {
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0) MAS_FAIL(MAS_EINVAL, "%s: empty shape [%d, %d, %d, %d]", what, N, C, H, W);
    if (x_dtype != MAS_F32 && x_dtype != MAS_BF16) MAS_FAIL(MAS_EUNSUPPORTED, "%s: prediction dtype %d (fp32 / bf16)", what, x_dtype);
    if ((x_layout != MAS_SEG_NCHW && x_layout != MAS_SEG_NHWC) || (t_layout != MAS_SEG_NCHW && t_layout != MAS_SEG_NHWC))
        MAS_FAIL(MAS_EINVAL, "%s: layout codes %d / %d (MAS_SEG_NCHW or MAS_SEG_NHWC)", what, x_layout, t_layout);
    const long long hw = (long long)H * W;
    if (hw > (1LL << 30) || C > (1 << 20)) MAS_FAIL(MAS_EUNSUPPORTED, "%s: H W = %lld > 2^30 or C = %d > 2^20", what, hw, C);
    if ((double)N * C * (double)hw > 4e18) MAS_FAIL(MAS_EUNSUPPORTED, "%s: more than 4e18 elements", what);
    pl->n = (long long)N * C * hw;
    pl->mixed = x_layout != t_layout && C > 1 && hw > 1;         // (one channel or one pixel: the two layouts are the same array)
    const int cus = mas_num_cus();
    if (!pl->mixed) {
        pl->te = NT * KU * (x_dtype == MAS_BF16 ? 8 : 4);
        pl->tiles = (pl->n + pl->te - 1) / pl->te;
        pl->lds = (size_t)C * sizeof(float);
        if (pl->lds > 60 * 1024) MAS_FAIL(MAS_EUNSUPPORTED, "%s: C = %d weights do not fit in LDS", what, C);   // (+ the forward's fp64 tree)
        pl->blocks = (int)(pl->tiles < (long long)cus * 8 ? pl->tiles : (long long)cus * 8);
        pl->P = pl->Cp = pl->tiles_per_img = 0;
    } else {
        const unsigned Cp = (unsigned)C | 1u;                    // odd pitch in dwords
        unsigned P = 64;
        while (P > 1 && ((size_t)P * Cp + 4 + C) * sizeof(float) > (size_t)LDS_TILE_BUDGET) P >>= 1;
        pl->lds = ((size_t)P * Cp + 4 + C) * sizeof(float);
        if (pl->lds > 60 * 1024) MAS_FAIL(MAS_EUNSUPPORTED, "%s: C = %d: one pixel of targets does not fit in LDS", what, C);
        pl->P = P; pl->Cp = Cp; pl->te = 0;
        pl->tiles_per_img = (unsigned)((hw + P - 1) / P);
        pl->tiles = (long long)N * pl->tiles_per_img;
        int per_cu = (int)((150 * 1024) / (pl->lds + 4096));     // (+ the fp64 tree of the forward)
        per_cu = per_cu < 1 ? 1 : per_cu > 8 ? 8 : per_cu;
        pl->blocks = (int)(pl->tiles < (long long)cus * per_cu ? pl->tiles : (long long)cus * per_cu);
    }
    return MAS_OK;
}

template <typename PT, typename TT, bool BWD>
void seg_launch(const Plan& pl, const Args& A, int x_layout, hipStream_t s) {
    const dim3 grid((unsigned)pl.blocks), block(NT);
    if (!pl.mixed) {
        if (x_layout == MAS_SEG_NHWC) hipLaunchKernelGGL((seg_flat_kernel<PT, TT, L_NHWC, BWD>), grid, block, pl.lds, s, A);
        else hipLaunchKernelGGL((seg_flat_kernel<PT, TT, L_NCHW, BWD>), grid, block, pl.lds, s, A);
    } else {
        if (x_layout == MAS_SEG_NHWC) hipLaunchKernelGGL((seg_mixed_kernel<PT, TT, L_NHWC, BWD>), grid, block, pl.lds, s, A);
        else hipLaunchKernelGGL((seg_mixed_kernel<PT, TT, L_NCHW, BWD>), grid, block, pl.lds, s, A);
    }
}

template <bool BWD>
int seg_run(const char* what, const void* x, int x_dtype, int x_layout, const void* t, int t_dtype, int t_layout, const float* w, int N, int C,
            int H, int W, int mse_on, double* partials, int partial_pairs, const float* g, void* dx, void* stream) {
    MAS_ENTER();
    Plan pl;
    if (int rc = seg_plan(what, N, C, H, W, x_dtype, x_layout, t_layout, &pl)) return rc;
    if (!x || !t || !w || (BWD ? (!g || !dx) : !partials)) MAS_FAIL(MAS_EINVAL, "%s: null argument", what);
    if (t_dtype != MAS_F32 && t_dtype != MAS_BF16 && t_dtype != MAS_SEG_U8)
        MAS_FAIL(MAS_EUNSUPPORTED, "%s: target dtype %d (fp32 / bf16 / uint8)", what, t_dtype);
    const size_t xe = mas_esize(x_dtype), te = t_dtype == MAS_SEG_U8 ? 1 : mas_esize(t_dtype);
    if (reinterpret_cast<uintptr_t>(x) % xe || reinterpret_cast<uintptr_t>(t) % te || (BWD && reinterpret_cast<uintptr_t>(dx) % xe))
        MAS_FAIL(MAS_EINVAL, "%s: a tensor is not aligned to its element size", what);
    if (!BWD && partial_pairs < pl.blocks)
        MAS_FAIL(MAS_EWORKSPACE, "%s: %d {bce, mse} pairs of workspace, mas_seg_loss_blocks says %d", what, partial_pairs, pl.blocks);
    Args A;
    memset(&A, 0, sizeof(A));
    A.x = x; A.dx = dx; A.t = t; A.w = w; A.n = pl.n; A.tiles = pl.tiles; A.C = (unsigned)C; A.HW = (unsigned)(H * W);
    A.P = pl.P; A.Cp = pl.Cp; A.tiles_per_img = pl.tiles_per_img;
    A.invC = 1.0f / (float)C; A.invHW = 1.0f / (float)A.HW; A.mse_on = mse_on != 0; A.g = g; A.inv_n = 1.0 / (double)pl.n;
    A.partials = partials;
    if (!pl.mixed) {
        const long long step = (long long)pl.blocks * pl.te;
        if (x_layout == MAS_SEG_NHWC) A.step_c = (unsigned)(step % C);
        else { A.step_r = (unsigned)(step % A.HW); A.step_c = (unsigned)((step / A.HW) % C); }
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
#define SEG_T(PT) do { \
        if (t_dtype == MAS_F32) seg_launch<PT, float, BWD>(pl, A, x_layout, s); \
        else if (t_dtype == MAS_BF16) seg_launch<PT, bf16_t, BWD>(pl, A, x_layout, s); \
        else seg_launch<PT, u8_t, BWD>(pl, A, x_layout, s); } while (0)
    if (x_dtype == MAS_BF16) SEG_T(bf16_t); else SEG_T(float);
#undef SEG_T
    MAS_CHECK_LAUNCH(what);
    return MAS_OK;
}

}  // namespace

extern "C" int mas_seg_loss_blocks(int N, int C, int H, int W, int x_dtype, int x_layout, int t_layout) {
    Plan pl;
    if (int rc = seg_plan("seg_loss_blocks", N, C, H, W, x_dtype, x_layout, t_layout, &pl)) return rc;
    return pl.blocks;
}

extern "C" int mas_seg_loss_fwd(const void* x, int x_dtype, int x_layout, const void* t, int t_dtype, int t_layout, const float* pos_weight,
                                int N, int C, int H, int W, int mse_on, double* partials, int partial_pairs, void* stream) {
    return seg_run<false>("seg_loss_fwd", x, x_dtype, x_layout, t, t_dtype, t_layout, pos_weight, N, C, H, W, mse_on, partials, partial_pairs,
                          nullptr, nullptr, stream);
}

extern "C" int mas_seg_loss_reduce(const double* partials, int partial_pairs, long long numel, int mse_on, float* out, void* stream) {
    MAS_ENTER();
    if (!partials || !out) MAS_FAIL(MAS_EINVAL, "seg_loss_reduce: null argument");
    if (partial_pairs <= 0 || numel <= 0) MAS_FAIL(MAS_EINVAL, "seg_loss_reduce: pairs=%d numel=%lld must be positive", partial_pairs, numel);
    hipLaunchKernelGGL(seg_reduce_kernel, dim3(1), dim3(NT), 0, reinterpret_cast<hipStream_t>(stream), partials, partial_pairs,
                       1.0 / (double)numel, mse_on != 0, out);
    MAS_CHECK_LAUNCH("seg_loss_reduce");
    return MAS_OK;
}

extern "C" int mas_seg_loss_bwd(const void* x, int x_dtype, int x_layout, const void* t, int t_dtype, int t_layout, const float* pos_weight,
                                int N, int C, int H, int W, int mse_on, const float* grad, void* dx, void* stream) {
    return seg_run<true>("seg_loss_bwd", x, x_dtype, x_layout, t, t_dtype, t_layout, pos_weight, N, C, H, W, mse_on, nullptr, 0, grad, dx,
                         stream);
}
