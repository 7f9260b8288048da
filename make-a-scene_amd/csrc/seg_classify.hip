// VQ-SEG logits back to label planes, and the counts a validation metric is made of.  The reference reads a reconstruction
// with log_utils.py:55-67: per group a slice argmax, and for the face and edge groups the argmax one-hot times `sigmoid > 0.2`.  Restated
// without a sigmoid (the argmax channel has the largest sigmoid, and sigmoid(x) > t <=> x > log(t / (1 - t)) = tau):
//   class plane (channels base .. base + S - 1): m = the largest logit, a = the FIRST channel that holds it; byte = m > tau ? a - base + 1 : 0
//   value plane (one channel)                  : byte = x > tau
// with tau = -inf where a plane has no threshold.  Logits are compared as fp32 (bf16 widens exactly): no rounding anywhere, the bytes are
// exact.  A NaN never wins a `>`: the byte stays within 0 .. S.
//   * seg_classify, NCHW: a lane owns V consecutive pixels (one 16-byte unit where the rows are 16-byte aligned, one pixel otherwise) and
//        walks the channels of a plane with {max, index} in registers, KC loads in flight; a wave reads 1 KB of one row at a time.  One
//        store of V bytes per plane.  The prediction is read exactly once.
//   * seg_classify, NHWC: a work-group takes SP pixels x all channels -- one contiguous block -- into LDS as fp32 with 16-byte loads
//        (head and tail elements one by one, as seg_labels.hip walks such a block), pixel rows padded to an ODD length, so that lane p
//        scanning its pixel's channels meets no bank conflict.  SP = what 40 KB of LDS hold, 256 at the most.
//   * seg_agreement: two plane tensors -> {inter, pred, target}[C], agree[P], pixels as 64-bit integer counts ADDED to the caller's buffer.
//        Class bytes index a work-group histogram in LDS only after the 1 <= v <= S check; value planes and `agree` count in registers.
//        One 64-bit integer atomic per non-zero counter and work-group at the end: integer sums are exact in any order.
// Grids depend on the shape and the CU count only; 64-bit offsets; no float atomics; nothing synchronises with the host.
#include "mas_common.h"
#include "seg_elem.h"
#include <math.h>

namespace {

constexpr int NT = SEG_NT;
constexpr int MAXP = MAS_SEG_MAX_PLANES;
constexpr int KC = 8;                                   // channels of a lane in flight (NCHW)
constexpr unsigned NHWC_LDS_BYTES = 40960;
typedef unsigned char u8_t;

struct CLayout {
    int P;
    unsigned C;
    unsigned base[MAXP], size[MAXP];                    // size 0: a value plane
    float tau[MAXP];
};

struct CArgs {
    CLayout L;
    const void* x;
    u8_t* planes;
    long long units;                                    // NCHW: lanes' work items; NHWC: tiles
    unsigned HW, upi;                                   // upi: units (tiles) per image
    unsigned SP, Cs;                                    // NHWC: pixels per tile, LDS row length (odd)
    float invC;
};

struct GArgs {
    CLayout L;
    const u8_t* pred; const u8_t* target;
    unsigned long long* counts;                         // [3][C], [P], [1]
    long long units, pixels;
    unsigned HW, upi;
};

template <int V> struct Bytes;
template <> struct Bytes<1> {
    static __device__ __forceinline__ void st(u8_t* p, const unsigned (&b)[1]) { p[0] = (u8_t)b[0]; }
    static __device__ __forceinline__ void ld(const u8_t* p, unsigned (&b)[1]) { b[0] = p[0]; }
};
template <> struct Bytes<4> {
    static __device__ __forceinline__ void st(u8_t* p, const unsigned (&b)[4]) {
        *reinterpret_cast<unsigned*>(p) = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
    }
    static __device__ __forceinline__ void ld(const u8_t* p, unsigned (&b)[4]) {
        const unsigned w = *reinterpret_cast<const unsigned*>(p);
        b[0] = w & 0xffu; b[1] = (w >> 8) & 0xffu; b[2] = (w >> 16) & 0xffu; b[3] = w >> 24;
    }
};
template <> struct Bytes<8> {
    static __device__ __forceinline__ void st(u8_t* p, const unsigned (&b)[8]) {
        *reinterpret_cast<u32x2*>(p) = u32x2{b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24), b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24)};
    }
};

// ---- classify ---------------------------------------------------------------------------------------------------------------------
// V = pixels per lane: one 16-byte unit (HW % V == 0, x 16-byte and planes 8-byte aligned) or 1
template <typename PT, int V>
__global__ __launch_bounds__(NT) void seg_classify_nchw_kernel(const CArgs A) {
    const unsigned HW = A.HW;
    for (long long u = (long long)blockIdx.x * NT + threadIdx.x; u < A.units; u += (long long)gridDim.x * NT) {
        const long long img = u / A.upi;
        const unsigned p0 = (unsigned)(u - img * A.upi) * V;
        const PT* xr = (const PT*)A.x + (img * A.L.C) * (long long)HW + p0;
        u8_t* ob = A.planes + (img * A.L.P) * (long long)HW + p0;
        for (int k = 0; k < A.L.P; ++k) {
            const unsigned size = A.L.size[k];
            const float tau = A.L.tau[k];
            const PT* xb = xr + (long long)A.L.base[k] * HW;
            float m[V];
            unsigned a[V], b[V];
            ld_n<PT, V>(xb, true, m);
#pragma unroll
            for (int i = 0; i < V; ++i) a[i] = 0;
            // channels past the group's last are read as its last: a repeated value never wins the strict `>`
            for (unsigned j0 = 1; j0 < size; j0 += KC) {
                float xv[KC][V];
                unsigned jj[KC];
#pragma unroll
                for (int q = 0; q < KC; ++q) {
                    jj[q] = j0 + q < size ? j0 + q : size - 1;
                    ld_n<PT, V>(xb + (long long)jj[q] * HW, true, xv[q]);
                }
#pragma unroll
                for (int q = 0; q < KC; ++q)
#pragma unroll
                    for (int i = 0; i < V; ++i)
                        if (xv[q][i] > m[i]) { m[i] = xv[q][i]; a[i] = jj[q]; }
            }
#pragma unroll
            for (int i = 0; i < V; ++i) b[i] = m[i] > tau ? a[i] + 1u : 0u;     // (a value plane: a = 0)
            Bytes<V>::st(ob + (long long)k * HW, b);
        }
    }
}

template <typename PT>
__global__ __launch_bounds__(NT) void seg_classify_nhwc_kernel(const CArgs A) {
    extern __shared__ __attribute__((aligned(16))) float s_x[];      // [SP][Cs]
    constexpr int U = 16 / (int)sizeof(PT);
    const unsigned C = A.L.C, Cs = A.Cs, HW = A.HW, tid = threadIdx.x;
    for (long long t = blockIdx.x; t < A.units; t += gridDim.x) {
        const long long img = t / A.upi;
        const unsigned s0 = (unsigned)(t - img * A.upi) * A.SP;
        const unsigned sw = HW - s0 < A.SP ? HW - s0 : A.SP;
        const PT* xb = (const PT*)A.x + (img * HW + s0) * (long long)C;
        const unsigned len = sw * C;
        unsigned head = (unsigned)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(xb) & 15)) & 15) / sizeof(PT));
        if (head > len) head = len;
        const unsigned nunits = (len - head) / U, tail0 = head + nunits * U;
        __syncthreads();                                             // the previous tile has been scanned
        if (tid < head || (tid >= 64 && tid - 64 < len - tail0)) {   // (head, tail < U <= 8)
            const unsigned e = tid < head ? tid : tail0 + tid - 64;
            unsigned p, c;
            divmod(e, C, A.invC, p, c);
            s_x[p * Cs + c] = to_f(xb[e]);
        }
#pragma unroll 2
        for (unsigned q = tid; q < nunits; q += NT) {
            const unsigned e = head + q * U;
            float v[U];
            ld_n<PT, U>(xb + e, true, v);
            unsigned p, c;
            divmod(e, C, A.invC, p, c);
#pragma unroll
            for (int i = 0; i < U; ++i) {
                s_x[p * Cs + c] = v[i];
                if (++c == C) { c = 0; ++p; }
            }
        }
        __syncthreads();
        if (tid < sw) {
            const float* row = s_x + tid * Cs;
            u8_t* ob = A.planes + (img * A.L.P) * (long long)HW + s0 + tid;
            for (int k = 0; k < A.L.P; ++k) {
                const unsigned size = A.L.size[k];
                const float* g = row + A.L.base[k];
                float m = g[0];
                unsigned a = 0;
#pragma unroll 8
                for (unsigned j = 1; j < size; ++j) {
                    const float xv = g[j];
                    if (xv > m) { m = xv; a = j; }
                }
                ob[(long long)k * HW] = (u8_t)(m > A.L.tau[k] ? a + 1u : 0u);
            }
        }
    }
}

// ---- agreement --------------------------------------------------------------------------------------------------------------------
// V = pixels per lane: 4 (HW % 4 == 0, both tensors 4-byte aligned) or 1
template <int V>
__global__ __launch_bounds__(NT) void seg_agreement_kernel(const GArgs A) {
    extern __shared__ unsigned s_h[];                                // [3][C] {inter, pred, target}, [P] agree: the layout of `counts`
    const unsigned C = A.L.C, HW = A.HW, tid = threadIdx.x;
    const unsigned nh = 3 * C + (unsigned)A.L.P;
    for (unsigned i = tid; i < nh; i += NT) s_h[i] = 0;
    __syncthreads();
    for (int k = 0; k < A.L.P; ++k) {                                // plane by plane: a value plane and `agree` count in registers
        const unsigned size = A.L.size[k], base = A.L.base[k];
        unsigned n_agree = 0, n_i = 0, n_p = 0, n_t = 0;
        for (long long u = (long long)blockIdx.x * NT + tid; u < A.units; u += (long long)gridDim.x * NT) {
            const long long img = u / A.upi;
            const unsigned p0 = (unsigned)(u - img * A.upi) * V;
            const long long off = (img * A.L.P + k) * (long long)HW + p0;
            unsigned pv[V], tv[V];
            Bytes<V>::ld(A.pred + off, pv);
            Bytes<V>::ld(A.target + off, tv);
#pragma unroll
            for (int i = 0; i < V; ++i) {
                if (size == 0) {
                    const unsigned pb = pv[i] > 0, tb = tv[i] > 0;
                    n_p += pb; n_t += tb; n_i += pb & tb; n_agree += pb == tb;
                } else {
                    const unsigned pc = pv[i] >= 1 && pv[i] <= size ? pv[i] : 0;         // above the group's size: sets nothing
                    const unsigned tc = tv[i] >= 1 && tv[i] <= size ? tv[i] : 0;
                    n_agree += pc == tc;
                    if (pc) atomicAdd(&s_h[C + base + pc - 1], 1u);                       // (1 <= pc <= size: inside the group)
                    if (tc) atomicAdd(&s_h[2 * C + base + tc - 1], 1u);
                    if (pc && pc == tc) atomicAdd(&s_h[base + pc - 1], 1u);
                }
            }
        }
        if (n_agree) atomicAdd(&s_h[3 * C + k], n_agree);
        if (n_i) atomicAdd(&s_h[base], n_i);                         // (zero for a class plane)
        if (n_p) atomicAdd(&s_h[C + base], n_p);
        if (n_t) atomicAdd(&s_h[2 * C + base], n_t);
    }
    __syncthreads();
    for (unsigned i = tid; i < nh; i += NT) {
        const unsigned v = s_h[i];
        if (v) atomicAdd(A.counts + i, (unsigned long long)v);
    }
    if (blockIdx.x == 0 && tid == 0) atomicAdd(A.counts + nh, (unsigned long long)A.pixels);
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
int cls_layout(const char* what, const int* groups, int n_groups, int value_channels, const float* tau, int N, int H, int W, CLayout* L) {
    if (N <= 0 || H <= 0 || W <= 0) MAS_FAIL(MAS_EINVAL, "%s: empty shape [%d, %d, %d]", what, N, H, W);
    if (n_groups < 0 || value_channels < 0 || n_groups + value_channels < 1)
        MAS_FAIL(MAS_EINVAL, "%s: %d groups + %d value channels", what, n_groups, value_channels);
    if (n_groups + value_channels > MAXP)
        MAS_FAIL(MAS_EUNSUPPORTED, "%s: %d groups + %d value channels (1 .. %d planes)", what, n_groups, value_channels, MAXP);
    memset(L, 0, sizeof(*L));
    unsigned c = 0;
    for (int g = 0; g < n_groups; ++g) {
        if (groups[g] < 1) MAS_FAIL(MAS_EINVAL, "%s: group %d has %d classes", what, g, groups[g]);
        if (groups[g] > 255) MAS_FAIL(MAS_EUNSUPPORTED, "%s: group %d has %d classes (1 .. 255)", what, g, groups[g]);
        L->base[g] = c; L->size[g] = (unsigned)groups[g];
        c += (unsigned)groups[g];
    }
    for (int k = 0; k < value_channels; ++k) { L->base[n_groups + k] = c++; L->size[n_groups + k] = 0; }
    L->P = n_groups + value_channels;
    L->C = c;
    for (int k = 0; k < L->P; ++k) {
        L->tau[k] = tau ? tau[k] : -INFINITY;
        if (isnan(L->tau[k])) MAS_FAIL(MAS_EINVAL, "%s: the threshold of plane %d is NaN", what, k);
    }
    if ((long long)H * W > (1LL << 30)) MAS_FAIL(MAS_EUNSUPPORTED, "%s: H W = %lld > 2^30", what, (long long)H * W);
    return MAS_OK;
}

}  // namespace

extern "C" int mas_seg_classify(const void* x, int x_dtype, int x_layout, const int* groups, int n_groups, int value_channels,
                                const float* tau, int N, int H, int W, unsigned char* planes, void* stream) {
    MAS_ENTER();
    const char* what = "seg_classify";
    if (!x || !planes || !tau || (n_groups > 0 && !groups)) MAS_FAIL(MAS_EINVAL, "%s: null argument", what);
    CArgs A;
    memset(&A, 0, sizeof(A));
    if (int rc = cls_layout(what, groups, n_groups, value_channels, tau, N, H, W, &A.L)) return rc;
    if (x_dtype != MAS_F32 && x_dtype != MAS_BF16) MAS_FAIL(MAS_EUNSUPPORTED, "%s: dtype %d (fp32 / bf16)", what, x_dtype);
    if (x_layout != MAS_SEG_NCHW && x_layout != MAS_SEG_NHWC) MAS_FAIL(MAS_EINVAL, "%s: layout code %d (MAS_SEG_NCHW or MAS_SEG_NHWC)", what, x_layout);
    const long long hw = (long long)H * W;
    if ((double)N * A.L.C * (double)hw > 4e18) MAS_FAIL(MAS_EUNSUPPORTED, "%s: more than 4e18 elements", what);
    const size_t xe = mas_esize(x_dtype);
    if (reinterpret_cast<uintptr_t>(x) % xe) MAS_FAIL(MAS_EINVAL, "%s: the prediction is not aligned to its element size", what);
    A.x = x; A.planes = planes; A.HW = (unsigned)hw;
    const long long cap = (long long)mas_num_cus() * 8;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (x_layout == MAS_SEG_NHWC) {
        A.Cs = A.L.C | 1u;
        const unsigned fit = NHWC_LDS_BYTES / (A.Cs * 4u);           // (C <= 2040: at least 5)
        A.SP = fit < (unsigned)NT ? fit : (unsigned)NT;
        if (A.SP > hw) A.SP = (unsigned)hw;
        A.upi = (unsigned)((hw + A.SP - 1) / A.SP);
        A.units = (long long)N * A.upi;
        A.invC = 1.0f / (float)A.L.C;
        const dim3 grid((unsigned)(A.units < cap ? A.units : cap)), block(NT);
        const size_t lds = (size_t)A.SP * A.Cs * sizeof(float);
        if (x_dtype == MAS_BF16) hipLaunchKernelGGL((seg_classify_nhwc_kernel<bf16_t>), grid, block, lds, s, A);
        else hipLaunchKernelGGL((seg_classify_nhwc_kernel<float>), grid, block, lds, s, A);
    } else {
        const int vu = 16 / (int)xe;
        const bool vec = hw % vu == 0 && reinterpret_cast<uintptr_t>(x) % 16 == 0 && reinterpret_cast<uintptr_t>(planes) % 8 == 0;
        A.upi = (unsigned)(vec ? hw / vu : hw);
        A.units = (long long)N * A.upi;
        const long long need = (A.units + NT - 1) / NT;
        const dim3 grid((unsigned)(need < cap ? need : cap)), block(NT);
#define CLS_GO(PT) do { \
        if (vec) hipLaunchKernelGGL((seg_classify_nchw_kernel<PT, 16 / (int)sizeof(PT)>), grid, block, 0, s, A); \
        else hipLaunchKernelGGL((seg_classify_nchw_kernel<PT, 1>), grid, block, 0, s, A); } while (0)
        if (x_dtype == MAS_BF16) CLS_GO(bf16_t); else CLS_GO(float);
#undef CLS_GO
    }
    MAS_CHECK_LAUNCH(what);
    return MAS_OK;
}

extern "C" int mas_seg_agreement(const unsigned char* pred, const unsigned char* target, const int* groups, int n_groups, int value_channels,
                                 int N, int H, int W, long long* counts, void* stream) {
    MAS_ENTER();
    const char* what = "seg_agreement";
    if (!pred || !target || !counts || (n_groups > 0 && !groups)) MAS_FAIL(MAS_EINVAL, "%s: null argument", what);
    GArgs A;
    memset(&A, 0, sizeof(A));
    if (int rc = cls_layout(what, groups, n_groups, value_channels, nullptr, N, H, W, &A.L)) return rc;
    const long long hw = (long long)H * W;
    // a work-group's LDS counters and a lane's registers are 32 bits wide: with at least 4 work-groups once there are that many pixels,
    // 2^32 pixels leave every one of them below 2^30
    if ((double)N * (double)hw > 4294967296.0) MAS_FAIL(MAS_EUNSUPPORTED, "%s: N H W = %.0f > 2^32", what, (double)N * (double)hw);
    if (reinterpret_cast<uintptr_t>(counts) % 8) MAS_FAIL(MAS_EINVAL, "%s: counts is not aligned to 8 bytes", what);
    A.pred = pred; A.target = target; A.counts = reinterpret_cast<unsigned long long*>(counts); A.HW = (unsigned)hw;
    A.pixels = (long long)N * hw;
    const bool vec = hw % 4 == 0 && reinterpret_cast<uintptr_t>(pred) % 4 == 0 && reinterpret_cast<uintptr_t>(target) % 4 == 0;
    A.upi = (unsigned)(vec ? hw / 4 : hw);
    A.units = (long long)N * A.upi;
    const long long cap = (long long)mas_num_cus() * 4, need = (A.units + NT - 1) / NT;
    const dim3 grid((unsigned)(need < cap ? need : cap)), block(NT);
    const size_t lds = (size_t)(3 * A.L.C + A.L.P) * sizeof(unsigned);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (vec) hipLaunchKernelGGL((seg_agreement_kernel<4>), grid, block, lds, s, A);
    else hipLaunchKernelGGL((seg_agreement_kernel<1>), grid, block, lds, s, A);
    MAS_CHECK_LAUNCH(what);
    return MAS_OK;
}
