// Decode attention split over keys ("flash-decoding") for low batch * heads: mas_attn_decode_split / mas_attn_decode_split_dev.
// attn_decode_kernel (attn_decode.hip) and attn_decode_dev_kernel (decode_step.hip) run one work-group per (row, head): at B = 1 with
// guidance and 16 heads that is 32 work-groups on 256 CUs, each walking up to 1535 cached rows -- serial latency, not bandwidth.  Here
// nsplit work-groups share the keys of one (row, head), in two launches that exchange data only through the launch boundary:
//
//   partial  grid (nsplit, rows*H), 256 lanes.  With L = past + 1 visible keys, split s owns keys [s*chunk, min(L, (s+1)*chunk)),
//            chunk = ceil(L / nsplit) rounded up to GRAN = 32 keys -- computed in the kernel, so it follows a `past` that lives in
//            device memory and every split has work at every token.  The HD-element row of a key is spread over G = HD*sizeof(T)/16
//            lanes, 16 bytes each (a wave's load covers 64/G whole rows: contiguous 16*G-byte segments), the dot product is finished by
//            log2(G) butterfly shuffles, and a lane keeps the online-softmax state (m, l) of its key slot and the 16/sizeof(T)
//            elements of o it owns.  Four keys per slot are loaded before the first is used.  The 256/G slots are merged as
//            attn_decode_kernel merges its lanes (common maximum, rescale, butterfly sums, then the 4 waves through LDS, all in a fixed
//            order) and the un-normalised state goes to workspace[(row*H + h)][s] = {o[HD], m, l} (fp32).  A split without keys
//            writes the neutral state m = -1e30, l = 0, o = 0.
//   combine  one work-group of max(64, HD) lanes per (row, head): common maximum of the nsplit states, rescale and add in split order,
//            divide by the sum, write the context row in the cache dtype.  Fixed order: the result repeats bit for bit.
//
// `past` is a host integer (the caller has appended the new row: mas_attn_decode's contract) or a device int32 with the new k / v row
// to append (mas_attn_decode_dev's contract).  Both forms are the SAME two kernels -- the device form only differs in where `past` is
// read and in the append below -- so they agree bit for bit.  The append: key `past` = L - 1 belongs to exactly one split of each
// (row, head), the last one with keys; that work-group, and no other, copies this head's 16-byte units of k_new / v_new into cache row
// `past` (lanes 0 .. 2G-1) and then passes __syncthreads() -- workgroup-scope release, barrier, acquire -- before any of its lanes loads
// a key, so the row is read back from the cache like every other key.  No other work-group of the launch loads those bytes: the other
// splits of the head stop before key `past`, the other heads read other columns.  When *past is outside [0, capacity) both kernels
// return at once: nothing is read or written, the workspace and o included.
#include "attn_decode_core.h"
#include <limits.h>
#include <math.h>

namespace {

constexpr int SNT = 256;     // lanes of the partial kernel
constexpr int GRAN = 32;     // a split's key range is a multiple of this
constexpr int KU = 4;        // keys in flight per slot

struct SplitParams {
    const void* q; const void* kn; const void* vn;   // kn / vn: the row to append (device-past form) or null
    const void* kc; const void* vc; void* o; float* ws;
    long long q_bs, new_bs, k_bs, v_bs, o_bs;        // batch strides (elements)
    int ld_k, ld_v;                                  // cache token strides (elements)
    int B, H, cap, nsplit, past;
    const int* past_dev;                             // null: `past` above
    float scale;
};

template <typename T, int HD>
__global__ __launch_bounds__(SNT) void attn_decode_split_partial_kernel(SplitParams p) {
    constexpr int EPU = 16 / (int)sizeof(T);     // elements of a 16-byte unit
    constexpr int G = HD / EPU;                  // lanes per key row (2 .. 32)
    constexpr int KPP = SNT / G;                 // key slots of the work-group
    const int past = p.past_dev ? *p.past_dev : p.past;
    if (past < 0 || past >= p.cap) return;       // misuse guard (uniform over the grid): nothing read or written
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int u = tid % G, slot = tid / G;
    const int split = blockIdx.x, bh = blockIdx.y, b = bh / p.H, h = bh % p.H;
    const int L = past + 1;                      // keys visible to the query: 0 .. past
    const int chunk = ((L + p.nsplit - 1) / p.nsplit + GRAN - 1) / GRAN * GRAN;
    const int begin = split * chunk;
    const int end = min(L, begin + chunk);

    T* kc = reinterpret_cast<T*>(const_cast<void*>(p.kc)) + (size_t)b * p.k_bs + (size_t)h * HD;
    T* vc = reinterpret_cast<T*>(const_cast<void*>(p.vc)) + (size_t)b * p.v_bs + (size_t)h * HD;
    if (p.kn) {                                  // device-past form: the split that owns key `past` appends it
        if (past >= begin && past < end && tid < 2 * G) {
            const bool isv = tid >= G;
            const int uu = isv ? tid - G : tid;
            const T* src = reinterpret_cast<const T*>(isv ? p.vn : p.kn) + (size_t)b * p.new_bs + (size_t)h * HD + uu * EPU;
            T* dstc = (isv ? vc + (size_t)past * p.ld_v : kc + (size_t)past * p.ld_k) + uu * EPU;
            *reinterpret_cast<u32x4*>(dstc) = *reinterpret_cast<const u32x4*>(src);
        }
        __syncthreads();
    }

    const T* __restrict__ Q = reinterpret_cast<const T*>(p.q) + (size_t)b * p.q_bs + (size_t)h * HD + u * EPU;
    const T* __restrict__ K = kc + u * EPU;
    const T* __restrict__ V = vc + u * EPU;

    float qf[EPU];                               // this lane's unit of the query, pre-scaled (transformer.py:56: q / sqrt(hd))
    {
        const u32x4 raw = *reinterpret_cast<const u32x4*>(Q);
        const T* e = reinterpret_cast<const T*>(&raw);
#pragma unroll
        for (int j = 0; j < EPU; ++j) qf[j] = (float)e[j] * p.scale;
    }

    float m = -1e30f, l = 0.0f, o[EPU];
#pragma unroll
    for (int j = 0; j < EPU; ++j) o[j] = 0.0f;

    for (int base = begin; base < end; base += KPP * KU) {      // uniform over the work-group: the shuffles below see every lane
        u32x4 kraw[KU], vraw[KU];
#pragma unroll
        for (int i = 0; i < KU; ++i) {
            const int key = base + i * KPP + slot;
            kraw[i] = u32x4{0u, 0u, 0u, 0u};
            vraw[i] = u32x4{0u, 0u, 0u, 0u};
            if (key < end) {                     // rows from `end` on are never loaded
                kraw[i] = *reinterpret_cast<const u32x4*>(K + (size_t)key * p.ld_k);
                vraw[i] = *reinterpret_cast<const u32x4*>(V + (size_t)key * p.ld_v);
            }
        }
#pragma unroll
        for (int i = 0; i < KU; ++i) {
            const int key = base + i * KPP + slot;
            const T* ke = reinterpret_cast<const T*>(&kraw[i]);
            float s = 0.0f;
#pragma unroll
            for (int j = 0; j < EPU; ++j) s += qf[j] * (float)ke[j];
#pragma unroll
            for (int off = G / 2; off >= 1; off >>= 1) s += __shfl_xor(s, off);   // the G lanes of the row: the same sum in each
            if (key < end) {
                const T* ve = reinterpret_cast<const T*>(&vraw[i]);
                const float m_new = fmaxf(m, s);
                const float a = __expf(m - m_new), pv = __expf(s - m_new);
                l = l * a + pv;
                m = m_new;
#pragma unroll
                for (int j = 0; j < EPU; ++j) o[j] = o[j] * a + pv * (float)ve[j];
            }
        }
    }

    // ---- merge the 64 / G slots of a wave: common maximum, rescale, butterfly sums (fixed order: deterministic) ----
    float mw = m;
#pragma unroll
    for (int off = 32; off >= G; off >>= 1) mw = fmaxf(mw, __shfl_xor(mw, off));
    const float f = __expf(m - mw);              // slots without a key: m = -1e30 -> f = 0 (or 1 when the whole wave is empty: l = o = 0)
    l *= f;
#pragma unroll
    for (int off = 32; off >= G; off >>= 1) l += __shfl_xor(l, off);
#pragma unroll
    for (int j = 0; j < EPU; ++j) {
        float x = o[j] * f;
#pragma unroll
        for (int off = 32; off >= G; off >>= 1) x += __shfl_xor(x, off);
        o[j] = x;
    }
    // ---- merge the 4 waves through LDS, write the split's state ----
    __shared__ float red[4][HD + 2];
    if (lane == 0) {
        red[wave][HD] = mw; red[wave][HD + 1] = l;
    }
    if (lane < G) {
#pragma unroll
        for (int j = 0; j < EPU; ++j) red[wave][lane * EPU + j] = o[j];
    }
    __syncthreads();
    if (tid < HD + 2) {
        const float m0 = red[0][HD], m1 = red[1][HD], m2 = red[2][HD], m3 = red[3][HD];
        const float mt = fmaxf(fmaxf(m0, m1), fmaxf(m2, m3));
        const float f0 = __expf(m0 - mt), f1 = __expf(m1 - mt), f2 = __expf(m2 - mt), f3 = __expf(m3 - mt);
        float* dst = p.ws + ((size_t)bh * p.nsplit + split) * (HD + 2);
        dst[tid] = tid == HD ? mt : red[0][tid] * f0 + red[1][tid] * f1 + red[2][tid] * f2 + red[3][tid] * f3;   // o[d] and, at HD + 1, l
    }
}

template <typename T, int HD>
__global__ __launch_bounds__(HD < 64 ? 64 : HD) void attn_decode_split_combine_kernel(SplitParams p) {
    const int past = p.past_dev ? *p.past_dev : p.past;
    if (past < 0 || past >= p.cap) return;
    const int bh = blockIdx.x, b = bh / p.H, h = bh % p.H;
    const int d = threadIdx.x < HD ? threadIdx.x : 0;            // HD < 64: the spare lanes shadow lane 0 and store nothing
    const float* __restrict__ ws = p.ws + (size_t)bh * p.nsplit * (HD + 2);
    float mt = -1e30f;
    for (int s = 0; s < p.nsplit; ++s) mt = fmaxf(mt, ws[s * (HD + 2) + HD]);
    float lt = 0.0f, acc = 0.0f;
    for (int s = 0; s < p.nsplit; ++s) {                          // split order; an empty split has f = 0 (split 0 never is: lt > 0)
        const float* st = ws + s * (HD + 2);
        const float f = __expf(st[HD] - mt);
        lt += st[HD + 1] * f;
        acc += st[d] * f;
    }
    if (threadIdx.x < HD) {
        T* dst = reinterpret_cast<T*>(p.o) + (size_t)b * p.o_bs + (size_t)h * HD;
        dst[d] = (T)(acc * (1.0f / lt));
    }
}

template <typename T, int HD>
void launch_pair(const SplitParams& p, hipStream_t s) {
    hipLaunchKernelGGL((attn_decode_split_partial_kernel<T, HD>), dim3((unsigned)p.nsplit, (unsigned)(p.B * p.H)), dim3(SNT), 0, s, p);
    hipLaunchKernelGGL((attn_decode_split_combine_kernel<T, HD>), dim3((unsigned)(p.B * p.H)), dim3(HD < 64 ? 64 : HD), 0, s, p);
}

template <typename T>
int launch_split(const SplitParams& p, int hd, hipStream_t s, const char* name) {
    if (!decode_dispatch_hd(hd, [&](auto hd_c) { launch_pair<T, decltype(hd_c)::value>(p, s); }))
        MAS_FAIL(MAS_EUNSUPPORTED, "%s: head_dim %d not in {16,32,64,128}", name, hd);
    MAS_CHECK_LAUNCH(name);
    return MAS_OK;
}

// the arguments both entries share: split count and workspace
int check_split(const char* name, int B, int H, int hd, int nsplit, const float* ws, size_t ws_floats) {
    if (nsplit < 1 || nsplit > MAS_ATTN_DECODE_MAX_SPLITS)
        MAS_FAIL(MAS_EINVAL, "%s: nsplit %d outside [1, %d]", name, nsplit, MAS_ATTN_DECODE_MAX_SPLITS);
    if (B <= 0 || H <= 0 || hd <= 0 || (long long)B * H > 65535) MAS_FAIL(MAS_EINVAL, "%s: bad shape B=%d H=%d hd=%d", name, B, H, hd);
    if (!ws) MAS_FAIL(MAS_EINVAL, "%s: null workspace", name);
    const size_t need = (size_t)B * H * nsplit * (hd + 2);
    if (ws_floats < need) MAS_FAIL(MAS_EWORKSPACE, "%s: workspace too small: %zu floats, %zu needed", name, ws_floats, need);
    if (reinterpret_cast<uintptr_t>(ws) & 3) MAS_FAIL(MAS_EUNSUPPORTED, "%s: workspace must be 4-byte aligned", name);
    return MAS_OK;
}

}  // namespace

extern "C" int mas_attn_decode_split(const void* q, const void* k_cache, const void* v_cache, void* o, int dtype, int B, int H, int nq,
                                     int past, int hd, int ld_q, int ld_k, int ld_v, int ld_o, long long q_bs, long long k_bs,
                                     long long v_bs, long long o_bs, float scale, int nsplit, float* workspace, size_t workspace_floats,
                                     void* stream) {
    MAS_ENTER();
    if (!q || !k_cache || !v_cache || !o) MAS_FAIL(MAS_EINVAL, "attn_decode_split: null argument");
    if (nq != 1) MAS_FAIL(MAS_EINVAL, "attn_decode_split: nq = %d, the split form takes one query row (nq = 1)", nq);
    if (past < 0 || past == INT_MAX) MAS_FAIL(MAS_EINVAL, "attn_decode_split: bad past=%d", past);
    if (const int rc = check_split("attn_decode_split", B, H, hd, nsplit, workspace, workspace_floats)) return rc;
    const size_t esz = mas_esize(dtype);
    const int epu = 16 / (int)esz;
    if ((ld_q % epu) || (ld_k % epu) || (ld_v % epu) || (q_bs % epu) || (k_bs % epu) || (v_bs % epu) ||
        ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k_cache) | reinterpret_cast<uintptr_t>(v_cache)) & 15))
        MAS_FAIL(MAS_EUNSUPPORTED, "attn_decode_split: q / k / v rows must be 16-byte aligned");
    SplitParams p;
    p.q = q; p.kn = nullptr; p.vn = nullptr; p.kc = k_cache; p.vc = v_cache; p.o = o; p.ws = workspace;
    p.q_bs = q_bs; p.new_bs = 0; p.k_bs = k_bs; p.v_bs = v_bs; p.o_bs = o_bs; p.ld_k = ld_k; p.ld_v = ld_v;
    p.B = B; p.H = H; p.cap = INT_MAX; p.nsplit = nsplit; p.past = past; p.past_dev = nullptr; p.scale = scale;
    (void)ld_o;                                   // nq = 1: one output row per batch element
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == MAS_BF16) return launch_split<bf16_t>(p, hd, s, "attn_decode_split");
    if (dtype == MAS_F32) return launch_split<float>(p, hd, s, "attn_decode_split");
    MAS_FAIL(MAS_EUNSUPPORTED, "attn_decode_split: dtype %d", dtype);
}

extern "C" int mas_attn_decode_split_dev(const void* q, const void* k_new, const void* v_new, long long new_bs, void* k_cache,
                                         void* v_cache, int ld_c, long long c_bs, int capacity, void* o, long long o_bs, int dtype, int B,
                                         int H, int hd, const int32_t* past, float scale, int nsplit, float* workspace,
                                         size_t workspace_floats, void* stream) {
    MAS_ENTER();
    if (!q || !k_new || !v_new || !k_cache || !v_cache || !o || !past) MAS_FAIL(MAS_EINVAL, "attn_decode_split_dev: null argument");
    if (const int rc = check_split("attn_decode_split_dev", B, H, hd, nsplit, workspace, workspace_floats)) return rc;
    if (capacity <= 0 || ld_c < H * hd || c_bs < (long long)capacity * ld_c)
        MAS_FAIL(MAS_EINVAL, "attn_decode_split_dev: bad shape B=%d H=%d hd=%d capacity=%d ld=%d", B, H, hd, capacity, ld_c);
    const size_t esz = mas_esize(dtype);
    const int epu = 16 / (int)esz;
    if ((ld_c % epu) || (new_bs % epu) || (c_bs % epu) ||
        ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k_new) | reinterpret_cast<uintptr_t>(v_new) |
          reinterpret_cast<uintptr_t>(k_cache) | reinterpret_cast<uintptr_t>(v_cache)) & 15))
        MAS_FAIL(MAS_EUNSUPPORTED, "attn_decode_split_dev: q / k / v rows must be 16-byte aligned");
    SplitParams p;
    p.q = q; p.kn = k_new; p.vn = v_new; p.kc = k_cache; p.vc = v_cache; p.o = o; p.ws = workspace;
    p.q_bs = new_bs; p.new_bs = new_bs; p.k_bs = c_bs; p.v_bs = c_bs; p.o_bs = o_bs; p.ld_k = ld_c; p.ld_v = ld_c;
    p.B = B; p.H = H; p.cap = capacity; p.nsplit = nsplit; p.past = 0; p.past_dev = past; p.scale = scale;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == MAS_BF16) return launch_split<bf16_t>(p, hd, s, "attn_decode_split_dev");
    if (dtype == MAS_F32) return launch_split<float>(p, hd, s, "attn_decode_split_dev");
    MAS_FAIL(MAS_EUNSUPPORTED, "attn_decode_split_dev: dtype %d", dtype);
}
