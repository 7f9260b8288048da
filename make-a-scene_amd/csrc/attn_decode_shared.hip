// Decode attention for candidates that share a prompt: mas_attn_decode_shared / mas_attn_decode_shared_dev (generate(num_samples=n)).
// rows = groups * group cache rows; the `group` consecutive rows r with r / group == g are candidates for ONE prompt, whose keys and
// values are stored once, prompt_k / prompt_v [groups, prompt_len, D], and each row's own cache [rows, capacity, D] holds only the image
// positions.  Query r attends to the prompt_len keys of block r / group and to its own keys 0 .. past - prompt_len (`past` counts the
// prompt, as in every decode entry).  Two launches on one stream, exchanging data only through the launch boundary:
//
//   partial  256 lanes, a 1-D grid of two kinds of work-group (the kind is uniform per work-group):
//            prompt  blocks [0, groups*H*tiles*nsplit_prompt), tiles = ceil(group / QT): one key range of one (group, head) for QT
//                    consecutive rows of the group.  Every 16-byte unit of a key / value row is loaded once and used for the QT queries
//                    (attn_decode_tile.h); range s = keys [s*chunk, min(prompt_len, (s+1)*chunk)), chunk = ceil(prompt_len /
//                    nsplit_prompt) rounded up to 32.  A tile that reaches past the group computes on the group's last row again and
//                    stores nothing for it.
//            own     the blocks after them, rows*H*nsplit_own: what attn_decode_split_partial_kernel does, on the L_own = past -
//                    prompt_len + 1 own keys (ranges: chunk = ceil(L_own / nsplit_own) rounded up to 32).  In the device-`past` form the
//                    one split that owns key L_own - 1 copies this head's units of k_new / v_new into cache row L_own - 1 and passes
//                    __syncthreads() before any of its lanes loads a key; no other work-group of the launch reads those bytes.
//            Each writes un-normalised states {o[hd], m, l} to workspace[(r*H + h)][s], s in [0, nsplit_prompt) for the prompt ranges
//            and nsplit_prompt + [0, nsplit_own) for the own ones (the neutral state m = -1e30, l = 0, o = 0 for a range without keys).
//   combine  one work-group of max(64, HD) lanes per (row, head): common maximum of the nsplit_prompt + nsplit_own states, rescale and
//            add in that order (prompt ranges first), divide, write the context row in the cache dtype.
//
// Fixed orders throughout: the same inputs give the same bits, and a row's bits depend on its query, its prompt block and its own cache
// only -- not on its place in the tile (every query slot runs the same instructions) nor on the other groups.  The host-`past` and the
// device-`past` entries are the SAME kernels and agree bit for bit.  Device guard: *past < prompt_len or *past - prompt_len >= capacity
// makes every work-group of both launches return at once: nothing read or written.
#include "attn_decode_tile.h"
#include <limits.h>

namespace {

// queries per prompt tile: 4 builds at 124-126 VGPRs in bf16 (4 waves per SIMD), 8 at 203-206 (2 waves per SIMD); neither uses scratch
// (profiles/shared_prompt_resources.txt has both builds)
constexpr int QT = MAS_ATTN_DECODE_SHARED_QT;

struct SharedParams {
    const void* q; const void* kn; const void* vn;   // kn / vn: the row to append (device-past form) or null
    const void* pk; const void* pv;                  // prompt blocks
    const void* kc; const void* vc; void* o; float* ws;
    long long q_bs, new_bs, p_bs, c_bs, o_bs;        // row / block strides (elements)
    int ld_p, ld_c;                                  // token strides (elements)
    int rows, group, H, plen, cap, nsp, nso, past, tiles;
    unsigned prompt_blocks;
    const int* past_dev;                             // null: `past` above
    float scale;
};

template <typename T, int HD>
__global__ __launch_bounds__(DECODE_NT) void attn_decode_shared_partial_kernel(SharedParams p) {
    constexpr int EPU = 16 / (int)sizeof(T);
    constexpr int G = HD / EPU;
    const int past = p.past_dev ? *p.past_dev : p.past;
    if (past < p.plen || past - p.plen >= p.cap) return;         // misuse guard (uniform over the grid): nothing read or written
    __shared__ float red[decode_tile_lds_floats<HD, QT>()];
    const int tid = threadIdx.x;
    const int nst = p.nsp + p.nso;
    if (blockIdx.x < p.prompt_blocks) {
        unsigned id = blockIdx.x;
        const int split = id % p.nsp; id /= p.nsp;
        const int tile = id % p.tiles; id /= p.tiles;
        const int g = id / p.H, h = id % p.H;
        int begin, end;
        decode_tile_range(p.plen, p.nsp, split, begin, end);
        const T* Q[QT];
        float* dst[QT];
#pragma unroll
        for (int i = 0; i < QT; ++i) {
            const int j = tile * QT + i;
            const size_t r = (size_t)g * p.group + min(j, p.group - 1);
            Q[i] = reinterpret_cast<const T*>(p.q) + r * p.q_bs + (size_t)h * HD;
            dst[i] = j < p.group ? p.ws + ((r * p.H + h) * nst + split) * (HD + 2) : nullptr;
        }
        const T* K = reinterpret_cast<const T*>(p.pk) + (size_t)g * p.p_bs + (size_t)h * HD;
        const T* V = reinterpret_cast<const T*>(p.pv) + (size_t)g * p.p_bs + (size_t)h * HD;
        decode_tile_partial<T, HD, QT>(Q, K, V, p.ld_p, p.ld_p, begin, end, p.scale, dst, red);
        return;
    }
    unsigned id = blockIdx.x - p.prompt_blocks;
    const int split = id % p.nso; id /= p.nso;
    const size_t b = id / p.H;
    const int h = id % p.H;
    const int last = past - p.plen;              // the own key the new row is
    int begin, end;
    decode_tile_range(last + 1, p.nso, split, begin, end);
    T* kc = reinterpret_cast<T*>(const_cast<void*>(p.kc)) + b * p.c_bs + (size_t)h * HD;
    T* vc = reinterpret_cast<T*>(const_cast<void*>(p.vc)) + b * p.c_bs + (size_t)h * HD;
    if (p.kn) {                                  // device-past form: the split that owns key `last` appends it
        if (last >= begin && last < end && tid < 2 * G) {
            const bool isv = tid >= G;
            const int uu = isv ? tid - G : tid;
            const T* src = reinterpret_cast<const T*>(isv ? p.vn : p.kn) + b * p.new_bs + (size_t)h * HD + uu * EPU;
            T* dstc = (isv ? vc : kc) + (size_t)last * p.ld_c + uu * EPU;
            *reinterpret_cast<u32x4*>(dstc) = *reinterpret_cast<const u32x4*>(src);
        }
        __syncthreads();
    }
    const T* Q[1] = {reinterpret_cast<const T*>(p.q) + b * p.q_bs + (size_t)h * HD};
    float* dst[1] = {p.ws + ((b * p.H + h) * nst + p.nsp + split) * (HD + 2)};
    decode_tile_partial<T, HD, 1>(Q, kc, vc, p.ld_c, p.ld_c, begin, end, p.scale, dst, red);
}

template <typename T, int HD>
__global__ __launch_bounds__(HD < 64 ? 64 : HD) void attn_decode_shared_combine_kernel(SharedParams p) {
    const int past = p.past_dev ? *p.past_dev : p.past;
    if (past < p.plen || past - p.plen >= p.cap) return;
    const size_t bh = blockIdx.x, b = bh / p.H;
    const int h = (int)(bh % p.H);
    const int nst = p.nsp + p.nso;
    const int d = threadIdx.x < HD ? threadIdx.x : 0;            // HD < 64: the spare lanes shadow lane 0 and store nothing
    const float* __restrict__ ws = p.ws + bh * nst * (HD + 2);
    // lane s of every wave fetches {m, l} of state s (nst <= 64): one round trip instead of one per state (the serial loop of the first
    // build cost 0.36 us per state: profiles/shared_prompt_sample_bench.txt); the maximum is a butterfly, the sums below still run in
    // state order, four loads of o in flight at a time (a state past nst adds f = 0, l * f = 0: the bits of the plain loop)
    const int lane = threadIdx.x & 63;
    float ms = -1e30f, ls = 0.0f;
    if (lane < nst) {
        ms = ws[lane * (HD + 2) + HD]; ls = ws[lane * (HD + 2) + HD + 1];
    }
    float mt = ms;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mt = fmaxf(mt, __shfl_xor(mt, off));
    const float fs = __expf(ms - mt);                             // an empty range, and a lane past nst: 0 (prompt range 0 never is empty)
    const float lf = ls * fs;
    float lt = 0.0f, acc = 0.0f;
    for (int s0 = 0; s0 < nst; s0 += 4) {                         // prompt ranges, then own ranges; s0 + 3 <= 63
        float x[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = s0 + j < nst ? ws[(s0 + j) * (HD + 2) + d] : 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            lt += __shfl(lf, s0 + j);
            acc = fmaf(x[j], __shfl(fs, s0 + j), acc);
        }
    }
    if (threadIdx.x < HD) {
        T* dst = reinterpret_cast<T*>(p.o) + b * p.o_bs + (size_t)h * HD;
        dst[d] = (T)(acc * (1.0f / lt));
    }
}

template <typename T, int HD>
void launch_pair(const SharedParams& p, unsigned blocks, hipStream_t s) {
    hipLaunchKernelGGL((attn_decode_shared_partial_kernel<T, HD>), dim3(blocks), dim3(DECODE_NT), 0, s, p);
    hipLaunchKernelGGL((attn_decode_shared_combine_kernel<T, HD>), dim3((unsigned)(p.rows * p.H)), dim3(HD < 64 ? 64 : HD), 0, s, p);
}

// everything both entries share: checks the arguments, fills the derived fields of p, launches
int run_shared(const char* name, SharedParams& p, int dtype, int hd, size_t ws_floats, const void* const* aligned, int n_aligned,
               void* stream) {
    if (p.rows <= 0 || p.H <= 0 || hd <= 0) MAS_FAIL(MAS_EINVAL, "%s: bad shape rows=%d H=%d hd=%d", name, p.rows, p.H, hd);
    if (p.group < 1) MAS_FAIL(MAS_EINVAL, "%s: group %d < 1", name, p.group);
    if (p.rows % p.group) MAS_FAIL(MAS_EINVAL, "%s: rows %d is not a multiple of group %d", name, p.rows, p.group);
    if (p.plen < 1) MAS_FAIL(MAS_EINVAL, "%s: prompt_len %d < 1", name, p.plen);
    if (p.nsp < 1 || p.nsp > MAS_ATTN_DECODE_MAX_SPLITS)
        MAS_FAIL(MAS_EINVAL, "%s: nsplit_prompt %d outside [1, %d]", name, p.nsp, MAS_ATTN_DECODE_MAX_SPLITS);
    if (p.nso < 1 || p.nso > MAS_ATTN_DECODE_MAX_SPLITS)
        MAS_FAIL(MAS_EINVAL, "%s: nsplit_own %d outside [1, %d]", name, p.nso, MAS_ATTN_DECODE_MAX_SPLITS);
    if (p.cap <= 0 || p.ld_c < (long long)p.H * hd || p.c_bs < (long long)p.cap * p.ld_c || p.ld_p < (long long)p.H * hd ||
        p.p_bs < (long long)p.plen * p.ld_p)
        MAS_FAIL(MAS_EINVAL, "%s: bad layout H=%d hd=%d capacity=%d ld_c=%d prompt_len=%d ld_p=%d", name, p.H, hd, p.cap, p.ld_c, p.plen,
                 p.ld_p);
    p.tiles = (p.group + QT - 1) / QT;
    const long long prompt_blocks = (long long)(p.rows / p.group) * p.H * p.tiles * p.nsp;
    const long long blocks = prompt_blocks + (long long)p.rows * p.H * p.nso;
    if (blocks > INT_MAX) MAS_FAIL(MAS_EINVAL, "%s: %lld work-groups: rows=%d H=%d is beyond one launch", name, blocks, p.rows, p.H);
    p.prompt_blocks = (unsigned)prompt_blocks;
    if (!p.ws) MAS_FAIL(MAS_EINVAL, "%s: null workspace", name);
    const size_t need = (size_t)p.rows * p.H * (p.nsp + p.nso) * (hd + 2);
    if (ws_floats < need) MAS_FAIL(MAS_EWORKSPACE, "%s: workspace too small: %zu floats, %zu needed", name, ws_floats, need);
    if (reinterpret_cast<uintptr_t>(p.ws) & 3) MAS_FAIL(MAS_EUNSUPPORTED, "%s: workspace must be 4-byte aligned", name);
    if (dtype != MAS_BF16 && dtype != MAS_F32) MAS_FAIL(MAS_EUNSUPPORTED, "%s: dtype %d", name, dtype);
    const int epu = 16 / (int)mas_esize(dtype);
    uintptr_t bits = 0;
    for (int i = 0; i < n_aligned; ++i) bits |= reinterpret_cast<uintptr_t>(aligned[i]);
    if ((p.ld_c % epu) || (p.ld_p % epu) || (p.q_bs % epu) || (p.new_bs % epu) || (p.c_bs % epu) || (p.p_bs % epu) || (bits & 15))
        MAS_FAIL(MAS_EUNSUPPORTED, "%s: q / k / v rows must be 16-byte aligned", name);
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const bool ok = decode_dispatch_hd(hd, [&](auto hd_c) {
        if (dtype == MAS_BF16) launch_pair<bf16_t, decltype(hd_c)::value>(p, (unsigned)blocks, s);
        else launch_pair<float, decltype(hd_c)::value>(p, (unsigned)blocks, s);
    });
    if (!ok) MAS_FAIL(MAS_EUNSUPPORTED, "%s: head_dim %d not in {16,32,64,128}", name, hd);
    MAS_CHECK_LAUNCH(name);
    return MAS_OK;
}

}  // namespace

extern "C" int mas_attn_decode_shared(const void* q, long long q_bs, const void* prompt_k, const void* prompt_v, int ld_p, long long p_bs,
                                      int prompt_len, const void* k_cache, const void* v_cache, int ld_c, long long c_bs, int capacity,
                                      void* o, long long o_bs, int dtype, int rows, int group, int H, int hd, int past, float scale,
                                      int nsplit_prompt, int nsplit_own, float* workspace, size_t workspace_floats, void* stream) {
    MAS_ENTER();
    if (!q || !prompt_k || !prompt_v || !k_cache || !v_cache || !o) MAS_FAIL(MAS_EINVAL, "attn_decode_shared: null argument");
    if (prompt_len >= 1 && (past < prompt_len || (capacity > 0 && past - prompt_len >= capacity)))
        MAS_FAIL(MAS_EINVAL, "attn_decode_shared: past %d outside [prompt_len, prompt_len + capacity) = [%d, %lld)", past, prompt_len,
                 (long long)prompt_len + capacity);
    SharedParams p;
    p.q = q; p.kn = nullptr; p.vn = nullptr; p.pk = prompt_k; p.pv = prompt_v; p.kc = k_cache; p.vc = v_cache; p.o = o; p.ws = workspace;
    p.q_bs = q_bs; p.new_bs = 0; p.p_bs = p_bs; p.c_bs = c_bs; p.o_bs = o_bs; p.ld_p = ld_p; p.ld_c = ld_c;
    p.rows = rows; p.group = group; p.H = H; p.plen = prompt_len; p.cap = capacity; p.nsp = nsplit_prompt; p.nso = nsplit_own;
    p.past = past; p.past_dev = nullptr; p.scale = scale;
    const void* aligned[] = {q, prompt_k, prompt_v, k_cache, v_cache};
    return run_shared("attn_decode_shared", p, dtype, hd, workspace_floats, aligned, 5, stream);
}

extern "C" int mas_attn_decode_shared_dev(const void* q, const void* k_new, const void* v_new, long long new_bs, const void* prompt_k,
                                          const void* prompt_v, int ld_p, long long p_bs, int prompt_len, void* k_cache, void* v_cache,
                                          int ld_c, long long c_bs, int capacity, void* o, long long o_bs, int dtype, int rows, int group,
                                          int H, int hd, const int32_t* past, float scale, int nsplit_prompt, int nsplit_own,
                                          float* workspace, size_t workspace_floats, void* stream) {
    MAS_ENTER();
    if (!q || !k_new || !v_new || !prompt_k || !prompt_v || !k_cache || !v_cache || !o || !past)
        MAS_FAIL(MAS_EINVAL, "attn_decode_shared_dev: null argument");
    SharedParams p;
    p.q = q; p.kn = k_new; p.vn = v_new; p.pk = prompt_k; p.pv = prompt_v; p.kc = k_cache; p.vc = v_cache; p.o = o; p.ws = workspace;
    p.q_bs = new_bs; p.new_bs = new_bs; p.p_bs = p_bs; p.c_bs = c_bs; p.o_bs = o_bs; p.ld_p = ld_p; p.ld_c = ld_c;
    p.rows = rows; p.group = group; p.H = H; p.plen = prompt_len; p.cap = capacity; p.nsp = nsplit_prompt; p.nso = nsplit_own;
    p.past = 0; p.past_dev = past; p.scale = scale;
    const void* aligned[] = {q, k_new, v_new, prompt_k, prompt_v, k_cache, v_cache};
    return run_shared("attn_decode_shared_dev", p, dtype, hd, workspace_floats, aligned, 7, stream);
}
