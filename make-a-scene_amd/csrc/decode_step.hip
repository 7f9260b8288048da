// The device side of one captured decode step (MakeAScene.generate(graph=True), models/decode_graph.py): every per-token quantity
// -- the step k, the cache length, the sampling temperature and guidance scale, the RNG seed -- is read from device memory, so one
// captured graph serves every token of every call.  Three kernels and a counter bump:
//   attn_decode_dev_kernel  mas_attn_decode with nq = 1 whose cache length is a device int32 and which appends the new key / value
//                           row itself;
//   decode_embed_kernel     image-token embedding + row / column position embedding of the token sampled at the previous step;
//   sample_kernel           guidance mix, logits write-out, teacher forcing / greedy argmax / top-k + top-p + Gumbel-max draw (Philox),
//                           with an image prompt (mas_sample_tokens_prompt) the given token at the positions a per-row mask keeps;
//   advance_kernel          one thread: the step counters + 1, after every other kernel of the step has read them (stream order).
#include "attn_decode_core.h"
#include "mas_philox.h"
#include <math.h>

namespace {

// ------------------------------------------------------------------------------------------------------------------------------
// decode attention, device-resident length.  The key-to-lane assignment, the per-lane online softmax and the merge order are those
// of attn_decode_kernel (attn_decode.hip) with nq = 1, so the output is bit for bit that of mas_attn_decode on a cache whose row
// `past` was appended beforehand.  The append comes first: lanes 0 .. NU-1 copy the 16-byte units of this (b, h) slice of k_new /
// v_new into cache row `past`, then __syncthreads() -- a workgroup-scope release fence (the stores are complete), the barrier, and an
// acquire fence -- orders those stores before every lane's loads, so the lane that owns key `past` (tid == past % 256) reads the row
// back from the cache like any other key.  Everything after the barrier is the SAME FUNCTION attn_decode_kernel calls (attn_decode_body,
// attn_decode_core.h), not a copy of it (a variant with a register hand-off inside the key loop contracted the dot products
// differently: not bit for bit).
// ------------------------------------------------------------------------------------------------------------------------------
struct DecodeDevParams {
    const void* q; const void* kn; const void* vn;   // the new row's q / k / v (slices of the qkv projection)
    void* kc; void* vc; void* o;
    long long new_bs, c_bs, o_bs;                    // batch strides (elements)
    int ld_c;                                        // cache token stride (elements)
    int B, H, cap;
    const int* past;
    float scale;
};

template <typename T, int HD>
__global__ __launch_bounds__(DECODE_NT) void attn_decode_dev_kernel(DecodeDevParams p) {
    constexpr int EPU = 16 / (int)sizeof(T);
    constexpr int NU = HD / EPU;                 // 16-byte units per row
    const int past = *p.past;
    if (past < 0 || past >= p.cap) return;       // misuse guard (uniform over the grid): nothing read or written past the cache
    const int tid = threadIdx.x;
    const int bh = blockIdx.x, b = bh / p.H, h = bh % p.H;

    if (tid < 2 * NU) {                          // append: unit tid % NU of k (tid < NU) or v
        const bool isv = tid >= NU;
        const int u = isv ? tid - NU : tid;
        const T* src = reinterpret_cast<const T*>(isv ? p.vn : p.kn) + (size_t)b * p.new_bs + (size_t)h * HD + u * EPU;
        T* dstc = reinterpret_cast<T*>(isv ? p.vc : p.kc) + (size_t)b * p.c_bs + (size_t)past * p.ld_c + (size_t)h * HD + u * EPU;
        *reinterpret_cast<u32x4*>(dstc) = *reinterpret_cast<const u32x4*>(src);
    }
    __syncthreads();

    const T* Q = reinterpret_cast<const T*>(p.q) + (size_t)b * p.new_bs + (size_t)h * HD;
    const T* K = reinterpret_cast<const T*>(p.kc) + (size_t)b * p.c_bs + (size_t)h * HD;
    const T* V = reinterpret_cast<const T*>(p.vc) + (size_t)b * p.c_bs + (size_t)h * HD;
    T* dst = reinterpret_cast<T*>(p.o) + (size_t)b * p.o_bs + (size_t)h * HD;
    attn_decode_body<T, HD>(Q, K, V, dst, p.ld_c, p.ld_c, past + 1, p.scale);   // keys visible to the query: 0 .. past
}

template <typename T>
int launch_decode_dev(const DecodeDevParams& p, int hd, hipStream_t s) {
    const dim3 grid((unsigned)(p.B * p.H));
    if (!decode_dispatch_hd(hd, [&](auto hd_c) {
            hipLaunchKernelGGL((attn_decode_dev_kernel<T, decltype(hd_c)::value>), grid, dim3(DECODE_NT), 0, s, p);
        }))
        MAS_FAIL(MAS_EUNSUPPORTED, "attn_decode_dev: head_dim %d not in {16,32,64,128}", hd);
    MAS_CHECK_LAUNCH("attn_decode_dev");
    return MAS_OK;
}

// ------------------------------------------------------------------------------------------------------------------------------
// out[r] = img_emb[tok] + (row_emb[i / n] + col_emb[i % n]), tok = tokens[r % B][i], i = step - 1: the eager
// ``image_token_embedding(t) + get_image_pos_embeddings(t, past_length=i)`` in its addition order, fp32.
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int ENT = 256;

__global__ __launch_bounds__(ENT) void decode_embed_kernel(const long long* __restrict__ tokens, long long ld_tok, const int* step,
                                                           const float* __restrict__ img, int vocab, const float* __restrict__ row_e,
                                                           const float* __restrict__ col_e, int n, float* __restrict__ out, int B, int D) {
    const int r = blockIdx.x;
    const int i = *step - 1;
    float* dst = out + (size_t)r * D;
    const long long t = (i >= 0 && i < n * n) ? tokens[(size_t)(r % B) * ld_tok + i] : -1;
    if (t < 0 || t >= vocab) {                      // no token to embed (misuse): a visible NaN row, nothing read out of range
        for (int d = threadIdx.x; d < D; d += ENT) dst[d] = __builtin_nanf("");
        return;
    }
    const float* e = img + (size_t)t * D;
    const float* pr = row_e + (size_t)(i / n) * D;
    const float* pc = col_e + (size_t)(i % n) * D;
    for (int d = threadIdx.x; d < D; d += ENT) dst[d] = e[d] + (pr[d] + pc[d]);
}

// ------------------------------------------------------------------------------------------------------------------------------
// sampler: one work-group per output row.  Passes over the row (L2-resident: re-read instead of held, so V is bounded by nothing
// but int range): write-out / argmax, then for top-k four 8-bit radix passes over order-preserving keys in LDS, for top-p a maximum
// pass and four more radix passes whose bins hold fixed-point softmax mass instead of counts, then the Gumbel-max draw.  Guidance mix
// and temperature in the eager code's fp32 operations, no contraction.
// ------------------------------------------------------------------------------------------------------------------------------
constexpr int SNT = 256;
enum { MODE_GREEDY = 0, MODE_SAMPLE = 1, MODE_FORCED = 2 };

struct SampleParams {
    const float* logits; long long ld_l, u_off;     // row r at logits + r*ld_l, its unconditional row u_off further
    int B, V, guided, mode, top_k, L;
    const float* params;                             // {temperature, cond_scale} and, with has_p, top_p
    int has_p;                                       // params holds a third float (mas_sample_tokens_topp)
    const long long* seed;                           // {seed, offset}
    const int* step;
    const long long* forced; long long ld_f;
    const unsigned char* keep; long long ld_k;       // image prompt (mas_sample_tokens_prompt): row r keeps forced[r, k] where keep[r, k] != 0
    long long* tokens; long long ld_t;
    float* lout; long long ld_lo;                    // row r, step k at lout + r*ld_lo + k*V
};

__device__ __forceinline__ unsigned okey(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float okey_inv(unsigned k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

__device__ __forceinline__ void better(float& bv, int& bi, float v, int i) {
    if (v > bv || (v == bv && i < bi)) { bv = v; bi = i; }
}

// block-wide (max, lowest index) of the per-thread bests; every thread gets the result
__device__ int block_argmax(float bv, int bi, float* sv, int* si) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(bv, off);
        const int oi = __shfl_xor(bi, off);
        better(bv, bi, ov, oi);
    }
    if (lane == 0) { sv[wave] = bv; si[wave] = bi; }
    __syncthreads();
    float v = sv[0];
    int i = si[0];
#pragma unroll
    for (int w = 1; w < SNT / 64; ++w) better(v, i, sv[w], si[w]);
    return i;
}

__global__ __launch_bounds__(SNT) void sample_kernel(SampleParams p) {
    const int r = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int k = *p.step;
    if (k < 0 || k >= p.L) return;                  // misuse guard: no token slot for this step
    const float* lc = p.logits + (size_t)r * p.ld_l;
    const float* lu = lc + p.u_off;
    const float s = p.params[1], T = p.params[0];
    const int V = p.V;
    auto mixed = [&](int j) -> float {
#pragma clang fp contract(off)
        return p.guided ? lu[j] + s * (lc[j] - lu[j]) : lc[j];      // the eager fp32 ops, each rounded (no fused multiply-add)
    };
    __shared__ float sv[SNT / 64];
    __shared__ int si[SNT / 64];

    if (p.lout) {
        float* dst = p.lout + (size_t)r * p.ld_lo + (size_t)k * V;
        for (int j = tid; j < V; j += SNT) dst[j] = mixed(j);
    }
    if (p.mode == MODE_FORCED || (p.keep && p.keep[(size_t)r * p.ld_k + k])) {    // uniform over the work-group: one row, one step
        if (tid == 0) p.tokens[(size_t)r * p.ld_t + k] = p.forced[(size_t)r * p.ld_f + k];
        return;
    }
    if (p.mode == MODE_GREEDY) {                     // torch.argmax: the first index of the maximum
        float bv = -INFINITY;
        int bi = 0x7fffffff;
        for (int j = tid; j < V; j += SNT) better(bv, bi, mixed(j), j);
        const int best = block_argmax(bv, bi, sv, si);
        if (tid == 0) p.tokens[(size_t)r * p.ld_t + k] = best < V ? best : 0;
        return;
    }

    // ---- top-k threshold: the k-th largest lg (radix select, MSB first, exact counts in LDS) ----
    float kth = -INFINITY;
    if (p.top_k > 0 && p.top_k < V) {
        __shared__ unsigned hist[256];
        __shared__ unsigned sel[2];
        unsigned prefix = 0, pmask = 0, need = (unsigned)p.top_k;
        for (int shift = 24; shift >= 0; shift -= 8) {
            hist[tid] = 0;
            __syncthreads();
            for (int j = tid; j < V; j += SNT) {
                const unsigned key = okey(mixed(j) / T);
                if ((key & pmask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (wave == 0) {                         // lane l holds bins 255-4l .. 252-4l (descending): inclusive scan, first lane >= need
                unsigned c[4], tot = 0;
#pragma unroll
                for (int e = 0; e < 4; ++e) { c[e] = hist[255 - 4 * lane - e]; tot += c[e]; }
                unsigned incl = tot;
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const unsigned t = __shfl_up(incl, off);
                    if (lane >= off) incl += t;
                }
                const unsigned long long bal = __ballot(incl >= need);
                if (lane == __ffsll((unsigned long long)bal) - 1) {
                    unsigned before = incl - tot;
                    int e = 0;
                    for (; e < 3; ++e) {
                        if (before + c[e] >= need) break;
                        before += c[e];
                    }
                    sel[0] = 255u - 4u * lane - e;
                    sel[1] = need - before;
                }
            }
            __syncthreads();
            prefix |= sel[0] << shift;
            pmask |= 255u << shift;
            need = sel[1];
        }
        kth = okey_inv(prefix);
    }

    // ---- top-p threshold (include/mas_hip.h, "Top-p"): t* = the largest value x whose mass at or above it exceeds top_p of the total over
    // the top-k set.  The same radix select as above with masses in the bins: w_j = floor(exp(lg_j - max) * 2^32) added as 64-bit integers
    // -- exact, so no sum depends on the order of the atomics, and the bins below a chosen bin add up to exactly its mass: every level
    // finds its crossing inside the bin chosen above it.  `above` is the mass of the keys greater than every key with the prefix.
    if (p.has_p && p.params[2] < 1.f) {              // uniform; NaN and >= 1 are off, like a launch without the third float
        const float tp = fmaxf(p.params[2], 0.f);
        float mv = -INFINITY;
        int mi = 0x7fffffff;
        for (int j = tid; j < V; j += SNT) {
            const float lg = mixed(j) / T;
            if (lg >= kth) better(mv, mi, lg, j);
        }
        const int at = block_argmax(mv, mi, sv, si);
        __syncthreads();                             // sv / si are read: the draw's reduction below may write them again
        const float mx = at < V ? mixed(at) / T : INFINITY;
        if (mx < INFINITY && mx > -INFINITY) {       // uniform.  No finite maximum: no softmax to cut, the top-k set stays as it is
            __shared__ unsigned long long mass[256];
            __shared__ unsigned long long msel[2];
            unsigned prefix = 0, pmask = 0;
            unsigned long long above = 0, line = 0;  // line = floor(top_p * W): for integers, incl > top_p * W  <=>  incl > line
            bool cut = true;
            for (int shift = 24; shift >= 0; shift -= 8) {
                mass[tid] = 0;
                __syncthreads();
                for (int j = tid; j < V; j += SNT) {
                    const float lg = mixed(j) / T;
                    if (!(lg >= kth)) continue;
                    const unsigned key = okey(lg);
                    if ((key & pmask) == prefix)
                        atomicAdd(&mass[(key >> shift) & 255u], (unsigned long long)(expf(lg - mx) * 4294967296.f));
                }
                __syncthreads();
                if (wave == 0) {                     // bins in descending order, as in the count select
                    unsigned long long c[4], tot = 0;
#pragma unroll
                    for (int e = 0; e < 4; ++e) { c[e] = mass[255 - 4 * lane - e]; tot += c[e]; }
                    unsigned long long incl = tot;
#pragma unroll
                    for (int off = 1; off < 64; off <<= 1) {
                        const unsigned long long t = __shfl_up(incl, off);
                        if (lane >= off) incl += t;
                    }
                    if (shift == 24) line = (unsigned long long)((double)tp * (double)__shfl(incl, 63));   // W: exact below 2^53
                    const unsigned long long bal = __ballot(above + incl > line);
                    if (bal == 0) {
                        if (lane == 0) msel[0] = 256;    // the line is not below the total (rounding at top_p next to 1): no cut
                    } else if (lane == __ffsll(bal) - 1) {
                        unsigned long long before = above + incl - tot;
                        int e = 0;
                        for (; e < 3; ++e) {
                            if (before + c[e] > line) break;
                            before += c[e];
                        }
                        msel[0] = 255u - 4u * lane - e;
                        msel[1] = before;
                    }
                }
                __syncthreads();
                if (msel[0] > 255) { cut = false; break; }     // uniform
                prefix |= (unsigned)msel[0] << shift;
                pmask |= 255u << shift;
                above = msel[1];
            }
            if (cut) kth = okey_inv(prefix);         // a key of the top-k set: never below the top-k threshold
        }
    }

    // ---- Gumbel-max over the kept entries: argmax(lg_j - log(-log u_j)), lowest index on ties ----
    const unsigned long long sd = (unsigned long long)p.seed[0];
    const unsigned s0 = (unsigned)sd, s1 = (unsigned)(sd >> 32), off = (unsigned)(unsigned long long)p.seed[1];
    float bv = -INFINITY;
    int bi = 0x7fffffff;
    for (int j4 = 4 * tid; j4 < V; j4 += 4 * SNT) {
        const MasU32x4 w = mas_sample_bits4(s0, s1, off, (unsigned)r, (unsigned)k, (unsigned)(j4 >> 2));
        const unsigned bits[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int j = j4 + e;
            if (j >= V) break;
            const float lg = mixed(j) / T;
            if (!(lg >= kth)) continue;
            const float u = mas_sample_uniform(bits[e]);
            better(bv, bi, lg - logf(-logf(u)), j);
        }
    }
    const int best = block_argmax(bv, bi, sv, si);
    if (tid == 0) p.tokens[(size_t)r * p.ld_t + k] = best < V ? best : 0;
}

__global__ void advance_kernel(int* ctr, int n) {
    if (threadIdx.x == 0)
        for (int i = 0; i < n; ++i) ctr[i] += 1;
}

}  // namespace

extern "C" int mas_attn_decode_dev(const void* q, const void* k_new, const void* v_new, long long new_bs, void* k_cache, void* v_cache,
                                   int ld_c, long long c_bs, int capacity, void* o, long long o_bs, int dtype, int B, int H, int hd,
                                   const int32_t* past, float scale, void* stream) {
    MAS_ENTER();
    if (!q || !k_new || !v_new || !k_cache || !v_cache || !o || !past) MAS_FAIL(MAS_EINVAL, "attn_decode_dev: null argument");
    if (B <= 0 || H <= 0 || capacity <= 0 || ld_c < H * hd || c_bs < (long long)capacity * ld_c)
        MAS_FAIL(MAS_EINVAL, "attn_decode_dev: bad shape B=%d H=%d hd=%d capacity=%d ld=%d", B, H, hd, capacity, ld_c);
    const size_t esz = mas_esize(dtype);
    const int epu = 16 / (int)esz;
    if ((ld_c % epu) || (new_bs % epu) || (c_bs % epu) ||
        ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k_new) | reinterpret_cast<uintptr_t>(v_new) |
          reinterpret_cast<uintptr_t>(k_cache) | reinterpret_cast<uintptr_t>(v_cache)) & 15))
        MAS_FAIL(MAS_EUNSUPPORTED, "attn_decode_dev: q / k / v rows must be 16-byte aligned");
    DecodeDevParams p;
    p.q = q; p.kn = k_new; p.vn = v_new; p.kc = k_cache; p.vc = v_cache; p.o = o;
    p.new_bs = new_bs; p.c_bs = c_bs; p.o_bs = o_bs; p.ld_c = ld_c;
    p.B = B; p.H = H; p.cap = capacity; p.past = past; p.scale = scale;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == MAS_BF16) return launch_decode_dev<bf16_t>(p, hd, s);
    if (dtype == MAS_F32) return launch_decode_dev<float>(p, hd, s);
    MAS_FAIL(MAS_EUNSUPPORTED, "attn_decode_dev: dtype %d", dtype);
}

extern "C" int mas_decode_embed(const int64_t* tokens, long long ld_tok, const int32_t* step, const float* img_emb, int vocab,
                                const float* row_emb, const float* col_emb, int n, float* out, int B, int rows, int D, void* stream) {
    MAS_ENTER();
    if (!tokens || !step || !img_emb || !row_emb || !col_emb || !out) MAS_FAIL(MAS_EINVAL, "decode_embed: null argument");
    if (B <= 0 || rows <= 0 || rows % B || D <= 0 || n <= 0 || vocab <= 0 || ld_tok < (long long)n * n)
        MAS_FAIL(MAS_EINVAL, "decode_embed: bad shape B=%d rows=%d D=%d n=%d vocab=%d", B, rows, D, n, vocab);
    hipLaunchKernelGGL(decode_embed_kernel, dim3((unsigned)rows), dim3(ENT), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const long long*>(tokens), ld_tok, step, img_emb, vocab, row_emb, col_emb, n, out, B, D);
    MAS_CHECK_LAUNCH("decode_embed");
    return MAS_OK;
}

namespace {
int sample_tokens_launch(const float* logits, long long ld_logits, long long uncond_off, int B, int V, int guided, int mode, int top_k,
                         const float* params, int has_p, const int64_t* seed, const int32_t* step, int L, const int64_t* forced,
                         long long ld_forced, const uint8_t* keep, long long ld_keep, int64_t* tokens, long long ld_tokens,
                         float* logits_out, long long ld_logits_out, void* stream) {
    if (!logits || !params || !step || !tokens) MAS_FAIL(MAS_EINVAL, "sample_tokens: null argument");
    if (B <= 0 || V <= 0 || L <= 0 || ld_logits < 0 || ld_tokens < L || (logits_out && ld_logits_out < (long long)L * V))
        MAS_FAIL(MAS_EINVAL, "sample_tokens: bad shape B=%d V=%d L=%d", B, V, L);
    if (mode != MODE_GREEDY && mode != MODE_SAMPLE && mode != MODE_FORCED) MAS_FAIL(MAS_EINVAL, "sample_tokens: mode %d", mode);
    if (mode == MODE_SAMPLE && !seed) MAS_FAIL(MAS_EINVAL, "sample_tokens: sampling needs a seed");
    if (mode == MODE_FORCED && (!forced || ld_forced < L)) MAS_FAIL(MAS_EINVAL, "sample_tokens: teacher forcing needs the tokens");
    SampleParams p;
    p.logits = logits; p.ld_l = ld_logits; p.u_off = guided ? uncond_off : 0;
    p.B = B; p.V = V; p.guided = guided != 0; p.mode = mode; p.top_k = top_k; p.L = L;
    p.params = params; p.has_p = has_p; p.seed = reinterpret_cast<const long long*>(seed); p.step = step;
    p.forced = reinterpret_cast<const long long*>(forced); p.ld_f = ld_forced;
    p.keep = keep; p.ld_k = ld_keep;
    p.tokens = reinterpret_cast<long long*>(tokens); p.ld_t = ld_tokens;
    p.lout = logits_out; p.ld_lo = ld_logits_out;
    hipLaunchKernelGGL(sample_kernel, dim3((unsigned)B), dim3(SNT), 0, reinterpret_cast<hipStream_t>(stream), p);
    MAS_CHECK_LAUNCH("sample_tokens");
    return MAS_OK;
}
}  // namespace

extern "C" int mas_sample_tokens(const float* logits, long long ld_logits, long long uncond_off, int B, int V, int guided, int mode,
                                 int top_k, const float* params, const int64_t* seed, const int32_t* step, int L, const int64_t* forced,
                                 long long ld_forced, int64_t* tokens, long long ld_tokens, float* logits_out, long long ld_logits_out,
                                 void* stream) {
    MAS_ENTER();
    return sample_tokens_launch(logits, ld_logits, uncond_off, B, V, guided, mode, top_k, params, 0, seed, step, L, forced, ld_forced,
                                nullptr, 0, tokens, ld_tokens, logits_out, ld_logits_out, stream);
}

extern "C" int mas_sample_tokens_topp(const float* logits, long long ld_logits, long long uncond_off, int B, int V, int guided, int mode,
                                      int top_k, const float* params, const int64_t* seed, const int32_t* step, int L,
                                      const int64_t* forced, long long ld_forced, int64_t* tokens, long long ld_tokens, float* logits_out,
                                      long long ld_logits_out, void* stream) {
    MAS_ENTER();
    return sample_tokens_launch(logits, ld_logits, uncond_off, B, V, guided, mode, top_k, params, 1, seed, step, L, forced, ld_forced,
                                nullptr, 0, tokens, ld_tokens, logits_out, ld_logits_out, stream);
}

extern "C" int mas_sample_tokens_prompt(const float* logits, long long ld_logits, long long uncond_off, int B, int V, int guided, int mode,
                                        int top_k, const float* params, const int64_t* seed, const int32_t* step, int L,
                                        const int64_t* forced, long long ld_forced, int64_t* tokens, long long ld_tokens, float* logits_out,
                                        long long ld_logits_out, const uint8_t* keep, long long ld_keep, void* stream) {
    MAS_ENTER();
    if (mode == MODE_FORCED) MAS_FAIL(MAS_EINVAL, "sample_tokens_prompt: mode 2 forces every position, it takes no mask");
    if (!keep || !forced || ld_keep < L || ld_forced < L)
        MAS_FAIL(MAS_EINVAL, "sample_tokens_prompt: needs the mask and the kept tokens, rows of at least L=%d elements", L);
    return sample_tokens_launch(logits, ld_logits, uncond_off, B, V, guided, mode, top_k, params, 1, seed, step, L, forced, ld_forced,
                                keep, ld_keep, tokens, ld_tokens, logits_out, ld_logits_out, stream);
}

extern "C" int mas_decode_advance(int32_t* counters, int n, void* stream) {
    MAS_ENTER();
    if (!counters || n <= 0 || n > 8) MAS_FAIL(MAS_EINVAL, "decode_advance: bad arguments");
    hipLaunchKernelGGL(advance_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), counters, n);
    MAS_CHECK_LAUNCH("decode_advance");
    return MAS_OK;
}
