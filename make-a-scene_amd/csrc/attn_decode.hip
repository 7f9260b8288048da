// Decode-time (KV-cached) attention for gfx950: a few new queries against a long cache of keys / values.
// Replaces the cached branch of SelfAttention.forward (reference models/transformer.py:73-115: qkv of the new positions,
// torch.cat with past_k / past_v, calculate_attention on the last rows of the mask, Softmax, matmul) for token-by-token
// sampling.  The reference re-concatenates the whole [B,H,S,hd] cache every step (O(S^2) copies per sample) and materialises
// the [B,H,nq,S] scores; here the cache is a preallocated [B, S_max, H*hd] buffer (the layout nn.Linear emits), the new
// rows are appended in place by the host wrapper, and scores never leave registers.
//
// Regime: HBM / L2 bound (every key and value row is read exactly once per query block: 2 * L * hd * sizeof(T) bytes per
// (batch, head)), no matrix cores -- one dot product per key.  One work-group per (batch, head, query); a lane owns a key:
// it reads the key's contiguous hd-element row (whole 128-byte lines at hd = 64 bf16), keeps an online-softmax partial
// (m, l, o[hd]) over its keys in registers, and the 256 partials are merged once at the end (wave shuffles, then LDS).
// Query i of the block (0 <= i < nq) sees keys 0 .. past + i (causal inside the block, transformer.py:260-263,366-370).
#include "attn_decode_core.h"

namespace {

struct DecodeParams {
    const void* q; const void* k; const void* v; void* o;
    long long q_bs, k_bs, v_bs, o_bs;   // batch strides (elements)
    int ld_q, ld_k, ld_v, ld_o;         // token strides (elements)
    int B, H, nq, past;
    float scale;
};

template <typename T, int HD>
__global__ __launch_bounds__(DECODE_NT) void attn_decode_kernel(DecodeParams p) {
    const int iq = blockIdx.x, bh = blockIdx.y, b = bh / p.H, h = bh % p.H;
    const T* Q = reinterpret_cast<const T*>(p.q) + (size_t)b * p.q_bs + (size_t)iq * p.ld_q + (size_t)h * HD;
    const T* K = reinterpret_cast<const T*>(p.k) + (size_t)b * p.k_bs + (size_t)h * HD;
    const T* V = reinterpret_cast<const T*>(p.v) + (size_t)b * p.v_bs + (size_t)h * HD;
    T* dst = reinterpret_cast<T*>(p.o) + (size_t)b * p.o_bs + (size_t)iq * p.ld_o + (size_t)h * HD;
    attn_decode_body<T, HD>(Q, K, V, dst, p.ld_k, p.ld_v, p.past + iq + 1, p.scale);   // query iq sees keys 0 .. past + iq
}

template <typename T>
int launch_decode(const DecodeParams& p, int hd, hipStream_t s) {
    const dim3 grid((unsigned)p.nq, (unsigned)(p.B * p.H));
    if (!decode_dispatch_hd(hd, [&](auto hd_c) {
            hipLaunchKernelGGL((attn_decode_kernel<T, decltype(hd_c)::value>), grid, dim3(DECODE_NT), 0, s, p);
        }))
        MAS_FAIL(MAS_EUNSUPPORTED, "attn_decode: head_dim %d not in {16,32,64,128}", hd);
    MAS_CHECK_LAUNCH("attn_decode");
    return MAS_OK;
}

}  // namespace

extern "C" int mas_attn_decode(const void* q, const void* k_cache, const void* v_cache, void* o, int dtype, int B, int H, int nq,
                               int past, int hd, int ld_q, int ld_k, int ld_v, int ld_o, long long q_bs, long long k_bs,
                               long long v_bs, long long o_bs, float scale, void* stream) {
    MAS_ENTER();
    if (!q || !k_cache || !v_cache || !o) MAS_FAIL(MAS_EINVAL, "attn_decode: null argument");
    if (B <= 0 || H <= 0 || nq <= 0 || past < 0) MAS_FAIL(MAS_EINVAL, "attn_decode: bad shape B=%d H=%d nq=%d past=%d", B, H, nq, past);
    const size_t esz = mas_esize(dtype);
    const int epu = 16 / (int)esz;
    if ((ld_q % epu) || (ld_k % epu) || (ld_v % epu) || (q_bs % epu) || (k_bs % epu) || (v_bs % epu) ||
        ((reinterpret_cast<uintptr_t>(q) | reinterpret_cast<uintptr_t>(k_cache) | reinterpret_cast<uintptr_t>(v_cache)) & 15))
        MAS_FAIL(MAS_EUNSUPPORTED, "attn_decode: q / k / v rows must be 16-byte aligned");
    DecodeParams p;
    p.q = q; p.k = k_cache; p.v = v_cache; p.o = o;
    p.q_bs = q_bs; p.k_bs = k_bs; p.v_bs = v_bs; p.o_bs = o_bs;
    p.ld_q = ld_q; p.ld_k = ld_k; p.ld_v = ld_v; p.ld_o = ld_o;
    p.B = B; p.H = H; p.nq = nq; p.past = past; p.scale = scale;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (dtype == MAS_BF16) return launch_decode<bf16_t>(p, hd, s);
    if (dtype == MAS_F32) return launch_decode<float>(p, hd, s);
    MAS_FAIL(MAS_EUNSUPPORTED, "attn_decode: dtype %d", dtype);
}
