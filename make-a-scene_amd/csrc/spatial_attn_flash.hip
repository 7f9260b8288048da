// The spatial self-attention core of AttnBlock beyond 256 tokens (gfx950): the arithmetic of spatial_attn.hip -- softmax_keys(q k^T C^-1/2) v
// on the fused [N, S, 3C] projection, bf16 storage / fp32 accumulate -- with an ONLINE softmax over 256-key chunks, so that S is bounded by
// nothing in LDS: 1 <= S <= 4096 (the 64x64 grid of a 1024^2 input; the 512^2 model of conf/img_config.yaml has 32x32 = 1024 tokens).
// Built from the same two tile products (spatial_attn_core.h): a chunk is exactly the shipped kernel's whole problem (<= 256 columns, one
// 32-column score tile per wave), and what is new is what lives ACROSS the chunks:
//   * the 32-row block is staged in LDS once and multiplied with every chunk (sp_prod_t<false>);
//   * the output accumulators are carried (sp_apply_run_t<false> adds into them);
//   forward        : per chunk  T = prod(Q_blk, K_c);  m' = max(m, rowmax T);  O *= exp(m - m');  l = l exp(m - m') + rowsum exp(T - m');
//                    P = bf16(exp(T - m')) (unnormalised) -> LDS;  O += apply(P, V_c).   After the loop O /= l, lse = m + log l.
//   backward, dQ   : delta = rowsum(dO o O) from the saved output, BEFORE the loop (it spans all chunks; published for the second launch);
//                    per chunk  P = exp(scale prod(Q_blk, K_c) - lse);  dP = prod(dO_blk, V_c);  dS = scale P (dP - delta);  dQ += apply(dS, K_c)
//   backward, dK/dV: block = 32 KEYS, chunks of queries (lse / delta indexed by column):  dV += apply(P^T, dO_c),  dK += apply(dS^T, Q_c),
//                    both accumulators live across the loop.
// 32 rows per work-group, 8 waves.  The blocks of an image start on different chunks (and, inside a chunk, on different tiles: `rot`), so that
// the work-groups an XCD runs together do not wait for the same lines.  No atomics: every output element is written exactly once, by one
// work-group, in an order that depends on its block index only -- results repeat bit for bit.
#include "spatial_attn_core.h"

namespace {

constexpr int KC = S_MAX;                        // keys (queries, in the dK/dV kernel) per chunk
constexpr int SF_S_MAX = 4096;
// Registers (256 per wave at two waves per SIMD; the accumulators carried across the chunks come on top of what spatial_attn.hip holds):
// fragment ring of the first product / tiles in flight in the second, per kernel.  The dK/dV kernel carries TWO accumulator sets: ring of
// 2, two tiles in flight, and P takes a round trip through LDS (see there).  Anything deeper spills.
constexpr int FWD_RING = 4, FWD_PF = 4, DQ_RING = 4, DQ_PF = 3, DKV_RING = 2, DKV_PF = 2;

// LDS map: one (forward) or two (backward) staged 32-row blocks, ONE bf16 P / dS operand of KC columns, the two M tile buffers, a pad.
// C = 512: 33280 x {1, 2} + 16896 + 2 x 34816 + 2048 = 121856 (forward), 155136 (backward) bytes -- one work-group per CU either way.
struct SfLds {
    int RX, SP, RM;
    int o_x, o_x2, o_p, o_m0, o_m1, o_r, total;
    __host__ __device__ SfLds(int C, bool two) {
        RX = ((C + 127) & ~127) * 2 + 16; SP = KC * 2 + 16; RM = C * 2 + 64;
        o_x = 0; o_x2 = 32 * RX; o_p = o_x2 + (two ? 32 * RX : 0); o_m0 = o_p + 32 * SP; o_m1 = o_m0 + 32 * RM; o_r = o_m1 + 32 * RM;
        total = o_r + 2 * NW * 32 * 4;
    }
};

// rows [r0, r0 + 32) of X -> xs (rows >= S and channels >= C zero); the caller's barrier makes them visible
__device__ __forceinline__ void sf_stage(unsigned char* xs, int RX, const bf16_t* X, int ldx, int r0, int S, int C, int tid) {
    const SpMap mp(C, tid);
    u32x4 xr[UPT];
    sp_rows_fetch(xr, X, ldx, r0, S, mp);
    sp_rows_commit(xr, xs, RX, r0, S, mp);
    sp_rows_zero_pad(xs, RX, C, tid);
}

// The per-lane addresses of a chunk's loads are functions of tid and of nothing that changes from chunk to chunk, so the compiler hoists
// every one of them out of the chunk loop and keeps them in registers across it (~100 VGPRs: the kernels spilled).  Computed from an
// opaque copy of tid they are rebuilt per chunk, beside memory round trips that hide them.
__device__ __forceinline__ int sf_opaque(int v) { asm volatile("" : "+v"(v)); return v; }

// a lane's own elements of the bf16 rows that sp_put_rows wrote (the same lane wrote them: no barrier in between); 0 for a tile past S
__device__ __forceinline__ void sf_get_rows(f32x16 (&v)[TPW], const unsigned char* ps, int SP, int S, const int (&mts)[TPW], int g, int l31) {
    asm volatile("" ::: "memory");
    const int n_mt = (S + 31) / 32;
#pragma unroll
    for (int ti = 0; ti < TPW; ++ti) {
        const int mt = mts[ti];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const bf16x4 o = *reinterpret_cast<const bf16x4*>(ps + l31 * SP + (min(mt, n_mt - 1) * 32 + 8 * q + 4 * g) * 2);
#pragma unroll
            for (int e = 0; e < 4; ++e) v[ti][4 * q + e] = mt < n_mt ? (float)o[e] : 0.0f;
        }
    }
}

struct SfChunk {
    int c0, Sc, rt;                              // first row of the chunk, its rows (1..KC), the apply's start tile (< its tile count)
    __device__ __forceinline__ SfChunk(int i, int nch, int rot, int S) {
        int c = i + rot % nch;                   // the blocks of an image walk the chunks from different starts
        if (c >= nch) c -= nch;
        c0 = c * KC; Sc = min(KC, S - c0); rt = rot % ((Sc + 31) / 32);
    }
};

// ---- forward: one work-group per (image, 32-query block) -----------------------------------------------------------------------
__global__ __launch_bounds__(SNT) void spatial_attn_flash_fwd_kernel(SpParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const SfLds L(p.C, false);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 5, l31 = lane & 31;
    const int nqb = (p.S + 31) / 32, nch = (p.S + KC - 1) / KC;
    const int blk = sp_logical_block((int)gridDim.x);
    const int n = blk / nqb, rot = blk % nqb, q0 = rot * 32;
    const int ld = 3 * p.C;
    const bf16_t* Q = p.qkv + (size_t)n * p.S * ld;
    const bf16_t* K = Q + p.C;
    const bf16_t* V = Q + 2 * p.C;
    float* pad = reinterpret_cast<float*>(smem + L.o_r);

    sf_stage(smem + L.o_x, L.RX, Q, ld, q0, p.S, p.C, tid);
    __syncthreads();
    f32x16 acc[CPW];
#pragma unroll
    for (int i = 0; i < CPW; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;
    float m = -1e30f, l = 0.0f;                   // running maximum and sum of query l31 (both lane halves hold them)
    for (int ci = 0; ci < nch; ++ci) {
        const SfChunk ch(ci, nch, rot, p.S);
        const int tl = sf_opaque(tid);
        const bf16_t* Kc = K + (size_t)ch.c0 * ld;
        const bf16_t* Vc = V + (size_t)ch.c0 * ld;
        int mt[TPW];
        sp_tiles(mt, wave, ch.Sc, rot);
        f32x16 sc[TPW];
        sp_prod_t<false, FWD_RING>(sc, mt, rot, smem + L.o_x, L.RX, nullptr, 0, 0, 0, Kc, ld, ch.Sc, p.C, tl);
        u32x4 pf[FWD_PF][UPT];
        sp_apply_issue(pf, Vc, ld, ch.Sc, p.C, ch.rt, tl);          // four V tiles travel while the softmax runs
        float mx = -1e30f;
#pragma unroll
        for (int ti = 0; ti < TPW; ++ti)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (sp_col(mt, ti, r, g) < ch.Sc) mx = fmaxf(mx, sc[ti][r] * p.scale);
        mx = sp_row_reduce<true>(mx, pad, wave, g, l31);
        const float mn = fmaxf(m, mx);            // (every chunk has a valid column: mn is a real score from the first chunk on)
        const float alpha = __expf(m - mn);       // first chunk: exp(-1e30 - mn) = 0, never inf - inf
        float sum = 0.0f;
#pragma unroll
        for (int ti = 0; ti < TPW; ++ti)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float e = sp_col(mt, ti, r, g) < ch.Sc ? __expf(sc[ti][r] * p.scale - mn) : 0.0f;
                sc[ti][r] = e;
                sum += e;
            }
        sum = sp_row_reduce<false>(sum, pad + NW * 32, wave, g, l31);
        l = l * alpha + sum;
        m = mn;
        sp_put_rows(smem + L.o_p, L.SP, sc, ch.Sc, mt, g, l31);
#pragma unroll
        for (int i = 0; i < CPW; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] *= alpha;         // acc[i][r] belongs to query l31, as alpha does
        sp_apply_run_t<false>(acc, pf, smem + L.o_p, L.SP, smem + L.o_m0, smem + L.o_m1, L.RM, Vc, ld, ch.Sc, p.C, ch.rt, tl);
    }
    const float inv = 1.0f / l;
#pragma unroll
    for (int i = 0; i < CPW; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] *= inv;
    if (wave == 0 && g == 0 && q0 + l31 < p.S && p.lse) p.lse[(size_t)n * p.S + q0 + l31] = m + __logf(l);
    sp_store(acc, p.out + (size_t)n * p.S * p.C, p.C, q0, p.S, p.C, tid);
}

// ---- backward, dQ: one work-group per (image, 32-query block); publishes delta ---------------------------------------------------
__global__ __launch_bounds__(SNT) void spatial_attn_flash_bwd_dq_kernel(SpParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const SfLds L(p.C, true);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 5, l31 = lane & 31;
    const int nb = (p.S + 31) / 32, nch = (p.S + KC - 1) / KC;
    const int blk = sp_logical_block((int)gridDim.x);
    const int n = blk / nb, rot = blk % nb, r0 = rot * 32;
    const int ld = 3 * p.C;
    const bf16_t* Q = p.qkv + (size_t)n * p.S * ld;
    const bf16_t* K = Q + p.C;
    const bf16_t* V = Q + 2 * p.C;
    const bf16_t* dO = p.dout + (size_t)n * p.S * p.C;
    const bf16_t* O = p.o + (size_t)n * p.S * p.C;
    float* pad = reinterpret_cast<float*>(smem + L.o_r);
    const bool row_ok = r0 + l31 < p.S;

    sf_stage(smem + L.o_x, L.RX, Q, ld, r0, p.S, p.C, tid);
    sf_stage(smem + L.o_x2, L.RX, dO, p.C, r0, p.S, p.C, tid);
    {   // delta_q = sum_c dO[q][c] O[q][c] (= sum_keys P dP): SNT / 32 threads per row, 16-byte units, the partial sums meet by lane shuffles
        constexpr int TPR = SNT / 32;
        const int row = tid / TPR, j = tid % TPR, rr = min(r0 + row, p.S - 1);
        float part = 0.0f;
        for (int cu = j; cu < p.C / 8; cu += TPR) {
            const bf16x8 a = *reinterpret_cast<const bf16x8*>(dO + (size_t)rr * p.C + cu * 8);
            const bf16x8 b = *reinterpret_cast<const bf16x8*>(O + (size_t)rr * p.C + cu * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) part += (float)a[e] * (float)b[e];
        }
#pragma unroll
        for (int o = TPR / 2; o > 0; o >>= 1) part += __shfl_xor(part, o);
        if (j == 0) {
            pad[row] = part;
            if (r0 + row < p.S) p.delta[(size_t)n * p.S + r0 + row] = part;
        }
    }
    __syncthreads();
    const float drow = pad[l31];
    const float lrow = row_ok ? p.lse[(size_t)n * p.S + r0 + l31] : 0.0f;
    f32x16 acc[CPW];
#pragma unroll
    for (int i = 0; i < CPW; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;
    for (int ci = 0; ci < nch; ++ci) {
        const SfChunk ch(ci, nch, rot, p.S);
        const int tl = sf_opaque(tid);
        const bf16_t* Kc = K + (size_t)ch.c0 * ld;
        const bf16_t* Vc = V + (size_t)ch.c0 * ld;
        int mt[TPW];
        sp_tiles(mt, wave, ch.Sc, rot);
        f32x16 pv[TPW], dp[TPW];
        sp_prod_t<false, DQ_RING>(pv, mt, rot, smem + L.o_x, L.RX, nullptr, 0, 0, 0, Kc, ld, ch.Sc, p.C, tl);
#pragma unroll
        for (int ti = 0; ti < TPW; ++ti)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                pv[ti][r] = (row_ok && sp_col(mt, ti, r, g) < ch.Sc) ? __expf(pv[ti][r] * p.scale - lrow) : 0.0f;
        sp_prod_t<false, DQ_RING>(dp, mt, rot + 2, smem + L.o_x2, L.RX, nullptr, 0, 0, 0, Vc, ld, ch.Sc, p.C, tl);
        u32x4 pf[DQ_PF][UPT];
        sp_apply_issue(pf, Kc, ld, ch.Sc, p.C, ch.rt, tl);          // K tiles travel under the dS arithmetic
#pragma unroll
        for (int ti = 0; ti < TPW; ++ti)
#pragma unroll
            for (int r = 0; r < 16; ++r) dp[ti][r] = p.scale * pv[ti][r] * (dp[ti][r] - drow);       // dS (pv is 0 outside the valid rows / columns)
        sp_put_rows(smem + L.o_p, L.SP, dp, ch.Sc, mt, g, l31);
        sp_apply_run_t<false>(acc, pf, smem + L.o_p, L.SP, smem + L.o_m0, smem + L.o_m1, L.RM, Kc, ld, ch.Sc, p.C, ch.rt, tl);   // dQ += dS K_c
    }
    sp_store(acc, p.dqkv + (size_t)n * p.S * ld, ld, r0, p.S, p.C, tid);
}

// ---- backward, dK / dV: one work-group per (image, 32-key block), chunks of queries; reads delta ---------------------------------
__global__ __launch_bounds__(SNT) void spatial_attn_flash_bwd_dkv_kernel(SpParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const SfLds L(p.C, true);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 5, l31 = lane & 31;
    const int nb = (p.S + 31) / 32, nch = (p.S + KC - 1) / KC;
    const int blk = sp_logical_block((int)gridDim.x);
    const int n = blk / nb, rot = blk % nb, r0 = rot * 32;
    const int ld = 3 * p.C;
    const bf16_t* Q = p.qkv + (size_t)n * p.S * ld;
    const bf16_t* K = Q + p.C;
    const bf16_t* V = Q + 2 * p.C;
    const bf16_t* dO = p.dout + (size_t)n * p.S * p.C;
    const float* lse = p.lse + (size_t)n * p.S;
    const float* delta = p.delta + (size_t)n * p.S;
    const bool row_ok = r0 + l31 < p.S;

    sf_stage(smem + L.o_x, L.RX, K, ld, r0, p.S, p.C, tid);
    sf_stage(smem + L.o_x2, L.RX, V, ld, r0, p.S, p.C, tid);
    __syncthreads();
    f32x16 accv[CPW], acck[CPW];
#pragma unroll
    for (int i = 0; i < CPW; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) { accv[i][r] = 0.0f; acck[i][r] = 0.0f; }
    for (int ci = 0; ci < nch; ++ci) {
        const SfChunk ch(ci, nch, rot, p.S);
        const int tl = sf_opaque(tid);
        const bf16_t* Qc = Q + (size_t)ch.c0 * ld;
        const bf16_t* dOc = dO + (size_t)ch.c0 * p.C;
        int mt[TPW];
        sp_tiles(mt, wave, ch.Sc, rot);
        f32x16 pv[TPW], dp[TPW];
        sp_prod_t<false, DKV_RING>(pv, mt, rot, smem + L.o_x, L.RX, nullptr, 0, 0, 0, Qc, ld, ch.Sc, p.C, tl);
#pragma unroll
        for (int ti = 0; ti < TPW; ++ti)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int mq = sp_col(mt, ti, r, g);
                const float lq = lse[ch.c0 + min(mq, ch.Sc - 1)];
                pv[ti][r] = (row_ok && mq < ch.Sc) ? __expf(pv[ti][r] * p.scale - lq) : 0.0f;
            }
        // P goes to LDS NOW (the last run of the previous chunk ended on a barrier) and comes back, rounded to bf16 as dV's operand is, after
        // the second product: with two accumulator sets live the 16 registers of P do not fit beside that product's fragments
        sp_put_rows(smem + L.o_p, L.SP, pv, ch.Sc, mt, g, l31);
        sp_prod_t<false, DKV_RING>(dp, mt, rot + 2, smem + L.o_x2, L.RX, nullptr, 0, 0, 0, dOc, p.C, ch.Sc, p.C, tl);
        f32x16 pb[TPW];
        sf_get_rows(pb, smem + L.o_p, L.SP, ch.Sc, mt, g, l31);
#pragma unroll
        for (int ti = 0; ti < TPW; ++ti)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float dq = delta[ch.c0 + min(sp_col(mt, ti, r, g), ch.Sc - 1)];
                dp[ti][r] = p.scale * pb[ti][r] * (dp[ti][r] - dq);
            }
        u32x4 pf[DKV_PF][UPT];
        sp_apply_issue(pf, dOc, p.C, ch.Sc, p.C, ch.rt, tl);        // (after the delta loads: nothing waits behind them)
        sp_apply_run_t<false>(accv, pf, smem + L.o_p, L.SP, smem + L.o_m0, smem + L.o_m1, L.RM, dOc, p.C, ch.Sc, p.C, ch.rt, tl);   // dV += P^T dO_c
        sp_apply_issue(pf, Qc, ld, ch.Sc, p.C, ch.rt, tl);
        sp_put_rows(smem + L.o_p, L.SP, dp, ch.Sc, mt, g, l31);      // (the run above ended on a barrier: every wave has left the P rows)
        sp_apply_run_t<false>(acck, pf, smem + L.o_p, L.SP, smem + L.o_m0, smem + L.o_m1, L.RM, Qc, ld, ch.Sc, p.C, ch.rt, tl);     // dK += dS^T Q_c
    }
    sp_store(accv, p.dqkv + (size_t)n * p.S * ld + 2 * p.C, ld, r0, p.S, p.C, tid);
    sp_store(acck, p.dqkv + (size_t)n * p.S * ld + p.C, ld, r0, p.S, p.C, tid);
}

int sf_check(const char* what, const void* a, const void* b, int dtype, int N, int S, int C) {
    if (!a || !b) MAS_FAIL(MAS_EINVAL, "%s: null argument", what);
    if (dtype != MAS_BF16) MAS_FAIL(MAS_EUNSUPPORTED, "%s: bf16 only (the fp32 parity mode keeps the library GEMM path)", what);
    if (N <= 0 || S <= 0 || S > SF_S_MAX || C <= 0 || C > C_MAX || (C % 32)) MAS_FAIL(MAS_EUNSUPPORTED, "%s: needs S <= %d tokens and C %% 32 == 0, C <= %d (got S=%d C=%d)", what, SF_S_MAX, C_MAX, S, C);
    if ((long long)N * ((S + 31) / 32) > 0x7fffffffLL) MAS_FAIL(MAS_EUNSUPPORTED, "%s: too many blocks (N=%d S=%d)", what, N, S);
    return MAS_OK;
}

}  // namespace

extern "C" int mas_spatial_attn_flash_fwd(const void* qkv, void* out, float* lse, int dtype, int N, int S, int C, void* stream) {
    MAS_ENTER();
    if (int rc = sf_check("spatial_attn_flash_fwd", qkv, out, dtype, N, S, C)) return rc;
    SpParams p{};
    p.qkv = (const bf16_t*)qkv; p.out = (bf16_t*)out; p.lse = lse; p.N = N; p.S = S; p.C = C; p.scale = 1.0f / sqrtf((float)C);
    const SfLds L(C, false);
    static mas_devmask_t mask{0};
    if (int rc = sp_set_lds(spatial_attn_flash_fwd_kernel, L.total, "spatial_attn_flash_fwd", mask)) return rc;
    hipLaunchKernelGGL(spatial_attn_flash_fwd_kernel, dim3((unsigned)(N * ((S + 31) / 32))), dim3(SNT), (size_t)L.total, reinterpret_cast<hipStream_t>(stream), p);
    MAS_CHECK_LAUNCH("spatial_attn_flash_fwd");
    return MAS_OK;
}

extern "C" int mas_spatial_attn_flash_bwd(const void* qkv, const void* out, const void* dout, const float* lse, float* delta, void* dqkv,
                                          int dtype, int N, int S, int C, void* stream) {
    MAS_ENTER();
    if (int rc = sf_check("spatial_attn_flash_bwd", qkv, dout, dtype, N, S, C)) return rc;
    if (!out || !lse || !delta || !dqkv) MAS_FAIL(MAS_EINVAL, "spatial_attn_flash_bwd: null argument");
    SpParams p{};
    p.qkv = (const bf16_t*)qkv; p.o = (const bf16_t*)out; p.dout = (const bf16_t*)dout; p.dqkv = (bf16_t*)dqkv;
    p.lse = const_cast<float*>(lse); p.delta = delta; p.N = N; p.S = S; p.C = C; p.scale = 1.0f / sqrtf((float)C);
    const SfLds L(C, true);
    static mas_devmask_t m0{0}, m1{0};
    if (int rc = sp_set_lds(spatial_attn_flash_bwd_dq_kernel, L.total, "spatial_attn_flash_bwd", m0)) return rc;
    if (int rc = sp_set_lds(spatial_attn_flash_bwd_dkv_kernel, L.total, "spatial_attn_flash_bwd", m1)) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(N * ((S + 31) / 32)));
    hipLaunchKernelGGL(spatial_attn_flash_bwd_dq_kernel, grid, dim3(SNT), (size_t)L.total, s, p);        // dQ, delta
    MAS_CHECK_LAUNCH("spatial_attn_flash_bwd(dq)");
    hipLaunchKernelGGL(spatial_attn_flash_bwd_dkv_kernel, grid, dim3(SNT), (size_t)L.total, s, p);       // dK, dV (reads delta)
    MAS_CHECK_LAUNCH("spatial_attn_flash_bwd(dkv)");
    return MAS_OK;
}
