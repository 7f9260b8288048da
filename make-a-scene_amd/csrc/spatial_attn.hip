// Single-head spatial self-attention core of AttnBlock for gfx950 (reference models/modules.py:174-187: w = softmax_keys(q^T k * C^-1/2),
// h = v w^T over the h*w tokens of one image), forward and backward, bf16 storage / fp32 accumulate.
// Replaces the two torch.bmm + softmax (and, backward, four bmm + the softmax gradient) of round 1 -- ~60 small library launches
// per VQ-IMG step -- by 1 forward + 2 backward launches per AttnBlock.  S = h*w <= 256 tokens, C <= 512 channels (the reference's
// blocks are 16x16x512 for VQ-IMG, 8x8x512 for VQ-SEG), so one 32-token block's whole score row fits LDS and no online softmax is
// needed.  q, k, v are read in place from the fused [N, S, 3C] projection (q | k | v on the channel axis).
//
// Every kernel is built from two tile products (8 waves = two per SIMD since the end of round 4, NW below; MFMA 32x32x16 bf16):
//   prod : T[32 rows][S]   = X_blk[32][C] . Y_all[S][C]^T     (contraction over channels: both operands channel-contiguous, so
//                             Y rows stream straight from global memory as MFMA A fragments, X_blk rows come from LDS; T STAYS IN
//                             THE ACCUMULATORS: wave w holds column tile w (tiles w and w+4 with 4 waves), a lane 16 (32) columns of one row)
//   apply: O[32 rows][C]   = P[32][S] . M_all[S][C]           (contraction over tokens: M tiles are staged in their natural
//                             [token][channel] layout and read with the LDS transpose read ds_read_b64_tr_b16 -- per-lane
//                             addressing as in conv_wgrad.hip -- P rows (bf16) come from LDS)
//   forward        : T = prod(Q_blk, K); P = softmax(scale T), lse;  O_blk  = apply(P, V)
//   backward, dQ   : P = exp(scale prod(Q_blk, K) - lse); dP = prod(dO_blk, V); delta = rowsum(P dP); dS = scale P (dP - delta);
//                    dQ_blk = apply(dS, K)
//   backward, dK/dV: the same with the roles of queries and keys swapped (block = 32 KEYS, columns = queries, lse / delta indexed
//                    by column): dV_blk = apply(P^T, dO), dK_blk = apply(dS^T, Q).
// With 256 work-groups of 4 waves the kernels are bound by exposed memory round trips (1.2 us each, measured with wall-clock stamps at
// the phase boundaries), not by MFMA (2 us per work-group) or bandwidth: round 4 keeps 16-32 KiB per wave in flight (prod: next 256-channel step prefetched,
// apply: M tiles four ahead and issued before the softmax) and does the softmax / dS arithmetic on the accumulators instead of
// bouncing fp32 scores through LDS row by row: forward 58 -> 23 us, backward 72 + 95 -> 31 + 43 us (profiles/r04_spatial_attn.txt).
// No atomics: every output element is written exactly once (deterministic).
#include "mas_lds.h"
#include <math.h>

#include "spatial_attn_core.h"

namespace {

// LDS map (bytes); row strides padded so that 32 consecutive rows do not share banks.  The scores never touch LDS in fp32 (round 4):
// they stay in the MFMA accumulators through the softmax / dS arithmetic, only the bf16 P / dS operand of the second product is staged.
struct SpLds {
    int RX;      // X_blk row stride: roundup(C,128)*2 + 16 (channels [C, roundup(C,128)) are zero: the products run whole 128-channel groups)
    int SP;      // P / dS row stride: roundup(S,32)*2 + 16
    int RM;      // M tile row stride: C*2 + 64 (the transpose read wants 4 consecutive rows x 64 B to tile a 256-byte bank row)
    int o_x, o_p, o_p2, o_m0, o_m1, o_r, total;
    __host__ __device__ SpLds(int S, int C) {
        const int Sp = (S + 31) & ~31;           // the products write whole 32-column tiles
        RX = ((C + 127) & ~127) * 2 + 16; SP = Sp * 2 + 16; RM = C * 2 + 64;
        o_x = 0; o_p = o_x + 32 * RX; o_p2 = o_p + 32 * SP; o_m0 = o_p2 + 32 * SP; o_m1 = o_m0 + 32 * RM; o_r = o_m1 + 32 * RM;
        total = o_r + 2 * NW * 32 * 4;           // two [waves][32 rows] fp32 reduction pads
    }
};

// ---- forward: one work-group per (image, 32-query block) -----------------------------------------------------------------------
__global__ __launch_bounds__(SNT) void spatial_attn_fwd_kernel(SpParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const SpLds L(p.S, p.C);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 5, l31 = lane & 31;
    const int nqb = (p.S + 31) / 32;
    const int blk = sp_logical_block((int)gridDim.x);
    const int n = blk / nqb, q0 = (blk % nqb) * 32;
    const int ld = 3 * p.C;
    const bf16_t* Q = p.qkv + (size_t)n * p.S * ld;
    const bf16_t* K = Q + p.C;
    const bf16_t* V = Q + 2 * p.C;
    float* pad = reinterpret_cast<float*>(smem + L.o_r);

    const int rot = blk % nqb;
    int mt[TPW];
    sp_tiles(mt, wave, p.S, rot);
    f32x16 sc[TPW];
    sp_prod(sc, mt, rot, smem + L.o_x, L.RX, Q, ld, q0, K, ld, p.S, p.C, tid);
    u32x4 pf[4][UPT];
    sp_apply_issue(pf, V, ld, p.S, p.C, rot, tid);                 // four V tiles travel while the softmax runs
    // softmax over keys, in the accumulators: lane (g, l31) holds 32 of query l31's scores
    float mx = -1e30f;
#pragma unroll
    for (int ti = 0; ti < TPW; ++ti)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            if (sp_col(mt, ti, r, g) < p.S) mx = fmaxf(mx, sc[ti][r] * p.scale);
    mx = sp_row_reduce<true>(mx, pad, wave, g, l31);
    float sum = 0.0f;
#pragma unroll
    for (int ti = 0; ti < TPW; ++ti)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float e = sp_col(mt, ti, r, g) < p.S ? __expf(sc[ti][r] * p.scale - mx) : 0.0f;
            sc[ti][r] = e;
            sum += e;
        }
    sum = sp_row_reduce<false>(sum, pad + NW * 32, wave, g, l31);
    const float inv = 1.0f / sum;
#pragma unroll
    for (int ti = 0; ti < TPW; ++ti)
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[ti][r] *= inv;
    sp_put_rows(smem + L.o_p, L.SP, sc, p.S, mt, g, l31);
    if (wave == 0 && g == 0 && q0 + l31 < p.S && p.lse) p.lse[(size_t)n * p.S + q0 + l31] = mx + __logf(sum);
    f32x16 acc[CPW];
    sp_apply_run(acc, pf, smem + L.o_p, L.SP, smem + L.o_m0, smem + L.o_m1, L.RM, V, ld, p.S, p.C, rot, tid);
    sp_store(acc, p.out + (size_t)n * p.S * p.C, p.C, q0, p.S, p.C, tid);
}

// ---- backward, shared body.  KEYS = false: block = 32 queries -> dQ (and delta); KEYS = true: block = 32 keys -> dK, dV ---------
template <bool KEYS>
__global__ __launch_bounds__(SNT) void spatial_attn_bwd_kernel(SpParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const SpLds L(p.S, p.C);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6), g = lane >> 5, l31 = lane & 31;
    const int nb = (p.S + 31) / 32;
    const int blk = sp_logical_block((int)gridDim.x);
    const int n = blk / nb, r0 = (blk % nb) * 32;
    const int ld = 3 * p.C;
    const bf16_t* Q = p.qkv + (size_t)n * p.S * ld;
    const bf16_t* K = Q + p.C;
    const bf16_t* V = Q + 2 * p.C;
    const bf16_t* dO = p.dout + (size_t)n * p.S * p.C;
    const float* lse = p.lse + (size_t)n * p.S;
    float* delta = p.delta + (size_t)n * p.S;
    float* pad = reinterpret_cast<float*>(smem + L.o_r);
    const bool row_ok = r0 + l31 < p.S;

    // ---- P (block rows x all columns): rows = queries (KEYS = false) or keys (KEYS = true); lse belongs to the QUERY
    const int rot = blk % nb;
    int mt[TPW];
    sp_tiles(mt, wave, p.S, rot);
    f32x16 pv[TPW], dp[TPW];
    sp_prod(pv, mt, rot, smem + L.o_x, L.RX, KEYS ? K : Q, ld, r0, KEYS ? Q : K, ld, p.S, p.C, tid);
    const float lrow = (!KEYS && row_ok) ? lse[r0 + l31] : 0.0f;
#pragma unroll
    for (int ti = 0; ti < TPW; ++ti)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = sp_col(mt, ti, r, g);
            const float l = KEYS ? lse[min(m, p.S - 1)] : lrow;
            pv[ti][r] = (row_ok && m < p.S) ? __expf(pv[ti][r] * p.scale - l) : 0.0f;
        }
    if constexpr (KEYS) sp_put_rows(smem + L.o_p, L.SP, pv, p.S, mt, g, l31);         // dV = P^T dO wants P itself
    // ---- dP: prod(dO_blk, V) (queries) or prod(V_blk, dO) (keys)
    sp_prod(dp, mt, rot + 2, smem + L.o_x, L.RX, KEYS ? V : dO, KEYS ? ld : p.C, r0, KEYS ? dO : V, KEYS ? p.C : ld, p.S, p.C, tid);
    u32x4 pf[4][UPT];
    if constexpr (!KEYS) sp_apply_issue(pf, K, ld, p.S, p.C, rot, tid);               // K tiles travel under the delta / dS arithmetic
    float drow = 0.0f;
    if constexpr (!KEYS) {                        // delta_q = sum_keys P dP  (= sum_c dO O), published for the dK/dV kernel
        float part = 0.0f;
#pragma unroll
        for (int ti = 0; ti < TPW; ++ti)
#pragma unroll
            for (int r = 0; r < 16; ++r) part += pv[ti][r] * dp[ti][r];
        drow = sp_row_reduce<false>(part, pad, wave, g, l31);
        if (wave == 0 && g == 0 && row_ok) delta[r0 + l31] = drow;
    }
#pragma unroll
    for (int ti = 0; ti < TPW; ++ti)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int m = sp_col(mt, ti, r, g);
            float d = drow;
            if constexpr (KEYS) d = delta[min(m, p.S - 1)];
            dp[ti][r] = p.scale * pv[ti][r] * (dp[ti][r] - d);         // dS (pv is 0 outside the valid rows / columns)
        }
    if constexpr (KEYS) sp_apply_issue(pf, dO, p.C, p.S, p.C, rot, tid);              // (after the delta loads: nothing waits behind them)
    sp_put_rows(smem + L.o_p2, L.SP, dp, p.S, mt, g, l31);
    f32x16 acc[CPW];
    if constexpr (!KEYS) {
        sp_apply_run(acc, pf, smem + L.o_p2, L.SP, smem + L.o_m0, smem + L.o_m1, L.RM, K, ld, p.S, p.C, rot, tid); // dQ = dS K
        sp_store(acc, p.dqkv + (size_t)n * p.S * ld, ld, r0, p.S, p.C, tid);
    } else {
        sp_apply_run(acc, pf, smem + L.o_p, L.SP, smem + L.o_m0, smem + L.o_m1, L.RM, dO, p.C, p.S, p.C, rot, tid); // dV = P^T dO
        sp_apply_issue(pf, Q, ld, p.S, p.C, rot, tid);                                                              // (Q tiles travel under the store)
        sp_store(acc, p.dqkv + (size_t)n * p.S * ld + 2 * p.C, ld, r0, p.S, p.C, tid);
        sp_apply_run(acc, pf, smem + L.o_p2, L.SP, smem + L.o_m0, smem + L.o_m1, L.RM, Q, ld, p.S, p.C, rot, tid); // dK = dS^T Q
        sp_store(acc, p.dqkv + (size_t)n * p.S * ld + p.C, ld, r0, p.S, p.C, tid);
    }
}

int sp_check(const char* what, const void* a, const void* b, int dtype, int N, int S, int C) {
    if (!a || !b) MAS_FAIL(MAS_EINVAL, "%s: null argument", what);
    if (dtype != MAS_BF16) MAS_FAIL(MAS_EUNSUPPORTED, "%s: bf16 only (the fp32 parity mode keeps the library GEMM path)", what);
    if (N <= 0 || S <= 0 || S > S_MAX || C <= 0 || C > C_MAX || (C % 32)) MAS_FAIL(MAS_EUNSUPPORTED, "%s: needs S <= %d tokens and C %% 32 == 0, C <= %d (got S=%d C=%d)", what, S_MAX, C_MAX, S, C);
    return MAS_OK;
}

}  // namespace

extern "C" int mas_spatial_attn_fwd(const void* qkv, void* out, float* lse, int dtype, int N, int S, int C, void* stream) {
    MAS_ENTER();
    if (int rc = sp_check("spatial_attn_fwd", qkv, out, dtype, N, S, C)) return rc;
    SpParams p{};
    p.qkv = (const bf16_t*)qkv; p.out = (bf16_t*)out; p.lse = lse; p.N = N; p.S = S; p.C = C; p.scale = 1.0f / sqrtf((float)C);
    const SpLds L(S, C);
    static mas_devmask_t mask{0};
    if (int rc = sp_set_lds(spatial_attn_fwd_kernel, L.total, "spatial_attn_fwd", mask)) return rc;
    hipLaunchKernelGGL(spatial_attn_fwd_kernel, dim3((unsigned)(N * ((S + 31) / 32))), dim3(SNT), (size_t)L.total, reinterpret_cast<hipStream_t>(stream), p);
    MAS_CHECK_LAUNCH("spatial_attn_fwd");
    return MAS_OK;
}

extern "C" int mas_spatial_attn_bwd(const void* qkv, const void* dout, const float* lse, float* delta, void* dqkv, int dtype, int N, int S,
                                    int C, void* stream) {
    MAS_ENTER();
    if (int rc = sp_check("spatial_attn_bwd", qkv, dout, dtype, N, S, C)) return rc;
    if (!lse || !delta || !dqkv) MAS_FAIL(MAS_EINVAL, "spatial_attn_bwd: null argument");
    SpParams p{};
    p.qkv = (const bf16_t*)qkv; p.dout = (const bf16_t*)dout; p.dqkv = (bf16_t*)dqkv; p.lse = const_cast<float*>(lse); p.delta = delta;
    p.N = N; p.S = S; p.C = C; p.scale = 1.0f / sqrtf((float)C);
    const SpLds L(S, C);
    static mas_devmask_t m0{0}, m1{0};
    if (int rc = sp_set_lds(spatial_attn_bwd_kernel<false>, L.total, "spatial_attn_bwd", m0)) return rc;
    if (int rc = sp_set_lds(spatial_attn_bwd_kernel<true>, L.total, "spatial_attn_bwd", m1)) return rc;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)(N * ((S + 31) / 32)));
    hipLaunchKernelGGL(spatial_attn_bwd_kernel<false>, grid, dim3(SNT), (size_t)L.total, s, p);      // dQ, delta
    MAS_CHECK_LAUNCH("spatial_attn_bwd(dq)");
    hipLaunchKernelGGL(spatial_attn_bwd_kernel<true>, grid, dim3(SNT), (size_t)L.total, s, p);       // dK, dV (reads delta)
    MAS_CHECK_LAUNCH("spatial_attn_bwd(dkv)");
    return MAS_OK;
}
