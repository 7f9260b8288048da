// Device code shared by the spatial-attention kernels (spatial_attn.hip: S <= 256, the whole score row in LDS; spatial_attn_flash.hip:
// online softmax over 256-key chunks): the two tile products, the fragment ring, the row staging, the XCD-aware block order.
// The header comment of spatial_attn.hip explains the scheme; per-file build flags apply to this code as to the rest of the
// translation unit that includes it.
#pragma once
#include "mas_lds.h"
#include <math.h>

namespace {

constexpr int NW = 8;                           // waves per work-group: two per SIMD (the A/B against 4: profiles/r04_spatial_attn.txt, section 8)
constexpr int SNT = 64 * NW;
constexpr int S_MAX = 256, C_MAX = 512;
constexpr int TPW = S_MAX / 32 / NW;            // 32-column score tiles per wave
constexpr int CPW = C_MAX / 32 / NW;            // 32-channel output tiles per wave
constexpr int UPT = 32 * (C_MAX / 8) / SNT;     // 16-byte units of a 32-row tile per thread

struct SpParams {
    const bf16_t* qkv; const bf16_t* o; const bf16_t* dout; bf16_t* out; bf16_t* dqkv; float* lse; float* delta;
    int N, S, C;
    float scale;
};

// 32 rows [r0, r0+32) of a [rows][ld] bf16 matrix (channel window [0, C)), <= 8 16-byte units per thread: global -> registers ...
// BRANCH-FREE on purpose: a load inside a conditional block makes the number of younger loads unknown to the compiler's wait-count
// pass, and every later wait becomes vmcnt(0) -- which silently serialises a prefetch pipeline (all 62 waits of the first version of
// this kernel were vmcnt(0)).  Out-of-range units / rows read a clamped, valid address; sp_rows_commit zeroes the rows >= S, and a
// clamped unit just rewrites the last real unit with the same bytes.
// (unit -> (row, 16-byte column) without a division per unit: at one wave per SIMD the address VALU work is not hidden by anything,
//  and tid + 256 k divided by a runtime C / 8, twice per tile, was a third of the apply loop)
struct SpMap {
    int r, cu, dr, dc, upr;
    __device__ __forceinline__ SpMap(int C, int tid) { upr = C / 8; r = tid / upr; cu = tid - r * upr; dr = SNT / upr; dc = SNT - dr * upr; }
};
__device__ __forceinline__ void sp_rows_fetch(u32x4 (&pf)[UPT], const bf16_t* src, int ld, int r0, int S, const SpMap& mp) {
    int r = mp.r, cu = mp.cu;
#pragma unroll
    for (int k = 0; k < UPT; ++k) {
        const int rr = min(r, 31), cc = r > 31 ? mp.upr - 1 : cu;          // units past the tile re-read its last unit
        pf[k] = *reinterpret_cast<const u32x4*>(src + (size_t)min(r0 + rr, S - 1) * ld + cc * 8);
        cu += mp.dc; r += mp.dr;
        if (cu >= mp.upr) { cu -= mp.upr; ++r; }
    }
}
// ... -> LDS with row stride RS (rows >= S are zero)
__device__ __forceinline__ void sp_rows_commit(const u32x4 (&pf)[UPT], unsigned char* dst, int RS, int r0, int S, const SpMap& mp) {
    int r = mp.r, cu = mp.cu;
#pragma unroll
    for (int k = 0; k < UPT; ++k) {
        const int rr = min(r, 31), cc = r > 31 ? mp.upr - 1 : cu;
        const bool ok = r0 + rr < S;
        const u32x4 v = {ok ? pf[k][0] : 0u, ok ? pf[k][1] : 0u, ok ? pf[k][2] : 0u, ok ? pf[k][3] : 0u};
        *reinterpret_cast<u32x4*>(dst + rr * RS + cc * 16) = v;
        cu += mp.dc; r += mp.dr;
        if (cu >= mp.upr) { cu -= mp.upr; ++r; }
    }
}

// zero channels [C, roundup(C, 128)) of the 32 staged rows: the products run whole 128-channel groups
__device__ __forceinline__ void sp_rows_zero_pad(unsigned char* xs, int RX, int C, int tid) {
    if (C & 127) {
        const int padu = (128 - (C & 127)) / 8;
        for (int u = tid; u < 32 * padu; u += SNT) *reinterpret_cast<u32x4*>(xs + (u / padu) * RX + (C / 8 + u % padu) * 16) = u32x4{0u, 0u, 0u, 0u};
    }
}

// Which score columns a lane holds: wave w owns the 32-column tiles w and w + 4 (accumulator slots mt[0], mt[1]); register r of
// slot ti is column m = mt[ti] * 32 + (r & 3) + 8 (r >> 2) + 4 g of block row n = l31  (g = lane >> 5, l31 = lane & 31).
// The 8 work-groups of an image run on one XCD at the same time and would otherwise walk K / V in lockstep: every line would be
// requested by all 8 while the first miss is still on the fabric, and all of them would sit out the full 1.2 us on every step
// (27 GB/s per CU measured = the L1 miss queue x 128 B / that latency, with 8 CUs spending it on the SAME lines).  `rot` (the block's
// index within its image) de-phases them: odd blocks start with their upper column tile, bit 1 flips the order of the two channel
// halves (here), and the apply walks its token tiles starting at tile `rot` -- the lines one block waits for are hits for the rest.
__device__ __forceinline__ void sp_tiles(int (&mt)[TPW], int wave, int S, int rot) {
    if constexpr (TPW == 2) {
        const bool swap = (wave + 4 < (S + 31) / 32) && (rot & 1);
        mt[0] = swap ? wave + 4 : wave;
        mt[TPW - 1] = swap ? wave : wave + 4;
    } else {
        mt[0] = wave;                            // 8 waves: one column tile each
    }
}
__device__ __forceinline__ int sp_col(const int (&mt)[TPW], int ti, int r, int g) { return mt[ti] * 32 + (r & 3) + 8 * (r >> 2) + 4 * g; }

// sc[ti][r] = sum_c X[r0 + n][c] * Y[m][c]: the 32 block rows are staged into xs (LDS) by this call, the rows of Y stream straight
// from global memory as MFMA A fragments (lane = m), B operand (lane = n) from LDS; the result stays in the accumulators.
// At one wave per SIMD nothing hides anything, so the loop is written for the two things that were found to cost (phase time stamps + the ISA):
// * memory-level parallelism: a step is 128 channels of one column tile (8 fragments, 8 KiB per wave); a ring of four fragment
//   buffers keeps THREE steps in flight behind the one being multiplied, and the first three are issued before the block rows are
//   committed to LDS, so that round trip overlaps too;
// * straight-line code: every load is unconditional (sp_rows_fetch explains why), the block rows are zero-padded to whole groups so
//   that a step has no per-fragment branch, and a step that does not exist for this wave / this C still loads (one clamped line) and
//   only skips its MFMAs under a wave-uniform branch.  The first version, with two 16-fragment buffers selected by `k & 1 ? a0 : a1`
//   and per-fragment bounds branches, compiled to 2700 v_accvgpr moves per product.
// sp_prod_t<STAGE, RING>: STAGE = false takes block rows that are ALREADY in xs (committed, zero-padded and visible: the chunked
// kernels of spatial_attn_flash.hip stage their block once and multiply it with every chunk; X, ldx, r0, Sx are then unused); Sx
// bounds the block rows, S the rows of Y.  RING fragment buffers (RING - 1 steps in flight): 4 as described above, 2 where the
// caller's live accumulators leave no room for 128 fragment registers.
template <bool STAGE, int RING = 4>
__device__ __forceinline__ void sp_prod_t(f32x16 (&sc)[TPW], const int (&mt)[TPW], int rot, unsigned char* xs, int RX, const bf16_t* X, int ldx,
                                          int r0, int Sx, const bf16_t* Y, int ld, int S, int C, int tid) {
    const int lane = tid & 63, g = lane >> 5, l31 = lane & 31;
    const int n_mt = (S + 31) / 32, n_grp = (C + 127) / 128;            // 1..4 channel groups
    const int my_tiles = (mt[0] < n_mt) + (TPW == 2 ? (mt[TPW - 1] < n_mt) : 0);      // 0, 1 or 2 (S <= 256); slot 0 is the valid one when 1
    const int gr = (rot >> 1) & 3;                                      // (the blocks of an image start on different groups)
    const SpMap mp(C, tid);
    u32x4 xr_[UPT];
    if constexpr (STAGE) sp_rows_fetch(xr_, X, ldx, r0, Sx, mp);
    bf16x8 a[RING][8];
    auto fetch = [&](bf16x8 (&f)[8], int k) {
        const int ti = k >> 2, grp = ((k & 3) + gr) & 3;
        const int m = mt[ti] < n_mt ? min(mt[ti] * 32 + l31, S - 1) : 0;          // columns >= S: a real row's bytes, masked by every consumer
        const bf16_t* yr = Y + (size_t)m * ld + 8 * g;
#pragma unroll
        for (int u = 0; u < 8; ++u) f[u] = *reinterpret_cast<const bf16x8*>(yr + min(grp * 128 + 16 * u, C - 16));
    };
#pragma unroll
    for (int k = 0; k < RING - 1; ++k) fetch(a[k], k);
    if constexpr (STAGE) {
        __syncthreads();                          // whoever read xs before is done
        sp_rows_commit(xr_, xs, RX, r0, Sx, mp);
        sp_rows_zero_pad(xs, RX, C, tid);
        __syncthreads();
    }
#pragma unroll
    for (int ti = 0; ti < TPW; ++ti)
#pragma unroll
        for (int r = 0; r < 16; ++r) sc[ti][r] = 0.0f;
    const unsigned char* xr = xs + l31 * RX + 16 * g;
#pragma unroll
    for (int k = 0; k < 4 * TPW; ++k) {
        if (k + RING - 1 < 4 * TPW) fetch(a[(k + RING - 1) % RING], k + RING - 1);
        const int grp = ((k & 3) + gr) & 3;
        if ((k >> 2) < my_tiles && grp < n_grp) {
            constexpr int UB = RING == 4 ? 8 : 4;                         // B fragments read at a time (the short ring is the low-register variant)
#pragma unroll
            for (int u0 = 0; u0 < 8; u0 += UB) {
                bf16x8 b[UB];
#pragma unroll
                for (int u = 0; u < UB; ++u) b[u] = *reinterpret_cast<const bf16x8*>(xr + (grp * 128 + 16 * (u0 + u)) * 2);
#pragma unroll
                for (int u = 0; u < UB; ++u) mma16(sc[k >> 2], a[k % RING][u0 + u], b[u]);
            }
        }
    }
}
__device__ __forceinline__ void sp_prod(f32x16 (&sc)[TPW], const int (&mt)[TPW], int rot, unsigned char* xs, int RX, const bf16_t* X, int ldx,
                                        int r0, const bf16_t* Y, int ld, int S, int C, int tid) {
    sp_prod_t<true>(sc, mt, rot, xs, RX, X, ldx, r0, S, Y, ld, S, C, tid);
}

// bf16 rows of P / dS for the second product: lane (g, l31) owns 4 consecutive columns per accumulator quad -> one 8-byte LDS write
__device__ __forceinline__ void sp_put_rows(unsigned char* ps, int SP, const f32x16 (&v)[TPW], int S, const int (&mts)[TPW], int g, int l31) {
    const int n_mt = (S + 31) / 32;
#pragma unroll
    for (int ti = 0; ti < TPW; ++ti) {
        const int mt = mts[ti];
        if (mt < n_mt) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const bf16x4 o = {(bf16_t)v[ti][4 * q], (bf16_t)v[ti][4 * q + 1], (bf16_t)v[ti][4 * q + 2], (bf16_t)v[ti][4 * q + 3]};
                *reinterpret_cast<bf16x4*>(ps + l31 * SP + (mt * 32 + 8 * q + 4 * g) * 2) = o;
            }
        }
    }
}

// row-wise reduction of one value per lane over ALL columns: the two lane halves (xor 32), then the 4 waves through an LDS pad.
template <bool MAX>
__device__ __forceinline__ float sp_row_reduce(float v, float* pad, int wave, int g, int l31) {
    const float o = __shfl_xor(v, 32);
    v = MAX ? fmaxf(v, o) : v + o;
    if (g == 0) pad[wave * 32 + l31] = v;
    __syncthreads();
    float acc = pad[l31];
#pragma unroll
    for (int w = 1; w < NW; ++w) acc = MAX ? fmaxf(acc, pad[w * 32 + l31]) : acc + pad[w * 32 + l31];
    return acc;
}

// O[n][c] = sum_s P[n][s] * M[s][c]: P (bf16 [32][S], LDS), M global [S][ld]; result acc tiles: wave w owns channel tiles
// ct = w, w+4, ... (<= 4 of them, C <= 512): acc[i][r] = D[c = ct*32 + (r&3)+8(r>>2)+4g][n = l31].
// The 32-token tiles of M go global -> registers -> LDS, FOUR tiles ahead: sp_apply_issue puts tiles 0..3 in flight (the callers do
// that before their softmax / dS arithmetic, M does not depend on it), sp_apply_run commits tile t+1 into the LDS buffer tile t-1 just
// left, re-arms its registers with tile t+4 and runs tile t's MFMAs -- one barrier per tile, and a tile's round trip (1.2 us measured)
// is spread over four tiles of work instead of being exposed 8 times (P.V phase of the forward: 11.3 -> 6.8 us).
__device__ __forceinline__ int sp_rot_tile(int t, int rot, int nt) { const int tt = t + rot; return tt >= nt ? tt - nt : tt; }   // rot < nt

// (D = the depth of that pipeline, deduced from the caller's register array: 4 as described; the dK/dV kernel of spatial_attn_flash.hip, with
//  two accumulator sets live, has room for 2)
template <int D>
__device__ __forceinline__ void sp_apply_issue(u32x4 (&pf)[D][UPT], const bf16_t* M, int ld, int S, int C, int rot, int tid) {
    const int nt = (S + 31) / 32;
    const SpMap mp(C, tid);
#pragma unroll
    for (int t = 0; t < D; ++t)
        if (t < nt) sp_rows_fetch(pf[t], M, ld, sp_rot_tile(t, rot, nt) * 32, S, mp);
}

// sp_apply_run_t<false> ADDS into acc (the chunked kernels carry O / dQ / dK / dV across their chunks).
template <bool ZERO, int D>
__device__ __forceinline__ void sp_apply_run_t(f32x16 (&acc)[CPW], u32x4 (&pf)[D][UPT], const unsigned char* ps, int SP, unsigned char* ms0,
                                               unsigned char* ms1, int RM, const bf16_t* M, int ld, int S, int C, int rot, int tid) {
    const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int g = lane >> 5, l31 = lane & 31, G16 = (lane >> 4) & 1, sl = lane & 15;
    const int n_ct = C / 32, nt = (S + 31) / 32;
    const SpMap mp(C, tid);
    if constexpr (ZERO) {
#pragma unroll
        for (int i = 0; i < CPW; ++i)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][r] = 0.0f;
    }
    __syncthreads();                              // the callers' P / dS rows are written; earlier readers of ms0 / ms1 are done
    sp_rows_commit(pf[0], ms0, RM, sp_rot_tile(0, rot, nt) * 32, S, mp);
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        if (t < nt) {
            const int s0 = sp_rot_tile(t, rot, nt) * 32;
            const unsigned char* cur = (t & 1) ? ms1 : ms0;
            __syncthreads();                      // tile t is visible; every wave has left tile t-1's buffer
            // (operands first, all of them, then the commit / re-arm traffic, then the 8 MFMAs: with the reads inside the per-channel-
            //  tile bounds branch each MFMA waited out its own LDS round trip -- 1.1 us per tile for 0.12 us of MFMA)
            bf16x8 bq[2], aq[2][CPW];
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bq[ks] = *reinterpret_cast<const bf16x8*>(ps + l31 * SP + (s0 + ks * 16 + 8 * g) * 2);     // P[n][s0 + 16 ks + 8 g ..+7]
                // transpose-read lane addressing: token (16 ks + 8 g + (sl >> 2)) (+4 for the second read), channels ct*32 + 16*G16 + 4*(sl&3) ..+3
                const unsigned char* a_lane = cur + (ks * 16 + 8 * g + (sl >> 2)) * RM + (16 * G16 + 4 * (sl & 3)) * 2;
#pragma unroll
                for (int i = 0; i < CPW; ++i) {
                    const int ct = min(wave + NW * i, n_ct - 1);         // a channel tile past C recomputes the last real one; sp_store drops it
                    aq[ks][i] = tr_frag(a_lane + ct * 64, a_lane + ct * 64 + 4 * RM);
                }
            }
            if (t + 1 < nt) sp_rows_commit(pf[(t + 1) % D], (t & 1) ? ms0 : ms1, RM, sp_rot_tile(t + 1, rot, nt) * 32, S, mp);
            if (t + D < nt) sp_rows_fetch(pf[t % D], M, ld, sp_rot_tile(t + D, rot, nt) * 32, S, mp);
#pragma unroll
            for (int ks = 0; ks < 2; ++ks)
#pragma unroll
                for (int i = 0; i < CPW; ++i) mma16(acc[i], aq[ks][i], bq[ks]);
        }
    }
    __syncthreads();                              // the last tile's reads are done: the caller may reuse both buffers
}
__device__ __forceinline__ void sp_apply_run(f32x16 (&acc)[CPW], u32x4 (&pf)[4][UPT], const unsigned char* ps, int SP, unsigned char* ms0,
                                             unsigned char* ms1, int RM, const bf16_t* M, int ld, int S, int C, int rot, int tid) {
    sp_apply_run_t<true>(acc, pf, ps, SP, ms0, ms1, RM, M, ld, S, C, rot, tid);
}

// writes acc tiles to out[n][c] (rows r0 + l31 < S), 4 consecutive channels (8 bytes) per accumulator quad
__device__ __forceinline__ void sp_store(const f32x16 (&acc)[CPW], bf16_t* out, int ld, int r0, int S, int C, int tid) {
    const int lane = tid & 63, wave = tid >> 6, g = lane >> 5, l31 = lane & 31;
    if (r0 + l31 >= S) return;
#pragma unroll
    for (int i = 0; i < CPW; ++i) {
        const int ct = wave + NW * i;
        if (ct >= C / 32) continue;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            bf16x4 o = {(bf16_t)acc[i][4 * q], (bf16_t)acc[i][4 * q + 1], (bf16_t)acc[i][4 * q + 2], (bf16_t)acc[i][4 * q + 3]};
            *reinterpret_cast<bf16x4*>(out + (size_t)(r0 + l31) * ld + ct * 32 + 8 * q + 4 * g) = o;
        }
    }
}

// Work-group -> (image, 32-row block).  The hardware deals work-groups to the 8 XCDs round-robin (id % 8), and each XCD has its own
// 4 MiB L2: with the plain id / nb decode the 8 row blocks of one image land on 8 different XCDs, every L2 sees the K and V of every
// image (32 x 512 KiB at the benched shape) and all of it streams from the fabric 8 times.  Here XCD x takes the x-th contiguous
// eighth of the (image, block) list, so the blocks that share an image's K / V run on the same L2 at the same time.
__device__ __forceinline__ int sp_logical_block(int total) {
    const int w = blockIdx.x;
    if (total % 8) return w;
    return (w % 8) * (total / 8) + w / 8;
}

template <typename K>
int sp_set_lds(K kern, int bytes, const char* what, mas_devmask_t& mask) {
    unsigned long long bit;
    if (mas_attr_needed(mask, &bit)) {
        if (hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess)
            MAS_FAIL(MAS_ELAUNCH, "%s: cannot set dynamic LDS size", what);
        mas_attr_done(mask, bit);
    }
    (void)bytes;
    return MAS_OK;
}

}  // namespace
