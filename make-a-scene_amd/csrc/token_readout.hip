// Stage-2 validation read-out for gfx950: what a stage-2 run is judged by, from ONE read of each logits row in its own dtype
//   * token_readout            : per row nll = (m - x_t) + log l, entropy = log l - (sum_j e_j d_j) / l with d_j = x_j - m, e_j = exp(d_j),
//                                argmax = the FIRST index of the maximum, rank = #{j : x_j > x_t} + #{j < t : x_j == x_t}
//   * token_readout_accumulate : per position p = r % L the fp64 sums of nll and entropy in increasing r, counts, top-k hits; the rank
//                                histogram and the number of invalid rows.  Everything is ADDED to device accumulators.
// Logits are addressed as in token_loss.hip: row r starts at base + (r / inner) * outer_stride + (r % inner) * ld.  One work-group of 256
// lanes per row.  A 16-byte aligned row of at most 4 16-byte units per lane (8192 bf16, 4096 fp32) stays in registers: the first pass over
// the registers finds the maximum (and per lane the first unit that holds it) and x_t; one work-group exchange; the second pass over the
// same registers forms the two sums and the rank count, the latter as lane-mask population counts on the scalar unit.  A NaN is found
// through l (exp keeps it), +inf and a row of -inf through m.  Longer rows and rows that are not 16-byte aligned stream: a lane keeps an
// online (m, l, a = sum e d), rescaled when its maximum moves, the lanes are merged in a fixed order, and the rank count is a second walk
// over the row (16 .. 64 KB, read a moment ago by the same work-group: it comes from L2).
// x_t is picked by comparing the running column with t: no load is indexed by a target value.  No atomics in token_readout; integer
// atomics only (exact in any order) for the two global tallies of token_readout_accumulate.
// The row walk's parts (Unit, cvt_unit, row_ptr, the row plan, the exchange of maxima, the wave reductions) are token_loss.hip's, from
// token_row_core.h; the loops over them are this kernel's own.
#include "token_row_core.h"
#include <float.h>
#include <limits.h>

namespace {

// second pass, one element against the row's maximum M: l += e, a += e d with d = x - M, e = exp(d).  An entry of -inf has e = 0 and its d
// is clamped to -FLT_MAX inside the product, so 0 * inf is never formed; a NaN keeps e = NaN and poisons l, which is how the row is found.
__device__ __forceinline__ void sum_elem(float v, float M, float& l, float& a) {
    const float d = v - M;
    const float e = __expf(d);
    l += e;
    a = fmaf(e, fmaxf(d, -FLT_MAX), a);
}

// One unit of the rank count: `gt` and `eq` are wave totals (read from lane 0), `own` is this lane's share of the target's own unit.
// before = the whole unit lies in front of column t; here = it holds column t, at element te.
template <int N>
__device__ __forceinline__ void rank_unit(const float (&v)[N], bool before, bool here, int te, float xt, int& gt, int& eq, int& own) {
#pragma unroll
    for (int e = 0; e < N; ++e) {
        gt += wave_count(v[e] > xt);
        eq += wave_count(before && v[e] == xt);
    }
    if (here) {
#pragma unroll
        for (int e = 0; e < N; ++e) own += (e < te && v[e] == xt) ? 1 : 0;
    }
}

template <typename T>
__global__ __launch_bounds__(NT) void token_readout_kernel(const T* __restrict__ x, long long rows, int V, long long inner,
                                                           long long outer_stride, long long ld, const long long* __restrict__ target,
                                                           long long ignore_index, float* __restrict__ nll, float* __restrict__ entropy,
                                                           int* __restrict__ argmax, int* __restrict__ rank) {
    constexpr int N = Unit<T>::N;
    __shared__ float s_max[NW];
    __shared__ float s_xt;
    __shared__ float s_l[NW], s_a[NW];
    __shared__ int s_cnt[NW], s_arg[NW];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (long long r = blockIdx.x; r < rows; r += gridDim.x) {
        const long long t = target[r];
        if (t == ignore_index || t < 0 || t >= (long long)V) {  // (uniform over the work-group) the row is not read
            if (tid == 0) {
                const bool ign = t == ignore_index;
                nll[r] = entropy[r] = ign ? 0.0f : __builtin_nanf("");
                argmax[r] = -1;
                rank[r] = ign ? -1 : V;
            }
            continue;
        }
        const auto [xr, nfull, e0] = row_plan(x, r, V, inner, outer_stride, ld);
        const int tc = (int)t;
        const int tu = tc < e0 ? tc / N : -1, te = tc % N;       // the unit that holds column t and the element inside it (no unit: the tail)
        const bool resident = nfull <= KMAX * NT && V - e0 <= NT;   // token_loss.hip spells the same test (token_row_core.h)
        float mx = -INFINITY, xt = 0.0f;
        int mcol = INT_MAX;                                      // where this lane first met its maximum: a unit's first column, or a tail column
        bool munit = false;                                      // ... and which of the two
        u32x4 raw[KMAX];                                        // resident rows: as loaded, 4 VGPRs per unit, converted at each use
        float vt = 0.0f;
        const bool has_t = tid < V - e0;                         // (resident rows) this lane's tail element
        float li = 0.0f, ai = 0.0f;                              // streaming rows: this lane's online sums against its own maximum mx
        // pass 1: the maximum (per unit, and the first unit that holds it) and x_t.  A lane meets its columns in increasing order and moves on
        // `>` only, so what it remembers is its first maximum.  fmaxf drops a NaN; a row with one is found through l below.
        if (resident) {
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                const int u = k * NT + tid;
                if (u < nfull) {
                    raw[k] = *reinterpret_cast<const u32x4*>(xr + (size_t)u * N);
                    float v[N];
                    cvt_unit<T, N>(raw[k], v);
                    const float um = unit_max(v);
                    if (um > mx) { mx = um; mcol = u * N; munit = true; }
                    if (u == tu) {
#pragma unroll
                        for (int e = 0; e < N; ++e) if (e == te) xt = v[e];
                    }
                }
            }
            if (has_t) {
                vt = (float)xr[e0 + tid];
                if (vt > mx) { mx = vt; mcol = e0 + tid; munit = false; }
                if (e0 + tid == tc) xt = vt;
            }
        } else {
#pragma unroll 1
            for (int u = tid; u < nfull; u += NT) {
                float v[N];
                cvt_unit<T, N>(*reinterpret_cast<const u32x4*>(xr + (size_t)u * N), v);
                const float um = unit_max(v);
                if (u == tu) {
#pragma unroll
                    for (int e = 0; e < N; ++e) if (e == te) xt = v[e];
                }
                if (um > mx) {       // the lane's maximum moves: rescale what it holds (f = 0 from mx = -inf); token_loss.hip's step for (m, l)
                    const float f = __expf(mx - um);
                    ai = f > 0.0f ? f * (ai + (mx - um) * li) : 0.0f;
                    li *= f;
                    mx = um; mcol = u * N; munit = true;
                }
                const float ms = exp_shift(mx);
#pragma unroll
                for (int e = 0; e < N; ++e) sum_elem(v[e], ms, li, ai);
            }
#pragma unroll 1
            for (int j = e0 + tid; j < V; j += NT) {
                const float a = (float)xr[j];
                if (j == tc) xt = a;
                if (a > mx) {
                    const float f = __expf(mx - a);
                    ai = f > 0.0f ? f * (ai + (mx - a) * li) : 0.0f;
                    li *= f;
                    mx = a; mcol = j; munit = false;
                }
                sum_elem(a, exp_shift(mx), li, ai);
            }
        }
        // exchange 1: the row's maximum and x_t (the one lane that met column t writes it)
        if ((tc < e0 ? tc / N : tc - e0) % NT == tid) s_xt = xt;  // unit u and tail element e0 + j belong to lanes u % 256 and j % 256
        const float M = row_max(mx, s_max, lane, wave);
        const float XT = s_xt;
        // the first index of the maximum: a lane whose maximum is the row's looks for the element inside the unit it remembered (its first
        // unit with that value: units and tail come in increasing columns within a lane); the smallest such column wins in exchange 2
        int acol = INT_MAX;
        if (mx == M) {
            acol = mcol;
            if (munit) {
                float v[N];
                if (resident) {
                    u32x4 w = raw[0];
#pragma unroll
                    for (int k = 1; k < KMAX; ++k) if ((k * NT + tid) * N == mcol) w = raw[k];
                    cvt_unit<T, N>(w, v);
                } else {
                    cvt_unit<T, N>(*reinterpret_cast<const u32x4*>(xr + mcol), v);
                }
                int fe = N - 1;
#pragma unroll
                for (int e = N - 2; e >= 0; --e) if (v[e] == M) fe = e;
                acol = mcol + fe;
            }
        }
        // pass 2: the sums against M and the rank count
        float l = 0.0f, a = 0.0f;
        int gt = 0, eq = 0, own = 0;
        if (resident) {
#pragma unroll
            for (int k = 0; k < KMAX; ++k) {
                const int u = k * NT + tid;
                if (u < nfull) {
                    float v[N];
                    cvt_unit<T, N>(raw[k], v);
#pragma unroll
                    for (int e = 0; e < N; ++e) sum_elem(v[e], M, l, a);
                    rank_unit<N>(v, tu < 0 || u < tu, u == tu, te, XT, gt, eq, own);
                }
            }
            if (has_t) {
                sum_elem(vt, M, l, a);
                gt += wave_count(vt > XT);
                eq += wave_count(vt == XT && e0 + tid < tc);
            }
        } else {
            const float f = __expf(mx - M);                      // (mx == M: exp(0) = 1 exactly; a lane without elements: mx = -inf, f = 0)
            l = li * f;
            a = f > 0.0f ? f * (ai + (mx - M) * li) : 0.0f;
            // the second walk: the row comes from L2
#pragma unroll 1
            for (int u = tid; u < nfull; u += NT) {
                float v[N];
                cvt_unit<T, N>(*reinterpret_cast<const u32x4*>(xr + (size_t)u * N), v);
                rank_unit<N>(v, tu < 0 || u < tu, u == tu, te, XT, gt, eq, own);
            }
#pragma unroll 1
            for (int j = e0 + tid; j < V; j += NT) {
                const float b = (float)xr[j];
                gt += wave_count(b > XT);
                eq += wave_count(b == XT && j < tc);
            }
        }
        l = wave_sum(l); a = wave_sum(a);
        const int cnt = gt + eq + wave_sum(own);                 // (lane 0's gt and eq are the wave's totals)
        acol = wave_min(acol);
        if (lane == 0) { s_l[wave] = l; s_a[wave] = a; s_cnt[wave] = cnt; s_arg[wave] = acol; }
        __syncthreads();
        if (tid == 0) {
            const float Ls = (s_l[0] + s_l[1]) + (s_l[2] + s_l[3]);
            // invalid: +inf in the row (M = +inf), -inf alone (M = -inf), a NaN (it went through exp into l)
            if (!(M > -INFINITY && M < INFINITY) || Ls != Ls) {
                nll[r] = entropy[r] = __builtin_nanf("");
                argmax[r] = -1;
                rank[r] = V;
            } else {
                const float As = (s_a[0] + s_a[1]) + (s_a[2] + s_a[3]);
                const float logl = logf(Ls);
                nll[r] = (M - XT) + logl;                        // {m, log l} stay apart
                entropy[r] = logl - As / Ls;
                argmax[r] = min(min(s_arg[0], s_arg[1]), min(s_arg[2], s_arg[3]));
                rank[r] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
            }
        }
        __syncthreads();                                          // the shared words are reused by the next row
    }
}

struct Thresholds { int k[MAS_TOKEN_MAX_KS]; };

// One lane per position p: rows p, p + L, ... in increasing order, fp64 from the first addition, then ONE addition to the held sums.  The
// rank histogram and the invalid count are integers: an LDS histogram per work-group, then 64-bit integer atomics (exact in any order).
__global__ __launch_bounds__(NT) void token_readout_accumulate_kernel(const float* __restrict__ nll, const float* __restrict__ entropy,
                                                                      const int* __restrict__ argmax, const int* __restrict__ rank,
                                                                      const long long* __restrict__ target, long long rows,
                                                                      long long ignore_index, long long L, Thresholds ks, int nk,
                                                                      double* __restrict__ nll_sum, double* __restrict__ entropy_sum,
                                                                      long long* __restrict__ count, long long* __restrict__ hits,
                                                                      long long* __restrict__ rank_hist, long long* __restrict__ invalid) {
    __shared__ unsigned s_hist[MAS_TOKEN_RANK_BINS + 1];         // the last word: invalid rows
    const int tid = threadIdx.x;
    if (tid <= MAS_TOKEN_RANK_BINS) s_hist[tid] = 0u;
    __syncthreads();
    const long long p = (long long)blockIdx.x * NT + tid;
    if (p < L) {
        double sn = 0.0, se = 0.0;
        long long c = 0;
        long long h[MAS_TOKEN_MAX_KS];
#pragma unroll
        for (int i = 0; i < MAS_TOKEN_MAX_KS; ++i) h[i] = 0;
        for (long long r = p; r < rows; r += L) {
            if (target[r] == ignore_index) continue;
            if (argmax[r] < 0) { atomicAdd(&s_hist[MAS_TOKEN_RANK_BINS], 1u); continue; }
            sn += (double)nll[r];
            se += (double)entropy[r];
            c += 1;
            const int rk = rank[r];
#pragma unroll
            for (int i = 0; i < MAS_TOKEN_MAX_KS; ++i) h[i] += (i < nk && rk < ks.k[i]) ? 1 : 0;
            atomicAdd(&s_hist[rk <= 0 ? 0 : 32 - __clz(rk)], 1u);
        }
        nll_sum[p] += sn;
        entropy_sum[p] += se;
        count[p] += c;
#pragma unroll
        for (int i = 0; i < MAS_TOKEN_MAX_KS; ++i)
            if (i < nk) hits[p * nk + i] += h[i];
    }
    __syncthreads();
    if (tid <= MAS_TOKEN_RANK_BINS && s_hist[tid]) {
        unsigned long long* dst = reinterpret_cast<unsigned long long*>(tid < MAS_TOKEN_RANK_BINS ? rank_hist + tid : invalid);
        atomicAdd(dst, (unsigned long long)s_hist[tid]);
    }
}

}  // namespace

extern "C" int mas_token_readout(const void* logits, int dtype, long long rows, int V, long long inner, long long outer_stride, long long ld,
                                 const int64_t* target, long long ignore_index, float* nll, float* entropy, int32_t* argmax, int32_t* rank,
                                 void* stream) {
    MAS_ENTER();
    if (int rc = row_check("token_readout", logits, dtype, rows, V, inner, outer_stride, ld, target, 0.0f)) return rc;
    if (!nll || !entropy || !argmax || !rank) MAS_FAIL(MAS_EINVAL, "token_readout: null argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid(row_grid(rows)), block(NT);
    const long long* tg = reinterpret_cast<const long long*>(target);
    if (dtype == MAS_BF16)
        hipLaunchKernelGGL((token_readout_kernel<bf16_t>), grid, block, 0, s, (const bf16_t*)logits, rows, V, inner, outer_stride, ld, tg,
                           ignore_index, nll, entropy, argmax, rank);
    else
        hipLaunchKernelGGL((token_readout_kernel<float>), grid, block, 0, s, (const float*)logits, rows, V, inner, outer_stride, ld, tg,
                           ignore_index, nll, entropy, argmax, rank);
    MAS_CHECK_LAUNCH("token_readout");
    return MAS_OK;
}

extern "C" int mas_token_readout_accumulate(const float* nll, const float* entropy, const int32_t* argmax, const int32_t* rank,
                                            const int64_t* target, long long rows, long long ignore_index, long long L, const int* ks,
                                            int nk, double* nll_sum, double* entropy_sum, long long* count, long long* hits,
                                            long long* rank_hist, long long* invalid, void* stream) {
    MAS_ENTER();
    if (rows <= 0 || L <= 0) MAS_FAIL(MAS_EINVAL, "token_readout_accumulate: rows=%lld L=%lld must be positive", rows, L);
    if (rows % L != 0) MAS_FAIL(MAS_EINVAL, "token_readout_accumulate: rows=%lld is not a multiple of the L=%lld positions", rows, L);
    if (nk < 0 || nk > MAS_TOKEN_MAX_KS)
        MAS_FAIL(MAS_EINVAL, "token_readout_accumulate: nk=%d thresholds (0 .. %d)", nk, (int)MAS_TOKEN_MAX_KS);
    if (nk > 0 && !ks) MAS_FAIL(MAS_EINVAL, "token_readout_accumulate: null argument (ks)");
    Thresholds th;
    for (int i = 0; i < MAS_TOKEN_MAX_KS; ++i) th.k[i] = 1;
    for (int i = 0; i < nk; ++i) {
        if (ks[i] < 1) MAS_FAIL(MAS_EINVAL, "token_readout_accumulate: threshold ks[%d]=%d must be at least 1", i, ks[i]);
        th.k[i] = ks[i];
    }
    if (L > (1LL << 31) * NT - NT) MAS_FAIL(MAS_EUNSUPPORTED, "token_readout_accumulate: L=%lld positions", L);
    if (!nll || !entropy || !argmax || !rank || !target || !nll_sum || !entropy_sum || !count || (nk > 0 && !hits) || !rank_hist || !invalid)
        MAS_FAIL(MAS_EINVAL, "token_readout_accumulate: null argument");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const dim3 grid((unsigned)((L + NT - 1) / NT)), block(NT);
    hipLaunchKernelGGL(token_readout_accumulate_kernel, grid, block, 0, s, nll, entropy, argmax, rank,
                       reinterpret_cast<const long long*>(target), rows, ignore_index, L, th, nk, nll_sum, entropy_sum, count, hits,
                       rank_hist, invalid);
    MAS_CHECK_LAUNCH("token_readout_accumulate");
    return MAS_OK;
}
