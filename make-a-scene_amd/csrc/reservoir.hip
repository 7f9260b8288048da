// The codebook's latent reservoir on the device (Codebook.enable_device_reservoir; reference models/modules.py:477-481 stated on sets).
// C contract and the construction: include/mas_hip.h, "Codebook reservoir".  tests/helpers/reservoir_ref.py restates it in numpy.
//
//   reservoir_plan_kernel   ONE work-group.  Reads state = {c, calls}, draws the 10 positions and the drop set from two keyed bijections,
//                           ranks the surviving candidates and the dropped old rows (block scans in LDS) and writes, per candidate,
//                           {destination slot or -1, source row of z} to `plan`.  After a barrier thread 0 stores the new {c, calls + 1}:
//                           nobody else reads the counters (mas_decode_advance is the precedent for the ordering).
//   reservoir_copy_kernel   64 lanes per candidate row, 16-byte loads and stores; reads `plan` only.
#include "mas_common.h"
#include "mas_philox.h"

#define RSV_THREADS 256

// ---- keyed bijection of [0, N): rsv_half_bits / rsv_feistel / rsv_perm live in mas_bijection.h, the one copy that kmeans.hip shares.
//      (tests/test_reservoir_cpu.py compiles the text from the declaration below to the next comment as host C++: it reaches the header.)
MAS_HD uint32_t rsv_half_bits(uint32_t N);
#include "mas_bijection.h"

// exclusive scan of one count per thread over the work-group (fixed order: thread 0 adds the 256 counts); returns the thread's offset
__device__ __forceinline__ int rsv_scan(int mine, int* s_scan) {
    __syncthreads();
    s_scan[threadIdx.x] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        int run = 0;
        for (int i = 0; i < RSV_THREADS; ++i) { const int v = s_scan[i]; s_scan[i] = run; run += v; }
    }
    __syncthreads();
    return s_scan[threadIdx.x];
}

__global__ __launch_bounds__(RSV_THREADS) void reservoir_plan_kernel(int* __restrict__ state, int* __restrict__ plan, uint32_t k0, uint32_t k1,
                                                                     int R, int B, int HW) {
    __shared__ int s_drop[MAS_RESERVOIR_MAX_CANDIDATES];      // candidate i is dropped
    __shared__ int s_old[MAS_RESERVOIR_MAX_CANDIDATES];       // draw t: the old slot it drops, or -1
    __shared__ int s_list[MAS_RESERVOIR_MAX_CANDIDATES];      // the dropped old slots in draw order
    __shared__ int s_pos[MAS_RESERVOIR_PER_IMAGE];
    __shared__ int s_scan[RSV_THREADS];
    const int tid = threadIdx.x, n = MAS_RESERVOIR_PER_IMAGE * B;
    const int c = state[0];
    const uint32_t calls = (uint32_t)state[1];
    if (c < 0 || c > R) {                                     // not a state this kernel wrote: hold nothing new, leave it as it is
        for (int i = tid; i < n; i += RSV_THREADS) { plan[2 * i] = -1; plan[2 * i + 1] = 0; }
        return;
    }
    const int m = c + n, d = m > R ? m - R : 0, free_slots = R - c;      // d <= n;  free_slots = n - d when d > 0
    if (tid < MAS_RESERVOIR_PER_IMAGE) s_pos[tid] = (int)rsv_perm((uint32_t)tid, (uint32_t)HW, rsv_half_bits((uint32_t)HW), 0u, calls, k0, k1);
    for (int i = tid; i < n; i += RSV_THREADS) { s_drop[i] = 0; s_old[i] = -1; }
    __syncthreads();
    const uint32_t hm = rsv_half_bits((uint32_t)m);
    for (int t = tid; t < d; t += RSV_THREADS) {
        const int x = (int)rsv_perm((uint32_t)t, (uint32_t)m, hm, 1u, calls, k0, k1);
        if (x >= c) s_drop[x - c] = 1; else s_old[t] = x;     // distinct x: no two draws touch one entry
    }
    __syncthreads();
    // contiguous chunks per thread keep both rankings in index order
    const int chunk = (n + RSV_THREADS - 1) / RSV_THREADS, lo = min(tid * chunk, n), hi = min(lo + chunk, n);
    int dropped_old = 0;
    for (int t = lo; t < hi; ++t) dropped_old += s_old[t] >= 0;
    int at = rsv_scan(dropped_old, s_scan);
    for (int t = lo; t < hi; ++t)
        if (s_old[t] >= 0) s_list[at++] = s_old[t];
    int alive = 0;
    for (int i = lo; i < hi; ++i) alive += !s_drop[i];
    int rank = rsv_scan(alive, s_scan);                       // (its barriers also publish s_list)
    for (int i = lo; i < hi; ++i) {
        int dst = -1;
        if (!s_drop[i]) { dst = rank < free_slots ? c + rank : s_list[rank - free_slots]; ++rank; }
        plan[2 * i] = dst;
        plan[2 * i + 1] = (i / MAS_RESERVOIR_PER_IMAGE) * HW + s_pos[i % MAS_RESERVOIR_PER_IMAGE];
    }
    __syncthreads();                                          // every read of the counters lies before this barrier
    if (tid == 0) { state[0] = m < R ? m : R; state[1] = (int)(calls + 1u); }
}

__global__ __launch_bounds__(RSV_THREADS) void reservoir_copy_kernel(const float* __restrict__ z, float* __restrict__ buf,
                                                                     const int* __restrict__ plan, int n, int R, long long rows, int D) {
    const int i = blockIdx.x * (RSV_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (i >= n) return;
    const int dst = plan[2 * i], src = plan[2 * i + 1];
    if (dst < 0 || dst >= R || src < 0 || src >= rows) return;
    const f32x4* from = reinterpret_cast<const f32x4*>(z + (size_t)src * D);
    f32x4* to = reinterpret_cast<f32x4*>(buf + (size_t)dst * D);
    for (int q = lane; q < D / 4; q += 64) to[q] = from[q];
}

extern "C" int mas_reservoir_collect(const float* z, float* buf, int32_t* state, int32_t* plan, long long seed, int R, int B, int HW, int D,
                                     void* stream) {
    MAS_ENTER();
    if (HW < MAS_RESERVOIR_PER_IMAGE) MAS_FAIL(MAS_EINVAL, "reservoir_collect: %d latent positions, fewer than the %d drawn per image", HW,
                                               MAS_RESERVOIR_PER_IMAGE);
    if (B <= 0 || R <= 0 || (long long)MAS_RESERVOIR_PER_IMAGE * B > R)
        MAS_FAIL(MAS_EINVAL, "reservoir_collect: %d candidates per call (10 * B, B=%d) exceed the reservoir's %d rows", 10 * B, B, R);
    if (D <= 0 || D % 4) MAS_FAIL(MAS_EINVAL, "reservoir_collect: D=%d is not a positive multiple of 4 (16-byte row copies)", D);
    if (MAS_RESERVOIR_PER_IMAGE * B > MAS_RESERVOIR_MAX_CANDIDATES)
        MAS_FAIL(MAS_EUNSUPPORTED, "reservoir_collect: B=%d gives more than %d candidates per call", B, MAS_RESERVOIR_MAX_CANDIDATES);
    if ((long long)R + MAS_RESERVOIR_PER_IMAGE * B > (1ll << 30) || (long long)B * HW > (1ll << 30))
        MAS_FAIL(MAS_EUNSUPPORTED, "reservoir_collect: R=%d, B*HW=%lld beyond 2^30 rows", R, (long long)B * HW);
    if (!z || !buf || !state || !plan) MAS_FAIL(MAS_EINVAL, "reservoir_collect: null argument");
    if (((uintptr_t)z | (uintptr_t)buf) & 15) MAS_FAIL(MAS_EINVAL, "reservoir_collect: z and buf must be 16-byte aligned");
    const int n = MAS_RESERVOIR_PER_IMAGE * B;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(reservoir_plan_kernel, dim3(1), dim3(RSV_THREADS), 0, s, state, plan, (uint32_t)((unsigned long long)seed & 0xffffffffu),
                       (uint32_t)((unsigned long long)seed >> 32), R, B, HW);
    MAS_CHECK_LAUNCH("reservoir_plan");
    hipLaunchKernelGGL(reservoir_copy_kernel, dim3(mas_cdiv(n, RSV_THREADS / 64)), dim3(RSV_THREADS), 0, s, z, buf, plan, n, R,
                       (long long)B * HW, D);
    MAS_CHECK_LAUNCH("reservoir_copy");
    return MAS_OK;
}
