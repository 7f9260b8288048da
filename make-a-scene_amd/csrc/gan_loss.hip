// The tail of the VQ-IMG objective for gfx950 (reference losses/loss_img.py:56-141): what follows the decoder, LPIPS and the PatchGAN
// discriminator -- the L1 reconstruction term, the generator / hinge terms over the logits, the adaptive generator weight and the loss --
// as a handful of launches that read nothing on the host, so that the step captures into a graph.
//   * gan_l1_fwd      : sum |rec - img| -> one fp64 partial per work-group.  A lane adds RUN = 8 terms in fp32 as a fixed pairwise tree
//                       (three additions deep), everything beyond that -- the lane's tiles, lanes, work-groups, the finalize -- is fp64.
//   * gan_l1_finalize : one work-group, fixed order -> out = {sum, nll = sum / n + perceptual_weight mean(p)} fp32, each rounded once
//   * gan_l1_bwd      : d rec = +coef where rec > img, -coef where rec < img, 0 otherwise (equal, or a NaN), coef = g / float(n)
//   * gan_logits_fwd  : ONE work-group over the PatchGAN logits -> {-mean(fake), mean(relu(1 - real)), mean(relu(1 + fake)), d_loss, gate}
//   * gan_logits_bwd  : elementwise; zero at the hinge knees, as ATen's relu backward
//   * gan_combine_fwd : ONE work-group: both squared norms, d_weight, the gate from the device step counter, the loss; optionally
//                       advances the counter
//   * gan_combine_bwd : one lane: the three coefficients of the (linear) loss times the upstream gradient
// Both images are read in place, each dense NCHW or dense NHWC, fp32 or bf16: the walk is rec's memory order (its gradient is written
// in 4-byte or 2-byte units along it), img's element is found by index arithmetic in 32 bits (n < 2^31).  No atomics anywhere: every sum
// has one order, fixed by the shape and the CU count.
#include "mas_common.h"

namespace {

constexpr int NT = 256;
constexpr int RUN = MAS_GAN_RUN;         // terms a lane adds in fp32 before the sum goes on in fp64
constexpr int TE = NT * RUN;             // elements per tile

__device__ __forceinline__ float ld_any(const void* p, int dt, unsigned i) {
    return dt == MAS_BF16 ? (float)reinterpret_cast<const bf16_t*>(p)[i] : reinterpret_cast<const float*>(p)[i];
}

// where element j of a dense [N, C, HW] tensor in layout `from` lies in the same tensor in the other layout
__device__ __forceinline__ unsigned other_layout(unsigned j, int from, unsigned C, unsigned HW) {
    const unsigned chw = C * HW, n = j / chw, r = j - n * chw;
    if (from == MAS_SEG_NCHW) { const unsigned c = r / HW, p = r - c * HW; return n * chw + p * C + c; }
    const unsigned p = r / C, c = r - p * C;
    return n * chw + c * HW + p;
}

// fixed tree over the work-group's 256 fp64 values; the result is valid in lane 0
__device__ __forceinline__ double block_sum(double v, double* s) {
    const int tid = threadIdx.x;
    __syncthreads();                     // (s may still be read from a previous call)
    s[tid] = v;
    __syncthreads();
    for (int o = NT / 2; o >= 1; o >>= 1) {
        if (tid < o) s[tid] += s[tid + o];
        __syncthreads();
    }
    return s[0];
}

// RUN = 8 fp32 terms -> their sum, three additions deep: with the one rounding of each term, no term passes through more than four
__device__ __forceinline__ float tree8(const float* d) { return ((d[0] + d[1]) + (d[2] + d[3])) + ((d[4] + d[5]) + (d[6] + d[7])); }

struct L1Args {
    const void* img; const void* rec; void* drec; float* dp;
    int img_dt, rec_dt, img_l, rec_l;
    unsigned n, C, HW, tiles;
    int B; float pw;
    const float* g;
    double* partials;
};

__global__ __launch_bounds__(NT) void gan_l1_fwd_kernel(const L1Args A) {
    __shared__ double s[NT];
    const bool same = A.img_l == A.rec_l;
    double acc = 0.0;
    for (unsigned tile = blockIdx.x; tile < A.tiles; tile += gridDim.x) {
        float d[RUN];
#pragma unroll
        for (int k = 0; k < RUN; ++k) {
            const unsigned j = tile * TE + k * NT + threadIdx.x;       // (tiles TE <= n + TE - 1 < 2^32)
            d[k] = 0.0f;
            if (j < A.n) {
                const unsigned i = same ? j : other_layout(j, A.rec_l, A.C, A.HW);
                d[k] = fabsf(ld_any(A.rec, A.rec_dt, j) - ld_any(A.img, A.img_dt, i));
            }
        }
        acc += (double)tree8(d);
    }
    const double total = block_sum(acc, s);
    if (threadIdx.x == 0) A.partials[blockIdx.x] = total;
}

__global__ __launch_bounds__(NT) void gan_l1_finalize_kernel(const double* __restrict__ partials, int blocks, double n, const float* __restrict__ p,
                                                             int B, float pw, float* __restrict__ out) {
    __shared__ double s[NT];
    double a = 0.0, q = 0.0;
    for (int i = threadIdx.x; i < blocks; i += NT) a += partials[i];
    for (int i = threadIdx.x; i < B; i += NT) q += (double)p[i];
    const double sum = block_sum(a, s);
    const double psum = block_sum(q, s);
    if (threadIdx.x == 0) {
        out[0] = (float)sum;
        out[1] = (float)(sum / n + (B > 0 ? (double)pw * (psum / (double)B) : 0.0));
    }
}

__global__ __launch_bounds__(NT) void gan_l1_bwd_kernel(const L1Args A) {
    const bool same = A.img_l == A.rec_l;
    const float g = A.g[0];
    const float coef = g / (float)A.n;
    if (A.dp && blockIdx.x == 0) {
        const float cp = g * (A.pw / (float)A.B);
        for (int b = threadIdx.x; b < A.B; b += NT) A.dp[b] = cp;
    }
    for (unsigned tile = blockIdx.x; tile < A.tiles; tile += gridDim.x) {
#pragma unroll
        for (int k = 0; k < RUN; ++k) {
            const unsigned j = tile * TE + k * NT + threadIdx.x;
            if (j < A.n) {
                const unsigned i = same ? j : other_layout(j, A.rec_l, A.C, A.HW);
                const float r = ld_any(A.rec, A.rec_dt, j), x = ld_any(A.img, A.img_dt, i);
                const float v = r > x ? coef : (r < x ? -coef : 0.0f);
                if (A.rec_dt == MAS_BF16) reinterpret_cast<bf16_t*>(A.drec)[j] = (bf16_t)v;
                else reinterpret_cast<float*>(A.drec)[j] = v;
            }
        }
    }
}

// the gate of the discriminator's terms (reference adopt_weight): on the device, from the step counter
__device__ __forceinline__ float gate_of(const long long* step, long long disc_start, float disc_factor) {
    return step[0] >= disc_start ? disc_factor : 0.0f;
}

// sum over n elements of f(x[i]) by the scheme of the L1 sum: fp32 trees of RUN terms per lane, fp64 beyond.  KIND 0: x, 1: relu(1 - x), 2: relu(1 + x)
template <int KIND>
__device__ __forceinline__ double logit_sum(const float* __restrict__ x, unsigned n, double* s) {
    double acc = 0.0;
    for (unsigned t0 = 0; t0 < n; t0 += TE) {
        float d[RUN];
#pragma unroll
        for (int k = 0; k < RUN; ++k) {
            const unsigned j = t0 + k * NT + threadIdx.x;
            d[k] = 0.0f;
            if (j < n) {
                const float v = x[j];
                if (KIND == 0) d[k] = v;
                else { const float t = KIND == 1 ? 1.0f - v : 1.0f + v; d[k] = t < 0.0f ? 0.0f : t; }      // (a NaN stays a NaN, as F.relu)
            }
        }
        acc += (double)tree8(d);
    }
    return block_sum(acc, s);
}

__global__ __launch_bounds__(NT) void gan_logits_fwd_kernel(const float* __restrict__ fake, unsigned n_fake, const float* __restrict__ real,
                                                            unsigned n_real, const long long* __restrict__ step, long long disc_start,
                                                            float disc_factor, float* __restrict__ out) {
    __shared__ double s[NT];
    const double sf = logit_sum<0>(fake, n_fake, s);
    const double hf = logit_sum<2>(fake, n_fake, s);
    const double hr = real ? logit_sum<1>(real, n_real, s) : 0.0;
    if (threadIdx.x == 0) {
        const double mr = real ? hr / (double)n_real : 0.0, mf = hf / (double)n_fake;
        out[0] = (float)(-(sf / (double)n_fake));
        out[1] = (float)mr;
        out[2] = (float)mf;
        const float gate = step ? gate_of(step, disc_start, disc_factor) : 0.0f;
        out[3] = (float)((double)gate * (0.5 * (mr + mf)));
        out[4] = gate;                                                           // what the backward reads: the counter may have moved by then
    }
}

// g_gen: upstream gradient of out[0] (or null): d fake = -(g_gen / n_fake).  g_d: upstream gradient of out[3] (or null), c = g_d (0.5 gate) / n
// with the gate the forward stored: d fake += c where fake > -1, d real = -c where real < 1.
__global__ __launch_bounds__(NT) void gan_logits_bwd_kernel(const float* __restrict__ fake, unsigned n_fake, const float* __restrict__ real,
                                                            unsigned n_real, const float* __restrict__ g_gen, const float* __restrict__ g_d,
                                                            const float* __restrict__ gate, float* __restrict__ dfake,
                                                            float* __restrict__ dreal) {
    const unsigned i = blockIdx.x * NT + threadIdx.x;
    const float half_gate = g_d ? 0.5f * gate[0] : 0.0f;
    const float hg = g_d ? g_d[0] * half_gate : 0.0f;
    if (i < n_fake) {
        float v = 0.0f;
        if (g_d) v = fake[i] > -1.0f ? hg / (float)n_fake : 0.0f;
        if (g_gen) v = v - g_gen[0] / (float)n_fake;
        dfake[i] = v;
    }
    if (dreal && i < n_real) dreal[i] = real[i] < 1.0f ? -(hg / (float)n_real) : 0.0f;
}

struct CombineArgs {
    const float* nll; const float* g_loss; const float* codebook; const float* face; const float* object;
    const float* nll_grads; const float* g_grads;
    long long* step;
    long long n_codebook, n_grads, disc_start;
    float disc_factor, disc_weight, codebook_weight;
    int advance;
    float* out;
};

__global__ __launch_bounds__(NT) void gan_combine_fwd_kernel(const CombineArgs A) {
    __shared__ double s[NT];
    double a = 0.0, b = 0.0, c = 0.0;
    for (long long i = threadIdx.x; i < A.n_grads; i += NT) {
        const double x = (double)A.nll_grads[i], y = (double)A.g_grads[i];
        a += x * x; b += y * y;
    }
    for (long long i = threadIdx.x; i < A.n_codebook; i += NT) c += (double)A.codebook[i];
    const double na = block_sum(a, s);
    const double nb = block_sum(b, s);
    const double cb = block_sum(c, s);
    if (threadIdx.x == 0) {
        const long long st = A.step[0];
        const float gate = st >= A.disc_start ? A.disc_factor : 0.0f;
        double ratio = sqrt(na) / (sqrt(nb) + 1e-4);
        ratio = ratio < 0.0 ? 0.0 : (ratio > 1e4 ? 1e4 : ratio);                 // (a NaN stays a NaN, as torch.clamp)
        const float d_weight = (float)(ratio * (double)A.disc_weight);
        const float c_g = d_weight * gate;
        double loss = (double)A.nll[0] + (double)c_g * (double)A.g_loss[0] + (double)A.codebook_weight * (cb / (double)A.n_codebook);
        if (A.face) loss += (double)A.face[0];
        if (A.object) loss += (double)A.object[0];
        A.out[0] = (float)loss;
        A.out[1] = d_weight;
        A.out[2] = c_g;
        A.out[3] = gate;
        if (A.advance) A.step[0] = st + 1;
    }
}

__global__ void gan_combine_bwd_kernel(const float* __restrict__ g, const float* __restrict__ out, float codebook_weight, long long n_codebook,
                                       float* __restrict__ grads) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        grads[0] = g[0];                                                         // nll, face, object
        grads[1] = g[0] * out[2];                                                // g_loss
        grads[2] = g[0] * (codebook_weight / (float)n_codebook);                 // every element of codebook_loss
    }
}

int l1_args(const char* what, const void* img, int img_dtype, int img_layout, const void* rec, int rec_dtype, int rec_layout, int N, int C, int H,
            int W, L1Args* A) {
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0) MAS_FAIL(MAS_EINVAL, "%s: empty shape [%d, %d, %d, %d]", what, N, C, H, W);
    if ((img_dtype != MAS_F32 && img_dtype != MAS_BF16) || (rec_dtype != MAS_F32 && rec_dtype != MAS_BF16))
        MAS_FAIL(MAS_EUNSUPPORTED, "%s: dtypes %d / %d (fp32 / bf16)", what, img_dtype, rec_dtype);
    if ((img_layout != MAS_SEG_NCHW && img_layout != MAS_SEG_NHWC) || (rec_layout != MAS_SEG_NCHW && rec_layout != MAS_SEG_NHWC))
        MAS_FAIL(MAS_EINVAL, "%s: layout codes %d / %d (MAS_SEG_NCHW or MAS_SEG_NHWC)", what, img_layout, rec_layout);
    const double n = (double)N * C * (double)H * W;
    if (n >= 2147483648.0) MAS_FAIL(MAS_EUNSUPPORTED, "%s: %.0f elements (fewer than 2^31)", what, n);
    if (!img || !rec) MAS_FAIL(MAS_EINVAL, "%s: null argument", what);
    if (reinterpret_cast<uintptr_t>(img) % mas_esize(img_dtype) || reinterpret_cast<uintptr_t>(rec) % mas_esize(rec_dtype))
        MAS_FAIL(MAS_EINVAL, "%s: a tensor is not aligned to its element size", what);
    memset(A, 0, sizeof(*A));
    A->img = img; A->rec = rec; A->img_dt = img_dtype; A->rec_dt = rec_dtype;
    A->C = (unsigned)C; A->HW = (unsigned)(H * W); A->n = (unsigned)n; A->tiles = (A->n + TE - 1) / TE;
    // one channel or one pixel: the two layouts are the same array
    A->img_l = (C == 1 || A->HW == 1) ? MAS_SEG_NCHW : img_layout;
    A->rec_l = (C == 1 || A->HW == 1) ? MAS_SEG_NCHW : rec_layout;
    return MAS_OK;
}

int l1_grid(unsigned tiles) {
    const long long cap = (long long)mas_num_cus() * 8;
    return (int)(tiles < cap ? tiles : cap);
}

}  // namespace

extern "C" int mas_gan_l1_blocks(int N, int C, int H, int W) {
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0) MAS_FAIL(MAS_EINVAL, "gan_l1_blocks: empty shape [%d, %d, %d, %d]", N, C, H, W);
    const double n = (double)N * C * (double)H * W;
    if (n >= 2147483648.0) MAS_FAIL(MAS_EUNSUPPORTED, "gan_l1_blocks: %.0f elements (fewer than 2^31)", n);
    return l1_grid(((unsigned)n + TE - 1) / TE);
}

extern "C" int mas_gan_l1_fwd(const void* img, int img_dtype, int img_layout, const void* rec, int rec_dtype, int rec_layout, int N, int C, int H,
                              int W, double* partials, int n_partials, void* stream) {
    MAS_ENTER();
    L1Args A;
    if (int rc = l1_args("gan_l1_fwd", img, img_dtype, img_layout, rec, rec_dtype, rec_layout, N, C, H, W, &A)) return rc;
    if (!partials) MAS_FAIL(MAS_EINVAL, "gan_l1_fwd: null argument");
    const int blocks = l1_grid(A.tiles);
    if (n_partials < blocks) MAS_FAIL(MAS_EWORKSPACE, "gan_l1_fwd: %d partial sums of workspace, mas_gan_l1_blocks says %d", n_partials, blocks);
    A.partials = partials;
    hipLaunchKernelGGL(gan_l1_fwd_kernel, dim3((unsigned)blocks), dim3(NT), 0, reinterpret_cast<hipStream_t>(stream), A);
    MAS_CHECK_LAUNCH("gan_l1_fwd");
    return MAS_OK;
}

extern "C" int mas_gan_l1_finalize(const double* partials, int n_partials, long long numel, const float* perceptual, int B,
                                   float perceptual_weight, float* out, void* stream) {
    MAS_ENTER();
    if (!partials || !out) MAS_FAIL(MAS_EINVAL, "gan_l1_finalize: null argument");
    if (n_partials <= 0 || numel <= 0 || B < 0) MAS_FAIL(MAS_EINVAL, "gan_l1_finalize: partials=%d numel=%lld B=%d", n_partials, numel, B);
    if (!perceptual) B = 0;
    hipLaunchKernelGGL(gan_l1_finalize_kernel, dim3(1), dim3(NT), 0, reinterpret_cast<hipStream_t>(stream), partials, n_partials, (double)numel,
                       perceptual, B, perceptual_weight, out);
    MAS_CHECK_LAUNCH("gan_l1_finalize");
    return MAS_OK;
}

extern "C" int mas_gan_l1_bwd(const void* img, int img_dtype, int img_layout, const void* rec, int rec_dtype, int rec_layout, int N, int C, int H,
                              int W, const float* grad, void* drec, float* dperceptual, int B, float perceptual_weight, void* stream) {
    MAS_ENTER();
    L1Args A;
    if (int rc = l1_args("gan_l1_bwd", img, img_dtype, img_layout, rec, rec_dtype, rec_layout, N, C, H, W, &A)) return rc;
    if (!grad || !drec) MAS_FAIL(MAS_EINVAL, "gan_l1_bwd: null argument");
    if (reinterpret_cast<uintptr_t>(drec) % mas_esize(rec_dtype)) MAS_FAIL(MAS_EINVAL, "gan_l1_bwd: drec is not aligned to its element size");
    if (dperceptual && B <= 0) MAS_FAIL(MAS_EINVAL, "gan_l1_bwd: B = %d perceptual terms", B);
    A.g = grad; A.drec = drec; A.dp = dperceptual; A.B = B; A.pw = perceptual_weight;
    hipLaunchKernelGGL(gan_l1_bwd_kernel, dim3((unsigned)l1_grid(A.tiles)), dim3(NT), 0, reinterpret_cast<hipStream_t>(stream), A);
    MAS_CHECK_LAUNCH("gan_l1_bwd");
    return MAS_OK;
}

static int logits_check(const char* what, const float* fake, long long n_fake, const float* real, long long n_real) {
    if (!fake || n_fake <= 0 || (real && n_real <= 0)) MAS_FAIL(MAS_EINVAL, "%s: fake=%p n_fake=%lld n_real=%lld", what, (const void*)fake, n_fake, n_real);
    if (n_fake > (1LL << 30) || n_real > (1LL << 30)) MAS_FAIL(MAS_EUNSUPPORTED, "%s: more than 2^30 logits", what);
    return MAS_OK;
}

extern "C" int mas_gan_logits_fwd(const float* fake, long long n_fake, const float* real, long long n_real, const long long* global_step,
                                  long long disc_start, float disc_factor, float* out, void* stream) {
    MAS_ENTER();
    if (int rc = logits_check("gan_logits_fwd", fake, n_fake, real, n_real)) return rc;
    if (!out) MAS_FAIL(MAS_EINVAL, "gan_logits_fwd: null argument");
    hipLaunchKernelGGL(gan_logits_fwd_kernel, dim3(1), dim3(NT), 0, reinterpret_cast<hipStream_t>(stream), fake, (unsigned)n_fake, real,
                       (unsigned)(real ? n_real : 0), global_step, disc_start, disc_factor, out);
    MAS_CHECK_LAUNCH("gan_logits_fwd");
    return MAS_OK;
}

extern "C" int mas_gan_logits_bwd(const float* fake, long long n_fake, const float* real, long long n_real, const float* grad_gen,
                                  const float* grad_d, const float* gate, float* dfake, float* dreal, void* stream) {
    MAS_ENTER();
    if (int rc = logits_check("gan_logits_bwd", fake, n_fake, real, n_real)) return rc;
    if (!dfake || (!grad_gen && !grad_d)) MAS_FAIL(MAS_EINVAL, "gan_logits_bwd: null argument");
    if (grad_d && !gate) MAS_FAIL(MAS_EINVAL, "gan_logits_bwd: the hinge terms need the gate the forward stored");
    if (dreal && (!real || !grad_d)) MAS_FAIL(MAS_EINVAL, "gan_logits_bwd: dreal without real logits or without grad_d");
    const long long n = dreal && n_real > n_fake ? n_real : n_fake;
    hipLaunchKernelGGL(gan_logits_bwd_kernel, dim3((unsigned)((n + NT - 1) / NT)), dim3(NT), 0, reinterpret_cast<hipStream_t>(stream), fake,
                       (unsigned)n_fake, real, (unsigned)(real ? n_real : 0), grad_gen, grad_d, gate, dfake, dreal);
    MAS_CHECK_LAUNCH("gan_logits_bwd");
    return MAS_OK;
}

extern "C" int mas_gan_combine_fwd(const float* nll, const float* g_loss, const float* codebook, long long n_codebook, const float* face,
                                   const float* object, const float* nll_grads, const float* g_grads, long long n_grads, long long* global_step,
                                   long long disc_start, float disc_factor, float disc_weight, float codebook_weight, int advance, float* out,
                                   void* stream) {
    MAS_ENTER();
    if (!nll || !g_loss || !codebook || !nll_grads || !g_grads || !global_step || !out) MAS_FAIL(MAS_EINVAL, "gan_combine_fwd: null argument");
    if (n_codebook <= 0 || n_grads <= 0) MAS_FAIL(MAS_EINVAL, "gan_combine_fwd: n_codebook=%lld n_grads=%lld must be positive", n_codebook, n_grads);
    if (reinterpret_cast<uintptr_t>(global_step) % 8) MAS_FAIL(MAS_EINVAL, "gan_combine_fwd: the global-step scalar is not 8-byte aligned");
    CombineArgs A;
    memset(&A, 0, sizeof(A));
    A.nll = nll; A.g_loss = g_loss; A.codebook = codebook; A.face = face; A.object = object; A.nll_grads = nll_grads; A.g_grads = g_grads;
    A.step = global_step; A.n_codebook = n_codebook; A.n_grads = n_grads; A.disc_start = disc_start; A.disc_factor = disc_factor;
    A.disc_weight = disc_weight; A.codebook_weight = codebook_weight; A.advance = advance != 0; A.out = out;
    hipLaunchKernelGGL(gan_combine_fwd_kernel, dim3(1), dim3(NT), 0, reinterpret_cast<hipStream_t>(stream), A);
    MAS_CHECK_LAUNCH("gan_combine_fwd");
    return MAS_OK;
}

extern "C" int mas_gan_combine_bwd(const float* grad, const float* out, float codebook_weight, long long n_codebook, float* grads, void* stream) {
    MAS_ENTER();
    if (!grad || !out || !grads) MAS_FAIL(MAS_EINVAL, "gan_combine_bwd: null argument");
    if (n_codebook <= 0) MAS_FAIL(MAS_EINVAL, "gan_combine_bwd: n_codebook=%lld must be positive", n_codebook);
    hipLaunchKernelGGL(gan_combine_bwd_kernel, dim3(1), dim3(64), 0, reinterpret_cast<hipStream_t>(stream), grad, out, codebook_weight, n_codebook,
                       grads);
    MAS_CHECK_LAUNCH("gan_combine_bwd");
    return MAS_OK;
}
