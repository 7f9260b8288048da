/*
 * mas_hip.h -- C ABI of libmas_hip.so, the MI355X (gfx950) kernels behind the
 * Make-A-Scene hot path (VQ-IMG / VQ-SEG conv stack, vector quantiser, attention).
 *
 * The reference (CasualGANPapers/Make-A-Scene) has no FFI layer: its arithmetic is
 * reached through torch.nn call sites.  Each entry point below names the reference
 * call site(s) it replaces.  The Python host (make-a-scene_amd/mas_hip/) binds these
 * with ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless noted.
 *   - the caller owns every buffer (incl. workspaces); the library never allocates or
 *     frees device memory and keeps no pointer after return.
 *   - asynchronous on the caller's hipStream_t (passed as void*); no hidden syncs.
 *   - return 0 on success, a negative MAS_E* code otherwise; mas_last_error() gives a
 *     thread-local message.  No C++ exception crosses the ABI.
 *   - activations are NHWC ("channels last"), element type MAS_BF16 or MAS_F32,
 *     accumulation is always fp32.
 */
#ifndef MAS_HIP_H
#define MAS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MAS_ABI_VERSION 10

enum { MAS_OK = 0, MAS_EINVAL = -1, MAS_EUNSUPPORTED = -2, MAS_ELAUNCH = -3, MAS_EWORKSPACE = -4 };
enum { MAS_F32 = 0, MAS_BF16 = 1 };
/* input prologue fused into the conv / wgrad loaders */
enum { MAS_ACT_NONE = 0,      /* a = x                                   */
       MAS_ACT_AFFINE = 1,    /* a = x*scale[n,c] + shift[n,c]  (GroupNorm apply, modules.py:40-41) */
       MAS_ACT_AFFINE_SILU = 2 /* a = silu(x*scale + shift)     (+ swish, modules.py:35-37)         */ };

typedef struct MasConvDesc {
    int32_t N, H, W, Cin;       /* input  [N,H,W,Cin]  (the tensor in memory; before any upsample fold) */
    int32_t Ho, Wo, Cout;       /* output [N,Ho,Wo,Cout] */
    int32_t ks;                 /* 1 or 3 (square); bf16 also 4 (forward / data gradient, stride 1 or 2) and 2 / 4 stride 1 (weight gradient):
                                   the PatchGAN discriminator of the loss stack, losses/discriminator.py:20-36 */
    int32_t stride;             /* 1 or 2           */
    int32_t pad_top, pad_left;  /* input row = ho*stride + kh - pad_top ; rows/cols outside [0,H)x[0,W) read 0
                                   (covers padding=1, and the right/bottom-only pad of Downsample, modules.py:76-78) */
    int32_t in_dtype;           /* MAS_F32 | MAS_BF16 : x, residual, (dy for wgrad) */
    int32_t out_dtype;          /* MAS_F32 | MAS_BF16 : y */
    int32_t act;                /* MAS_ACT_* prologue applied to x on load (padding stays exactly 0) */
    int32_t upsample;           /* 1: logical input is nearest-x2 of x (F.interpolate, modules.py:56): pixel (h,w) reads x[h>>1][w>>1];
                                   H,W above are then the PHYSICAL (pre-upsample) size */
    int32_t w_layout;           /* MAS_WLAYOUT_*: how w_packed was packed; mas_conv_fwd requires mas_conv_weight_layout(d)
                                   or MAS_WLAYOUT_K64 (always accepted); ignored by mas_conv_wgrad */
    int32_t wgrad_cus;          /* (ABI v10) CUs the persistent 3x3 weight-gradient grid is sized for, which sets its split-K count:
                                   0 = all of them, -1 = three quarters (for a caller that runs the weight gradient on a second stream
                                   beside other kernels), n > 0 = n (values above the device's count: all).  Read by mas_conv_wgrad_splits,
                                   mas_conv_wgrad_partial and mas_conv_wgrad only -- hand the SAME value to splits and partial; ignored
                                   by every other entry point */
} MasConvDesc;

int         mas_abi_version(void);
const char* mas_last_error(void);
/* Name of the kernel the last successful launch of this process ran ("conv3x3_wide", "conv_s2_fwd", "wgrad_thin", ...; "" before the
 * first one; process-wide, because a backward pass launches from autograd's threads): every entry point dispatches on shape, and
 * tests / per-shape profiles assert which kernel a shape really took.  A diagnostic: meaningful while one thread launches at a time. */
const char* mas_last_kernel(void);

/* ---- weight packing (host-visible layout contract) -------------------------------
 * Packs an OIHW fp32 parameter (nn.Conv2d.weight, e.g. modules.py:93-104) into the
 * kernel layout [ks*ks][Cout_pad][Cin_pad] (dtype `dtype`, zero padded; Cout_pad =
 * roundup(Cout,128), Cin_pad = roundup(Cin,64), so the kernels load tiles without bounds checks).
 *   transpose=0 : forward operand            Wp[t][o][i] = W[o][i][kh][kw], t = kh*ks+kw
 *   transpose=1 : data-gradient operand      Wp[t][i][o] = W[o][i][ks-1-kh][ks-1-kw]
 *                 (conv of dY with the flipped, in/out-swapped filter; then "Cout"=Cin)
 */
size_t mas_packed_weight_elems(int Cout, int Cin, int ks);
int    mas_pack_conv_weight(const float* w_oihw, void* packed, int Cout, int Cin, int ks,
                            int transpose, int dtype, void* stream);
/* Two LDS images exist.  MAS_WLAYOUT_K64 (what mas_pack_conv_weight emits; every kernel but one reads it):
 * [Cin/64 chunks][tap][Cout_pad][128 B], 16-byte slots XOR-swizzled with (row>>1)&7.  MAS_WLAYOUT_K32 (bf16 only; the
 * wide 3x3 kernel, conv3x3_wide.hip): [Cin/32 chunks][tap][Cout_pad][64 B], slots XOR-swizzled with (row>>2)&3.
 * mas_conv_weight_layout(d) tells which image mas_conv_fwd prefers for a convolution; a K64 image is always accepted
 * (the call then takes the kernels that read it).  Same buffer size for both (mas_packed_weight_elems).
 * MAS_WLAYOUT_UP2 (bf16, 3x3 only; conv_up2.hip): the sub-pixel form of `Upsample` + conv (reference models/modules.py:44-59) --
 * output pixel (2i + a, 2j + b) of the convolution over the nearest-x2 image sees the 2x2 window x[i + a - 1 + r][j + b - 1 + s] with
 * Wp[a][b][r][s] = sum of W[kh][kw] over kh in R(a, r), kw in R(b, s), R(0,0) = {0}, R(0,1) = {1,2}, R(1,0) = {0,1}, R(1,1) = {2}
 * (summed in fp32, then rounded).  Image: [phase 2a+b][Cin/32 chunks][tap 2r+s][Cout_pad][64 B], rows and slots as K32;
 * transpose = 1 (data-gradient operand): in/out swapped and tap (1-r, 1-s) stored at (r, s).  mas_packed_weight_elems_up2 elements. */
enum { MAS_WLAYOUT_K64 = 0, MAS_WLAYOUT_K32 = 1, MAS_WLAYOUT_UP2 = 2 };
size_t mas_packed_weight_elems_up2(int Cout, int Cin);
int    mas_conv_weight_layout(const MasConvDesc* d);
int    mas_pack_conv_weight_layout(const float* w_oihw, void* packed, int Cout, int Cin, int ks,
                                   int transpose, int dtype, int layout, void* stream);

/* Batched packing: every item of a device-resident table in ONE launch (a training step repacks ~160 weight images after the
 * optimizer step; one launch instead of 160 dependent 8-us launches).  The table is built by the caller: item i covers work-groups
 * [first_block, first_block + n_blocks) of the grid, n_blocks = mas_pack_batch_blocks(...) for its shape, items in ascending
 * first_block order, total_blocks = their sum.  Same images as mas_pack_conv_weight_layout (K32: bf16 3x3 only).               */
typedef struct MasPackItem {
    const float* w_oihw; void* packed;
    int Cout, Cin, ks, transpose, dtype, layout, first_block, n_blocks;
} MasPackItem;
int    mas_pack_batch_blocks(int Cout, int Cin, int ks, int transpose, int dtype, int layout);
int    mas_pack_conv_weight_batch(const MasPackItem* items_device, int n_items, int total_blocks, void* stream);

/* The bf16 images of many parameters in ONE launch, each parameter READ ONCE: a work-group stages a 64 x 64 x taps tile of the OIHW
 * tensor in LDS (coalesced runs) and writes every image the item lists -- forward / data-gradient operand, K64 / K32 -- from it,
 * zero padding included.  Bitwise the images of mas_pack_conv_weight_layout.  Item i covers work-groups [first_block, first_block +
 * mas_pack_tile_blocks(Cout, Cin, ks)), items in ascending first_block order; max_ks = the largest ks in the table (sizes the LDS).    */
typedef struct MasPackTileItem {
    const float* w_oihw; void* img[4];
    int transpose[4], layout[4];
    int n_img, Cout, Cin, ks, first_block, pad_;
} MasPackTileItem;
int    mas_pack_tile_blocks(int Cout, int Cin, int ks);
int    mas_pack_conv_weight_tiles(const MasPackTileItem* items_device, int n_items, int total_blocks, int max_ks, void* stream);

/* ---- Adam over many tensors in ONE launch (replaces torch.optim.Adam.step of reference train.py:99-103 for fp32 parameters; same
 * arithmetic in the same order as torch's fused kernel: g' = g + wd p; m = b1 m + (1-b1) g'; v = b2 v + (1-b2) g'^2;
 * p -= (lr / bias_correction1) * m / (sqrt(v) / sqrt(bias_correction2) + eps), bias_correction_k = 1 - beta_k^step from the caller).
 * Item i covers work-groups [first_block, first_block + mas_adam_blocks(n)); items in ascending first_block order, table in DEVICE memory.
 * No amsgrad, no maximize; p, g, m, v fp32 of n elements each (16-byte aligned tensors take the vector path).                        */
typedef struct MasAdamItem {
    float* p; const float* g; float* m; float* v;
    long long n;
    int first_block, pad_;
} MasAdamItem;
int    mas_adam_blocks(long long numel);
int    mas_adam_multi(const MasAdamItem* items_device, int n_items, int total_blocks, float lr, float beta1, float beta2, float eps,
                      float weight_decay, double bias_correction1, double bias_correction2, void* stream);

/* ---- Global-norm gradient clipping and AdamW over the same table (what torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW do between
 * backward() and step(); additions under ABI 10).  Every entry walks the MasAdamItem table above (g, n, first_block; p, m, v are read only
 * by mas_adam_multi_ex), total_blocks = the sum of mas_adam_blocks(n).
 *   mas_grad_sqnorm_multi: partials[b] = sum of g^2 over work-group b's (at most 4096) elements, squared and added in fp64; `partials` holds
 *     total_blocks doubles, owned by the caller.  Fixed summation order: the same data gives the same bits.  No atomics.
 *   mas_grad_clip_coef: ONE work-group adds partials[0 .. n_partials) and then extra[0 .. n_extra) in fp64 (`extra`: squared norms of tensors
 *     that no table holds; may be NULL with n_extra = 0, and n_partials may be 0 when n_extra is not), then writes
 *     out[0] = (float)sqrt(sum), out[1] = min(max_norm / (out[0] + 1e-6f), 1) in fp32 -- clip_grad_norm_'s coefficient.  A NaN sum gives a NaN
 *     norm AND a NaN coefficient (error_if_nonfinite = False).  max_norm <= 0, NaN or infinite: MAS_EINVAL.
 *   mas_adam_multi_ex: mas_adam_multi with g * (*grad_scale_device) in place of g (NULL: no scaling; g is not written) and, with
 *     decoupled_wd != 0, AdamW's weight decay: p -= lr wd p ahead of the moment update, no wd p term in g.  NULL and 0 is mas_adam_multi.
 *   mas_grad_scale_multi: g *= *scale_device in place (the items' g is WRITTEN here, const in the struct notwithstanding).               */
int    mas_grad_sqnorm_multi(const MasAdamItem* items_device, int n_items, int total_blocks, double* partials, void* stream);
int    mas_grad_clip_coef(const double* partials, int n_partials, const double* extra, int n_extra, float max_norm, float* out, void* stream);
int    mas_adam_multi_ex(const MasAdamItem* items_device, int n_items, int total_blocks, float lr, float beta1, float beta2, float eps,
                         float weight_decay, double bias_correction1, double bias_correction2, const float* grad_scale_device,
                         int decoupled_wd, void* stream);
int    mas_grad_scale_multi(const MasAdamItem* items_device, int n_items, int total_blocks, const float* scale_device, void* stream);

/* ---- An exponential moving average of the weights inside the Adam launch, a guard against a non-finite gradient norm, and the swap that
 * puts the averaged weights in front of the kernels (what torch._foreach_lerp_ after step(), a host read of the norm, and
 * `w.data.copy_(ema)` do; additions under ABI 10).  Both entries walk the MasAdamItem table above and take a second DEVICE array of n_items
 * pointers beside it: entry i belongs to item i, fp32 of n elements.
 *   mas_adam_multi_ema: mas_adam_multi_ex, and after the update of an element e = fma(1 - ema_decay, p_new - e, e) -- torch.lerp(e, p_new,
 *     1 - ema_decay), 1 - ema_decay rounded to fp32 once -- with e = ema_device[i]; e is read with p, g, m, v and written with p, m, v (36
 *     bytes per element; the vector path needs all five pointers 16-byte aligned).  A NULL entry: that item keeps no average; ema_device
 *     itself may be NULL.  grad_norm_device non-NULL (normally `out` of mas_grad_clip_coef, with grad_scale_device = out + 1): every
 *     work-group reads *grad_norm_device once, and when it is NaN or +-inf returns before its first store -- p, m, v and e of EVERY item keep
 *     their bits; the caller's step count is its own business.  Both NULL is mas_adam_multi_ex.  ema_decay outside [0, 1) or NaN: MAS_EINVAL.
 *   mas_swap_multi: p and other_device[i] exchange their n elements (p, n, first_block of the items are read; g, m, v are not); items with
 *     a NULL entry are left alone.  Twice is the identity.                                                                              */
int    mas_adam_multi_ema(const MasAdamItem* items_device, float* const* ema_device, int n_items, int total_blocks, float lr, float beta1,
                          float beta2, float eps, float weight_decay, double bias_correction1, double bias_correction2,
                          const float* grad_scale_device, int decoupled_wd, float ema_decay, const float* grad_norm_device, void* stream);
int    mas_swap_multi(const MasAdamItem* items_device, float* const* other_device, int n_items, int total_blocks, void* stream);

/* ---- The Adam step with everything that changes from step to step read from DEVICE memory, so that the launches can be captured into a
 * graph once and replayed (additions under ABI 10).
 *   mas_adam_multi_dev: mas_adam_multi_ema with the learning rate (*lr_device, fp32), the step count of item i (*step_device[i], fp32: the
 *     number of steps ALREADY taken, so this step is t = *step_device[i] + 1; one pointer per item beside the table, like ema_device) and the
 *     EMA counter (*ema_count_device, fp32) read on the device.  Two launches: a small one (one thread per item) writes item i's record
 *     scalars_device[4 i ..] = {(float)(lr / (1 - beta1^t)), (float)sqrt(1 - beta2^t), lr, ema_w}, the powers, the division and the root in
 *     fp64 from the fp64 betas as the host entries' callers form them; the Adam launch reads its item's record.  scalars_device: 4 n_items
 *     floats, 16-byte aligned, owned by the caller.  ema_w = 1 - (float)ema_decay, or with ema_count_device non-NULL
 *     1 - (float)min(ema_decay, (1 + k) / (10 + k)), k = *ema_count_device.  ema_device, grad_scale_device, decoupled_wd and
 *     grad_norm_device are mas_adam_multi_ema's.  The entry advances nothing.
 *   mas_adam_advance_dev: counters[0 .. n) += 1 (fp32), one launch, to be issued BEHIND the step's Adam launches.                       */
int    mas_adam_multi_dev(const MasAdamItem* items_device, float* const* ema_device, const float* const* step_device, int n_items,
                          int total_blocks, const float* lr_device, double beta1, double beta2, float eps, float weight_decay,
                          const float* grad_scale_device, int decoupled_wd, double ema_decay, const float* ema_count_device,
                          const float* grad_norm_device, float* scalars_device, void* stream);
int    mas_adam_advance_dev(float* counters, int n, void* stream);

/* ---- GroupNorm statistics (replaces the reduction half of torch.nn.GroupNorm,
 * modules.py:40-41).  x: [N,HW,C] NHWC.  Outputs:
 *   mean_rstd [N][G][2] fp32, scale_shift [N][C][2] fp32 with
 *   scale = rstd*gamma, shift = beta - mean*rstd*gamma  (consumed by the conv prologue).
 * workspace: mas_gn_stats_workspace(N,C) bytes.                                      */
size_t mas_gn_stats_workspace(int N, int C);
int    mas_gn_stats(const void* x, int dtype, int N, int HW, int C, int G, float eps,
                    const float* gamma, const float* beta, float* mean_rstd, float* scale_shift,
                    void* workspace, size_t ws_bytes, void* stream);

/* ---- GroupNorm(+SiLU) backward.  Given da = dL/d act(gn(x)) computes
 *   dx [N,HW,C] (+ dres if non-NULL, the residual-branch gradient), dgamma[C], dbeta[C].
 * act is MAS_ACT_AFFINE or MAS_ACT_AFFINE_SILU.                                       */
size_t mas_gn_bwd_workspace(int N, int C);
int    mas_gn_bwd(const void* x, const void* da, const void* dres, int dtype, int N, int HW, int C, int G,
                  int act, const float* gamma, const float* mean_rstd, const float* scale_shift,
                  void* dx, float* dgamma, float* dbeta, void* workspace, size_t ws_bytes, void* stream);
/* mas_gn_bwd takes the small-map kernel (bf16, h*w <= 512 pixels, see mas_gn_small_supported) where it applies and otherwise
 * mas_gn_bwd_3pass: reduce / finalize / apply as three launches (x and da are read twice; every dtype and shape), also callable
 * directly.  Same arguments, same workspace; bitwise reproducible run to run.  (Round 4's one-launch kernels lost to it on MI355X and
 * are shelved: docs/history/experiments/r4_gn_queue.patch, profiles/r04_gn_queue_v2.txt.)                                            */
int    mas_gn_bwd_3pass(const void* x, const void* da, const void* dres, int dtype, int N, int HW, int C, int G,
                        int act, const float* gamma, const float* mean_rstd, const float* scale_shift,
                        void* dx, float* dgamma, float* dbeta, void* workspace, size_t ws_bytes, void* stream);

/* ---- materialised GroupNorm(+SiLU) output: a [N,HW,C] = act(x * scale + shift), scale_shift [N][C][2] from mas_gn_stats, act
 * MAS_ACT_AFFINE or MAS_ACT_AFFINE_SILU, rounded to `dtype` exactly as the fused loaders of mas_conv_fwd / mas_conv_wgrad round it
 * (reference models/modules.py:121-128 as a tensor).  The optional alternative to the fused prologue: one read + one write, after
 * which the convolution and its weight gradient run prologue-free (act = NONE) on `a`.                                          */
int mas_gn_act(const void* x, void* a, int dtype, int N, int HW, int C, int act, const float* scale_shift, void* stream);

/* Small maps (bf16, h*w <= 1024 pixels, C % 64 == 0, whole groups inside a 64-channel block: mas_gn_small_supported != 0): the
 * statistics of mas_gn_stats AND the tensor of mas_gn_act in ONE launch -- a work-group keeps an (image, 64-channel block) slab in
 * registers between the reduction and the element-wise phase; three dependent launches become one.  mas_gn_bwd takes the matching
 * backward kernel for such tensors by itself (one launch + the batch sums for dgamma / dbeta).                                     */
int mas_gn_small_supported(int dtype, int HW, int C, int G);
int mas_gn_stats_act(const void* x, void* a, int dtype, int N, int HW, int C, int G, float eps, const float* gamma,
                     const float* beta, int act, float* mean_rstd, float* scale_shift, void* stream);

/* ---- convolution forward  (replaces F.conv2d at modules.py:49,68,93,100,113,145-160,
 * 219,236,345,364 and vqvae.py:15,18, with the GroupNorm-apply/SiLU of modules.py:121-128
 * fused into the input loader and bias / residual add (modules.py:136,191) into the epilogue).
 *   x         [N,H,W,Cin]     in_dtype
 *   scale_shift [N][Cin][2]   fp32, required iff act != NONE
 *   w_packed  from mas_pack_conv_weight (same dtype as x)
 *   bias      [Cout] fp32 or NULL
 *   residual  [N,Ho,Wo,Cout]  in_dtype or NULL (added in fp32 before the store)
 *   y         [N,Ho,Wo,Cout]  out_dtype
 * The data gradient of a stride-1 conv is this same entry point called on dy with the
 * transpose=1 packing and pad = ks-1-pad.                                             */
int mas_conv_fwd(const MasConvDesc* d, const void* x, const float* scale_shift, const void* w_packed,
                 const float* bias, const void* residual, void* y, void* stream);

/* Fused GroupNorm statistics: mas_conv_fwd_stats is mas_conv_fwd that ALSO writes, per output tile, the sum and the sum of squares
 * of every output channel (of the values as stored, i.e. after the bf16 rounding) into stats_partial [N][rows][Cout][2] fp32, where
 * rows = mas_conv_stat_rows(d) > 0 (0: this convolution's kernel has no fused statistics -- call mas_conv_fwd and mas_gn_stats).
 * mas_gn_stats_from_partials then replaces mas_gn_stats' pass over the tensor for the GroupNorm that consumes y (same outputs).
 * No atomics: the table is written once per tile and summed in a fixed order (bitwise run-to-run deterministic).                   */
int mas_conv_stat_rows(const MasConvDesc* d);
int mas_conv_fwd_stats(const MasConvDesc* d, const void* x, const float* scale_shift, const void* w_packed,
                       const float* bias, const void* residual, void* y, float* stats_partial, void* stream);
int mas_gn_stats_from_partials(const float* partial, int N, int HW, int C, int G, int rows, float eps, const float* gamma,
                               const float* beta, float* mean_rstd, float* scale_shift, void* stream);

/* ---- convolution weight gradient  (autograd of the F.conv2d sites above)
 *   dw [Cout][ks][ks][Cin] fp32 (caller zero-fills; accumulated with fp32 atomics),
 *   dbias [Cout] fp32 or NULL (same).  x / scale_shift / act as in mas_conv_fwd
 *   (the activated input is recomputed in the loader, never stored).                   */
int mas_conv_wgrad(const MasConvDesc* d, const void* x, const float* scale_shift, const void* dy,
                   float* dw, float* dbias, void* stream);
/* Commit of a weight gradient: acc = the zero-initialised accumulator handed to mas_conv_wgrad as dw ([Cout][ks][ks][Cin] fp32,
 * immediately followed by [Cout] bias sums when dbias != NULL) -> dw_oihw [Cout][Cin][ks][ks] (nn.Conv2d.weight.grad's layout),
 * dbias [Cout]; acc is zeroed again while it is read, so ONE scratch per stream serves every convolution of a step without fill
 * launches (the caller still owns it).                                                                                              */
int mas_wgrad_commit(float* acc, float* dw_oihw, float* dbias, int Cout, int Cin, int ks, void* stream);
/* Downsample's data gradient without the zero-stuffed tensor (reference models/modules.py:62-81 under autograd): d describes the
 * FORWARD convolution (3x3, stride 2, pads 0); w_packed_t = mas_pack_conv_weight_layout(transpose = 1, MAS_WLAYOUT_K64).           */
int mas_conv_s2_dgrad_supported(const MasConvDesc* d);
int mas_conv_s2_dgrad(const MasConvDesc* d, const void* dy, const void* w_packed_t, void* dx, void* stream);
/* Deterministic split-K (ABI v3): for the convolutions that carry the FLOPs (mas_conv_wgrad_splits(d) = nsplit > 0: bf16, stride 1, no
 * prologue; 3x3 with Cin % 64 == 0, Cout % 128 == 0, or 1x1 with Cin % 128 == 0, Cout % 128 == 0: part is then [nsplit][Cout][ks][ks][Cin]) mas_conv_wgrad_partial writes the nsplit partial sums -- part [nsplit][Cout][3][3][Cin] fp32,
 * part_bias [nsplit][Cout] or NULL, every element exactly once, plain stores, no initialisation required -- and mas_wgrad_reduce adds
 * the slabs in a fixed order into dw_oihw [Cout][Cin][ks][ks] / dbias [Cout]: no atomics, bitwise reproducible run to run.
 * Round 6 (no ABI change): every other geometry mas_conv_wgrad accepts (ks 1..4, stride 1 / 2, bf16 / fp32, prologue or not, Cin % 4 == 0)
 * reports nsplit > 0 too and runs the general kernels in slab mode; 0 is returned only for Cin % 4 != 0 (or MAS_WGRAD_GENERAL_SLABS=0),
 * and only then is mas_conv_wgrad's atomic commit the route.                                                                         */
int mas_conv_wgrad_splits(const MasConvDesc* d);
int mas_conv_wgrad_partial(const MasConvDesc* d, const void* x, const float* scale_shift, const void* dy,
                           float* part, float* part_bias, void* stream);
int mas_wgrad_reduce(const float* part, const float* part_bias, int nsplit, float* dw_oihw, float* dbias, int Cout, int Cin, int ks,
                     void* stream);

/* `Upsample` + convolution in its sub-pixel form (conv_up2.hip; MAS_WLAYOUT_UP2 above): 2.25x fewer FLOPs than the 3x3 convolution over
 * the x2 image.  d describes the FORWARD convolution as for mas_conv_fwd (upsample = 1, H x W the input map, Ho x Wo = 2H x 2W, 3x3,
 * stride 1, pads 1, bf16, no prologue).  Forward: mas_conv_up2_supported(d) != 0 -> pack the weight with MAS_WLAYOUT_UP2, set
 * d->w_layout to it and call mas_conv_fwd / mas_conv_fwd_stats (no residual).  Data gradient with respect to the LOW-resolution input:
 * dx [N,H,W,Cin] from dy [N,Ho,Wo,Cout] and w_packed_t = the MAS_WLAYOUT_UP2 image with transpose = 1 -- replaces the stride-1
 * data-gradient convolution at the high resolution plus the x2 sum-pooling pass.                                                   */
int mas_conv_up2_supported(const MasConvDesc* d);
int mas_conv_up2_dgrad_supported(const MasConvDesc* d);
int mas_conv_up2_dgrad(const MasConvDesc* d, const void* dy, const void* w_packed_t, void* dx, void* stream);
/* The weight gradient of the same layer in the same form (conv_wgrad_dma.hip with 2x2 taps per phase): mas_conv_up2_wgrad_splits(d) =
 * slabs PER PHASE (0: unsupported, take mas_conv_wgrad_partial); mas_conv_up2_wgrad_partial writes part [4][nsplit][Cout][2][2][Cin] fp32
 * and (when non-NULL) part_bias [4 * nsplit][Cout], every element once, plain stores; mas_wgrad_reduce_up2 adds the slabs in a fixed
 * order and folds the 4 x 4 phase taps into dw_oihw [Cout][Cin][3][3] / dbias [Cout] (bitwise reproducible run to run).              */
int mas_conv_up2_wgrad_splits(const MasConvDesc* d);
int mas_conv_up2_wgrad_partial(const MasConvDesc* d, const void* x, const void* dy, float* part, float* part_bias, void* stream);
int mas_wgrad_reduce_up2(const float* part, const float* part_bias, int nsplit, float* dw_oihw, float* dbias, int Cout, int Cin, void* stream);

/* ---- vector quantiser  (replaces Codebook.forward's distance / argmin / gather / loss,
 * modules.py:501-509; never materialises d[M,K]).
 *   z [M][D] fp32 (NHWC latent rows), codebook [K][D] fp32.
 *   idx [M] int64 : argmin_k ( (|z|^2+|e_k|^2) - 2 z.e_k ), first minimum on ties
 *   zq  [M][D] fp32 = codebook[idx]
 *   sqerr [1] fp32 = sum (zq - z)^2      (loss = (1+beta) * sqerr / (M*D), modules.py:509)
 * workspace: mas_vq_workspace(M,K) bytes.                                             */
size_t mas_vq_workspace(int M, int K);
int    mas_vq_argmin_fwd(const float* z, const float* codebook, int M, int K, int D,
                         int64_t* idx, float* zq, float* sqerr, void* workspace, size_t ws_bytes, void* stream);
/* backward of (z_q straight-through, loss):  dz = g_zq + g_loss*2/(M*D)*(z-e[idx]);
 * dcodebook[idx] += g_loss*beta*2/(M*D)*(e[idx]-z).  For D <= 256, D % 4 == 0 (every codebook_dim of mas_vq_argmin_fwd) EVERY row of
 * dcodebook is written, summed in a fixed order (no atomics: bitwise run-to-run deterministic, no zero fill needed); other D add
 * with fp32 atomics into a buffer the caller zero-filled.  g_loss is a device scalar.                                            */
int    mas_vq_bwd(const float* z, const float* codebook, const int64_t* idx, const float* g_zq,
                  const float* g_loss, float beta, int M, int K, int D, float* dz, float* dcodebook, void* stream);

/* ---- causal multi-head self-attention forward (flash style)  (replaces calculate_attention + Softmax +
 * matmul(probs, v), models/transformer.py:44-71,90-97, training configuration: pb-relax shift is softmax-invariant,
 * the net mask is pure causal -- SURVEY 3.4).  q,k,v: element (b, s, h, d) at ptr[b*bs + s*ld + h*hd + d] (so the
 * fused [B,S,3*H*hd] qkv tensor is addressed in place); o: [B,S,H*hd] contiguous; lse: [B,H,S] fp32 (log-sum-exp of
 * the scaled scores, for the backward) or NULL.  hd in {16,32,64,128}.                                          */
int mas_attn_causal_fwd(const void* q, const void* k, const void* v, void* o, float* lse, int dtype, int B, int H,
                        int S, int hd, int ld_q, int ld_k, int ld_v, long long q_bs, long long k_bs, long long v_bs,
                        float scale, void* stream);

/* backward of mas_attn_causal_fwd on the fused projection: qkv and dqkv are [B,S,3*H*hd] contiguous (q|k|v stacked on
 * the last axis), o / dout [B,S,H*hd], lse from the forward, delta [B,H,S] fp32 scratch.  Every element of dqkv is
 * written exactly once (no atomics, deterministic).                                                             */
int mas_attn_causal_bwd(const void* qkv, const void* o, const void* dout, const float* lse, float* delta, void* dqkv,
                        int dtype, int B, int H, int S, int hd, float scale, void* stream);

/* ---- Dropout  (reference models/transformer.py:32,92 attn_drop on the probabilities; models/modules.py:99,127 ResnetBlock dropout)
 * Generator: Philox4x32-10 (Random123), make-a-scene_amd/csrc/mas_philox.h.  seed: DEVICE pointer to two int64 {seed, offset}, read by
 * the kernels (no host synchronisation, safe under graph capture).  key = (lo32(seed), hi32(seed)).  Each call yields 8 16-bit values;
 * slot j is bits 16 (j & 1) .. +15 of output word j >> 1.  An element is kept iff its value >= t = round(p * 65536) (p quantised to
 * 1/65536), kept values are scaled by 65536 / (65536 - t); p = 1 (t = 65536) gives zeros.  p in [0, 1].
 *   attention (b, h, query, key), bh = b*H + h:  counter = (key >> 2, query >> 1, bh, lo32(offset)),  slot = 4 (query & 1) + (key & 3)
 *     -- one call per (bh, 4-query block, 4-key block, query half), independent of any kernel's tiling.
 *   element-wise, flat index i (memory order):    counter = (lo32(i >> 3), hi32(i >> 3), 0, lo32(offset)),  slot = i & 7.
 * mas_attn_causal_fwd_drop / _bwd_drop: mas_attn_causal_fwd / _bwd with O = (P o Z s) V; dV = (P o Z s)^T dO, dS = P o (dP o Z s - D)
 * scale; lse and D are those of the undropped P.  The backward regenerates Z: nothing [S, S] is stored.  Same envelope as the plain
 * entries (bf16 head width 128 forward: the generic kernel).
 * mas_attn_dropout_mask: keep[b, h, query, key] (uint8 0 / 1, [B,H,S,S] contiguous) for tests and debugging.
 * mas_dropout_apply: y = x o Z s over n elements (x, y 16-byte aligned; y may be x); its own backward with the same seed.            */
int mas_attn_causal_fwd_drop(const void* q, const void* k, const void* v, void* o, float* lse, int dtype, int B, int H,
                             int S, int hd, int ld_q, int ld_k, int ld_v, long long q_bs, long long k_bs, long long v_bs,
                             float scale, float p, const int64_t* seed, void* stream);
int mas_attn_causal_bwd_drop(const void* qkv, const void* o, const void* dout, const float* lse, float* delta, void* dqkv,
                             int dtype, int B, int H, int S, int hd, float scale, float p, const int64_t* seed, void* stream);
int mas_attn_dropout_mask(const int64_t* seed, int B, int H, int S, float p, uint8_t* keep, void* stream);
int mas_dropout_apply(const void* x, void* y, long long n, int dtype, float p, const int64_t* seed, void* stream);

/* ---- single-head spatial self-attention core of AttnBlock  (replaces the two torch.bmm + softmax of models/modules.py:174-187 and
 * their autograd).  qkv: [N, S, 3C] bf16, q | k | v stacked on the channel axis (the fused 1x1 projection, NHWC with S = h*w);
 * out [N, S, C] = softmax_keys(q k^T * C^-1/2) v;  lse [N, S] fp32 (log-sum-exp of the scaled scores; may be NULL when no backward
 * follows).  Backward: dout [N, S, C] -> dqkv [N, S, 3C] (every element written exactly once, no atomics); delta [N, S] fp32 scratch.
 * bf16 only, S <= 256 tokens, C <= 512 and C % 32 == 0 (the reference's blocks: 16x16x512, 8x8x512).                                */
int mas_spatial_attn_fwd(const void* qkv, void* out, float* lse, int dtype, int N, int S, int C, void* stream);
int mas_spatial_attn_bwd(const void* qkv, const void* dout, const float* lse, float* delta, void* dqkv, int dtype, int N, int S, int C,
                         void* stream);
/* The same core beyond 256 tokens (the 512^2 model's AttnBlocks see 32x32 = 1024): an online softmax over 256-key chunks, so the scores
 * are bounded by nothing in LDS and no [S, S] tensor exists.  Same layouts and conventions as the pair above; 1 <= S <= 4096, C <= 512,
 * C % 32 == 0, bf16 only.  Forward: out [N, S, C], lse [N, S] fp32 (NULL when no backward follows).  Backward: two launches, both
 * recomputing the probabilities from lse; it also takes `out`, the forward's output, because delta = rowsum(dout o out) has to exist
 * before the first key chunk (delta [N, S] fp32 is written by the first launch and read by the second).  dqkv [N, S, 3C]: every element
 * written exactly once, no atomics, results repeat bit for bit.  Not bit-equal to the pair above at S <= 256: the probabilities are
 * rounded to bf16 before the normalisation here and after it there.                                                                  */
int mas_spatial_attn_flash_fwd(const void* qkv, void* out, float* lse, int dtype, int N, int S, int C, void* stream);
int mas_spatial_attn_flash_bwd(const void* qkv, const void* out, const void* dout, const float* lse, float* delta, void* dqkv, int dtype,
                               int N, int S, int C, void* stream);

/* ---- decode-time (KV-cached) attention  (replaces the cached branch of SelfAttention.forward, models/transformer.py:73-115,
 * for token-by-token sampling: SURVEY 8(f) rank 3).  nq new queries of every (batch, head) against a cache of past + nq keys /
 * values: query i (0 <= i < nq) attends to keys 0 .. past + i (causal inside the block).  q: element (b, i, h, d) at
 * q[b*q_bs + i*ld_q + h*hd + d]; k_cache / v_cache: element (b, s, h, d) at ptr[b*bs + s*ld + h*hd + d], rows 0 .. past+nq-1
 * valid (the caller appends the new rows BEFORE the call); o likewise with (o_bs, ld_o).  HBM-bound: each key / value row is
 * read once per query; no [nq, S] score tensor exists.  hd in {16,32,64,128}; rows 16-byte aligned.                        */
int mas_attn_decode(const void* q, const void* k_cache, const void* v_cache, void* o, int dtype, int B, int H, int nq,
                    int past, int hd, int ld_q, int ld_k, int ld_v, int ld_o, long long q_bs, long long k_bs,
                    long long v_bs, long long o_bs, float scale, void* stream);

/* ---- one decode step with device-resident state (MakeAScene.generate(graph=True), models/decode_graph.py): every per-token value is read
 * from device memory, so a captured graph of the step is replayed once per token.  Step counters: int32 ctr[2] = {k, past}, k the image
 * token the step samples, past = (prompt length) + k - 1 the cache row it appends; mas_decode_advance adds 1 to both after the step.
 * mas_attn_decode_dev: mas_attn_decode with nq = 1 whose cache length is *past (device) and which appends the new row itself: q, k_new,
 *   v_new are the new row's projections (element (b, h, d) at ptr[b*new_bs + h*hd + d]), the block of (b, h) writes k_new / v_new into
 *   cache row *past and attends to rows 0 .. *past.  Same key-to-lane assignment and merge order as mas_attn_decode: the output is bit
 *   for bit that of mas_attn_decode on a cache where the row was appended beforehand.  The grid is B*H, independent of *past; when
 *   *past is outside [0, capacity) the kernel reads and writes nothing (o is left as it was).  hd in {16,32,64,128}; rows 16-byte aligned.
 * mas_decode_embed: out[r, :] (fp32 [rows, D], rows = B or 2B under guidance) = img_emb[t] + (row_emb[i / n] + col_emb[i % n]),
 *   i = *step - 1, t = tokens[(r % B) * ld_tok + i] (int64): the eager image embedding of the previous step's token.  A token outside
 *   [0, vocab) or i outside [0, n*n) writes a NaN row and reads nothing else.  Embedding tables fp32 [*, D].
 * mas_sample_tokens: one work-group per output row r < B, step k = *step (nothing when k is outside [0, L)).  logits fp32, row r at
 *   logits + r*ld_logits (ld_logits may be 0: every row reads the same logits); with guided != 0 the unconditional row is uncond_off
 *   elements further and the row is l = lu + s*(lc - lu) (fp32, no contraction; params = {temperature, s} on the device).  logits_out
 *   (may be NULL): l goes to logits_out[r*ld_logits_out + k*V + j].  mode 2: tokens[r, k] = forced[r*ld_forced + k]; mode 0: the first
 *   index of max l (torch.argmax); mode 1: lg = l / temperature, kth = the top_k-th largest lg (top_k <= 0 or >= V: no cut), and the
 *   token is argmax over {j : lg_j >= kth} of lg_j - log(-log u_j) (Gumbel-max: an exact draw from softmax(lg) restricted to the kept
 *   entries; ties at kth are kept; lowest index on equal scores), u_j from the Sampling mapping below.  tokens int64, row stride ld_tokens.
 * Sampling mapping: seed = DEVICE pointer to int64 {seed, offset} (as for Dropout), key = (lo32(seed), hi32(seed));  u_j of row r at
 *   step k:  counter = (j >> 2, k, r, lo32(offset)),  32-bit slot j & 3 (words x, y, z, w),  u = ((bits >> 9) + 0.5) * 2^-23
 *   (exact in float32, in [2^-24, 1 - 2^-24]: never 0 or 1, so every score is finite).
 *   (make-a-scene_amd/csrc/mas_philox.h: mas_sample_bits4, mas_sample_uniform.)
 * Top-p: mas_sample_tokens_topp is mas_sample_tokens with params = {temperature, s, top_p} (three device floats); both launch the same
 *   kernel.  In mode 1, with K = {j : lg_j >= kth} the set top-k keeps (everything when top-k is off), q = softmax(lg restricted to K)
 *   and M_>(x) = the sum of q_i over i in K with lg_i > x (strict), entry j stays iff j is in K and M_>(lg_j) <= top_p: the usual
 *   nucleus rule (drop the sorted entries whose inclusive cumulative probability exceeds top_p, shifted by one so that the first one
 *   over the line stays) stated on values.  The maximum and its ties always stay; the kept set is {lg_j >= t*} for one value t*, ties
 *   at t* kept; top-k first, then top-p on the re-normalised masses.  The token is the Gumbel-max draw over the kept set, same mapping.
 *   !(top_p < 1) (1, more, NaN) is off: the instructions and tokens of mas_sample_tokens.  top_p <= 0 keeps the maximum and its ties.
 *   Modes 0 and 2 ignore it.  t* comes from a radix select over fixed-point masses floor(exp(lg_j - max) * 2^32) summed as 64-bit
 *   integers: repeatable bit for bit, exact line for V < 2^21; an entry 2^-32 below the maximum weighs nothing (it can still be kept).
 * Image prompt: mas_sample_tokens_prompt is mas_sample_tokens_topp (params = three device floats, top_p = 1 for "off") with a per-row
 *   mask, keep uint8, row r at keep + r*ld_keep (ld_keep >= L): after the logits write-out the work-group of a row with
 *   keep[r*ld_keep + k] != 0 stores tokens[r, k] = forced[r*ld_forced + k] and returns; every other row goes on as in mode 0 / 1.  The
 *   same kernel: a free row's token is the one mas_sample_tokens_topp gives (the Philox counter holds the row, the step and the
 *   vocabulary slot, nothing about the other rows or steps).  Modes 0 and 1 only, keep and forced required: anything else is MAS_EINVAL.
 * mas_decode_advance: counters[0 .. n-1] += 1 (one thread, n <= 8), ordered after the step's kernels by the stream.                  */
int mas_attn_decode_dev(const void* q, const void* k_new, const void* v_new, long long new_bs, void* k_cache, void* v_cache, int ld_c,
                        long long c_bs, int capacity, void* o, long long o_bs, int dtype, int B, int H, int hd, const int32_t* past,
                        float scale, void* stream);
int mas_decode_embed(const int64_t* tokens, long long ld_tok, const int32_t* step, const float* img_emb, int vocab, const float* row_emb,
                     const float* col_emb, int n, float* out, int B, int rows, int D, void* stream);
int mas_sample_tokens(const float* logits, long long ld_logits, long long uncond_off, int B, int V, int guided, int mode, int top_k,
                      const float* params, const int64_t* seed, const int32_t* step, int L, const int64_t* forced, long long ld_forced,
                      int64_t* tokens, long long ld_tokens, float* logits_out, long long ld_logits_out, void* stream);
int mas_sample_tokens_topp(const float* logits, long long ld_logits, long long uncond_off, int B, int V, int guided, int mode, int top_k,
                           const float* params, const int64_t* seed, const int32_t* step, int L, const int64_t* forced,
                           long long ld_forced, int64_t* tokens, long long ld_tokens, float* logits_out, long long ld_logits_out,
                           void* stream);
int mas_sample_tokens_prompt(const float* logits, long long ld_logits, long long uncond_off, int B, int V, int guided, int mode, int top_k,
                             const float* params, const int64_t* seed, const int32_t* step, int L, const int64_t* forced,
                             long long ld_forced, int64_t* tokens, long long ld_tokens, float* logits_out, long long ld_logits_out,
                             const uint8_t* keep, long long ld_keep, void* stream);
int mas_decode_advance(int32_t* counters, int n, void* stream);

/* ---- decode attention split over keys (low batch * heads: make-a-scene_amd/csrc/attn_decode_split.hip).  mas_attn_decode /
 * mas_attn_decode_dev run one work-group per (row, head); these run nsplit of them over contiguous key ranges and a second small launch
 * that merges their states, nq = 1 only.  With L = past + 1 visible keys, split s owns keys [s*chunk, min(L, (s+1)*chunk)), chunk =
 * ceil(L / nsplit) rounded up to 32 keys (computed on the device); it writes its un-normalised online-softmax state {o[hd], m, l} (fp32;
 * m = -1e30, l = 0, o = 0 when it has no key) to workspace[((b*H + h)*nsplit + s)*(hd + 2)], and the combine launch takes the common
 * maximum, rescales and adds in split order, divides and writes o.  Fixed orders throughout: the same inputs give the same bits; the
 * bits are not those of the unsplit kernels (another summation order, within the same tolerance).
 * workspace: device fp32, at least B*H*nsplit*(hd + 2) floats (workspace_floats is checked: MAS_EWORKSPACE), owned by the caller, free
 *   to reuse once the call's work on `stream` is done (calls on one stream may share it).  1 <= nsplit <= MAS_ATTN_DECODE_MAX_SPLITS;
 *   B*H <= 65535; hd in {16,32,64,128}; rows 16-byte aligned.
 * mas_attn_decode_split: the arguments and layout of mas_attn_decode (rows 0 .. past valid: the caller appends the new row BEFORE the
 *   call); nq must be 1 (MAS_EINVAL otherwise).
 * mas_attn_decode_split_dev: the arguments and contract of mas_attn_decode_dev: *past on the device, the new k / v row appended to cache
 *   row *past by the one work-group of each (b, h) whose key range holds it, before that work-group loads any key; *past outside
 *   [0, capacity): nothing read or written, workspace and o included.  Bit for bit the output of mas_attn_decode_split with the same
 *   nsplit on a cache where the row was appended beforehand (the same two kernels).                                                  */
#define MAS_ATTN_DECODE_MAX_SPLITS 32
int mas_attn_decode_split(const void* q, const void* k_cache, const void* v_cache, void* o, int dtype, int B, int H, int nq, int past,
                          int hd, int ld_q, int ld_k, int ld_v, int ld_o, long long q_bs, long long k_bs, long long v_bs, long long o_bs,
                          float scale, int nsplit, float* workspace, size_t workspace_floats, void* stream);
int mas_attn_decode_split_dev(const void* q, const void* k_new, const void* v_new, long long new_bs, void* k_cache, void* v_cache,
                              int ld_c, long long c_bs, int capacity, void* o, long long o_bs, int dtype, int B, int H, int hd,
                              const int32_t* past, float scale, int nsplit, float* workspace, size_t workspace_floats, void* stream);

/* ---- decode attention for candidates that share a prompt (generate(num_samples=n): make-a-scene_amd/csrc/attn_decode_shared.hip).
 * rows = groups * group cache rows, one new query row each (nq = 1); the `group` consecutive rows r with r / group == g are candidates
 * for one prompt.  The keys live in two places:
 *   prompt_k / prompt_v  [groups, prompt_len, H*hd]: read-only, block g shared by the rows of group g; ld_p elements between tokens, p_bs
 *                        between blocks (views into a larger buffer are fine).
 *   k_cache / v_cache    [rows, capacity, H*hd]: each row's image positions only; ld_c between tokens, c_bs between rows.
 * Query r attends to the prompt_len keys of block r / group and to its own keys 0 .. past - prompt_len.  `past` keeps the meaning it has
 * in every decode entry -- the number of positions before the new row, prompt included -- so a step counter serves both layouts.
 * Two launches on `stream`, no parallel branch: "partial" -- groups*H*ceil(group / QT)*nsplit_prompt work-groups that walk one range of
 * the prompt's keys for QT = MAS_ATTN_DECODE_SHARED_QT rows of a group at once (every 16-byte unit of a key row loaded once for the
 * QT queries; ranges: chunks of ceil(prompt_len / nsplit_prompt) rounded up to 32 keys) and rows*H*nsplit_own work-groups that walk a row's own L_own = past -
 * prompt_len + 1 keys (chunks of ceil(L_own / nsplit_own) rounded up to 32, as mas_attn_decode_split) -- and "combine", which merges the
 * nsplit_prompt + nsplit_own states {o[hd], m, l} of workspace[(r*H + h)][s] in a fixed order: prompt ranges, then own ranges.
 * The same inputs give the same bits; a row's bits depend on its query, its prompt block and its own cache alone (not on its place in
 * the group, nor on other groups); they are not the bits of mas_attn_decode / _split on a concatenated cache (another summation order,
 * the same tolerance).
 * workspace: device fp32, at least rows*H*(nsplit_prompt + nsplit_own)*(hd + 2) floats (MAS_EWORKSPACE), the caller's, reusable by the
 *   next call on the stream.  Each split count in [1, MAS_ATTN_DECODE_MAX_SPLITS]; group >= 1, rows % group == 0, prompt_len >= 1
 *   (MAS_EINVAL); hd in {16,32,64,128}; dtype bf16 or fp32; rows 16-byte aligned (MAS_EUNSUPPORTED).  Nothing is launched on an error.
 * mas_attn_decode_shared: host `past` in [prompt_len, prompt_len + capacity) (MAS_EINVAL otherwise); own rows 0 .. past - prompt_len
 *   valid: the caller appends the new row BEFORE the call.  q: row r at q + r*q_bs.
 * mas_attn_decode_shared_dev: *past on the device; the new k / v row (row r at k_new + r*new_bs, q likewise) is appended to own cache
 *   row *past - prompt_len by the one work-group of each (r, h) whose range holds it, before that work-group loads any key.  *past <
 *   prompt_len or *past - prompt_len >= capacity: every work-group returns at once; caches, workspace and o untouched.  Bit for bit the
 *   output of mas_attn_decode_shared on a cache where the row was appended beforehand (the same two kernels).                        */
#define MAS_ATTN_DECODE_SHARED_QT 4
int mas_attn_decode_shared(const void* q, long long q_bs, const void* prompt_k, const void* prompt_v, int ld_p, long long p_bs,
                           int prompt_len, const void* k_cache, const void* v_cache, int ld_c, long long c_bs, int capacity, void* o,
                           long long o_bs, int dtype, int rows, int group, int H, int hd, int past, float scale, int nsplit_prompt,
                           int nsplit_own, float* workspace, size_t workspace_floats, void* stream);
int mas_attn_decode_shared_dev(const void* q, const void* k_new, const void* v_new, long long new_bs, const void* prompt_k,
                               const void* prompt_v, int ld_p, long long p_bs, int prompt_len, void* k_cache, void* v_cache, int ld_c,
                               long long c_bs, int capacity, void* o, long long o_bs, int dtype, int rows, int group, int H, int hd,
                               const int32_t* past, float scale, int nsplit_prompt, int nsplit_own, float* workspace,
                               size_t workspace_floats, void* stream);

/* ---- small NHWC helpers on the path -------------------------------------------------
 * nearest x2 upsample (F.interpolate, modules.py:56) and its adjoint (2x2 sum);
 * zero-stuffing used by the stride-2 data gradient (adjoint of modules.py:76-78).      */
int mas_upsample2x(const void* x, void* y, int dtype, int N, int H, int W, int C, void* stream);
int mas_sumpool2x(const void* x, void* y, int dtype, int N, int Ho, int Wo, int C, void* stream);
int mas_zero_stuff2x(const void* x, void* y, int dtype, int N, int H, int W, int C, int Hout, int Wout, void* stream);
/* y[n][h'][w'][(dy*2+dx)*C + c] = x[n][2h'+dy-pad][2w'+dx-pad][c] (0 outside), y is [N,Ho,Wo,4C]: a stride-2 K x K convolution of x
 * equals the stride-1 (K/2) x (K/2) convolution of y -- the weight gradient of the discriminator's 4x4 stride-2 convolutions
 * (losses/discriminator.py:20,27) runs as mas_conv_wgrad with ks = 2 on y.                                                       */
int mas_space_to_depth2x(const void* x, void* y, int dtype, int N, int H, int W, int C, int Ho, int Wo, int pad, void* stream);

/* -------------------------------------------------------------------------------------------
 * Transformer row operators (streaming, HBM-bound).
 * mas_gelu_tanh_*: OpenAI tanh-GELU of reference models/transformer.py:11-14 (MLP.forward :129) over n elements.
 * mas_layernorm_*: torch.nn.LayerNorm(D, eps) as used four times per TransformerLayer
 *   (models/transformer.py:159-163,197-210), rows x D, with an optional fused residual  y = residual + LN(x)
 *   (residual / y / dy have out_dtype; x / dx have in_dtype; gamma, beta, dgamma, dbeta fp32).
 *   mean_rstd [rows][2] fp32 is written by the forward (may be NULL when no backward follows) and read by the
 *   backward.  D must be a multiple of the 16-byte vector (8 for bf16->bf16, else 4) and at most 256 vectors.      */
int mas_gelu_tanh_fwd(const void* x, void* y, int dtype, long long n, void* stream);
int mas_gelu_tanh_bwd(const void* x, const void* dy, void* dx, int dtype, long long n, void* stream);
/* mas_gelu_tanh_bwd_colsum (ABI v9): mas_gelu_tanh_bwd over a [rows][cols] tensor that ALSO returns dx_colsum[cols] (fp32) = the column sums of
 *   the dx it writes (as stored; fixed summation order): the bias gradient of the Linear layer that produced x (`lin1`, reference
 *   models/transformer.py:125,129: grad_bias = grad_output.sum(0) with grad_output = this dx), otherwise a mas_colsum pass over dx.
 *   cols % 8 == 0 (bf16) / % 4 (fp32); workspace: mas_gelu_tanh_bwd_colsum_workspace bytes (0 = shape not supported), caller-owned.                */
size_t mas_gelu_tanh_bwd_colsum_workspace(int dtype, int cols);
int mas_gelu_tanh_bwd_colsum(const void* x, const void* dy, void* dx, float* dx_colsum, int dtype, long long rows, int cols, void* workspace,
                             size_t workspace_bytes, void* stream);
int mas_layernorm_fwd(const void* x, const float* gamma, const float* beta, const void* residual, void* y,
                      float* mean_rstd, int in_dtype, int out_dtype, int rows, int D, float eps, void* stream);
size_t mas_layernorm_bwd_workspace(int rows, int D);
int mas_layernorm_bwd(const void* x, const void* dy, const float* gamma, const float* mean_rstd, void* dx,
                      float* dgamma, float* dbeta, int in_dtype, int out_dtype, int rows, int D,
                      void* workspace, size_t workspace_bytes, void* stream);

/* mas_layernorm_bwd_add: mas_layernorm_bwd with dx = (LayerNorm input gradient) + dx_add -- dx_add [rows][D] in in_dtype is the
 *   gradient that reached x along its skip connection (x feeds the pre-LayerNorm AND the residual of the block's sandwich
 *   LayerNorm, reference models/transformer.py:197-210): one pass instead of the backward plus a separate add.  dx_add NULL =
 *   mas_layernorm_bwd; dx_add may alias dx.                                                                                  */
int mas_layernorm_bwd_add(const void* x, const void* dy, const float* gamma, const float* mean_rstd, const void* dx_add, void* dx,
                          float* dgamma, float* dbeta, int in_dtype, int out_dtype, int rows, int D,
                          void* workspace, size_t workspace_bytes, void* stream);

/* mas_layernorm_bwd_colsum: mas_layernorm_bwd_add that ALSO returns dx_colsum[D] (fp32) = the column sums of dx as stored (rounded to
 *   in_dtype; fixed summation order) -- the bias gradient of the Linear layer whose output this LayerNorm normalises (out_proj / lin2
 *   in front of the sandwich LayerNorms, reference models/transformer.py:201-203,207-209: grad_bias = grad_output.sum(0) with
 *   grad_output = this dx), which otherwise costs a mas_colsum pass over dx.  dx_colsum NULL = mas_layernorm_bwd_add.             */
int mas_layernorm_bwd_colsum(const void* x, const void* dy, const float* gamma, const float* mean_rstd, const void* dx_add, void* dx,
                             float* dgamma, float* dbeta, float* dx_colsum, int in_dtype, int out_dtype, int rows, int D,
                             void* workspace, size_t workspace_bytes, void* stream);

/* mas_token_ce_* (ABI v9): the stage-2 objective, F.cross_entropy(pred_logit.view(-1, V), img_token.view(-1)) of reference train.py:152 for
 *   class-index targets, with ignore_index and label smoothing, on fp32 or bf16 logits read IN PLACE: row r of `rows` starts at element
 *   logits + (r / inner) * outer_stride + (r % inner) * ld and holds V contiguous classes (a contiguous matrix: inner = rows,
 *   outer_stride = 0, ld = V; the [B, L, V] slice of a [B, S, V] tensor: inner = L, outer_stride = S * V, ld = V).  V any positive int,
 *   rows * V may exceed 2^31.  Rows that start on a 16-byte boundary are read in 16-byte units, their tail V % (16 / sizeof) and every
 *   other row element by element.  target int64 [rows]; target == ignore_index: row loss 0 and a zero gradient row; any other target outside
 *   [0, V): NaN in that row's loss and gradient row (no load is indexed by a target value).  Arithmetic fp32; no atomics: results repeat bit
 *   for bit.  No host synchronisation: the three calls capture into a graph.
 *   mas_token_ce_fwd: one pass.  row_loss [rows] fp32 = (1 - eps) ((m - x_t) + log l) + eps ((m - mean_j x_j) + log l) with m = max_j x_j,
 *     l = sum_j exp(x_j - m); stats [rows][2] fp32 = {m, log l} for the backward (kept apart: m + log l would round at large logits).
 *   mas_token_ce_reduce: reduction MAS_CE_MEAN | MAS_CE_SUM: out[0] = the sum of row_loss in fp64, fixed order (MEAN: divided by the count),
 *     out[1] = the count of rows whose target is not ignore_index, both fp32 on the device; all rows ignored: MEAN gives NaN.
 *   mas_token_ce_bwd: dx [rows][V] contiguous, in the logits' dtype (rounded once), dx_j = w_r (exp((x_j - m) - log l) - (1 - eps) [j = t]
 *     - eps / V); w_r = grad[0] (MAS_CE_SUM), grad[0] / loss_count[1] (MAS_CE_MEAN; loss_count = the reduce call's out), grad[r]
 *     (MAS_CE_NONE); grad fp32 on the device.                                                                                          */
enum { MAS_CE_NONE = 0, MAS_CE_MEAN = 1, MAS_CE_SUM = 2 };
int mas_token_ce_fwd(const void* logits, int dtype, long long rows, int V, long long inner, long long outer_stride, long long ld,
                     const int64_t* target, long long ignore_index, float label_smoothing, float* row_loss, float* stats, void* stream);
int mas_token_ce_reduce(const float* row_loss, const int64_t* target, long long rows, long long ignore_index, int reduction, float* out,
                        void* stream);
int mas_token_ce_bwd(const void* logits, int dtype, long long rows, int V, long long inner, long long outer_stride, long long ld,
                     const int64_t* target, long long ignore_index, float label_smoothing, const float* stats, const float* grad,
                     const float* loss_count, int reduction, void* dx, void* stream);

/* mas_seg_loss_* (additions under ABI 10): the VQ-SEG objective of reference losses/loss_seg.py:6-41 in one pass each way.  For x = the
 *   prediction logits [N, C, H, W], t = the target of the same shape, w = pos_weight [C] fp32 (any content) and n = N C H W:
 *     lw = 1 + (w[c] - 1) t;  bce = (1 - t) x + lw softplus(-x);  mse = (sigmoid(x) - t)^2;  loss = mean(bce) + mse_on mean(mse)
 *     dx = g / n [ (1 - t) - lw (1 - sigmoid(x)) + mse_on 2 (sigmoid(x) - t) sigmoid(x) (1 - sigmoid(x)) ]
 *   = F.binary_cross_entropy_with_logits(pos_weight = w) (+ F.mse_loss(sigmoid(x), t)), from one exp(-|x|) per element: finite for any
 *   finite x.  x fp32 or bf16 (MAS_F32 / MAS_BF16); t fp32, bf16 or MAS_SEG_U8 (bool: 0 / 1 bytes).  Each tensor is DENSE and on its own
 *   MAS_SEG_NCHW or MAS_SEG_NHWC (channels_last memory); neither is copied, base pointers need the element's alignment only, n may
 *   exceed 2^31 (H W <= 2^30; C <= 15360 when both tensors have the same layout, C <= 7679 when they differ: the weights, and then one
 *   pixel of targets beside them, must fit in LDS; beyond that MAS_EUNSUPPORTED).  Arithmetic fp32, sums fp64 across tiles, lanes and work-groups; no atomics, and the grid depends
 *   on the shape and the CU count alone: results repeat bit for bit.  No host synchronisation: the calls capture into a graph.
 *   mas_seg_loss_blocks: the work-groups of the forward = the {bce_sum, mse_sum} fp64 pairs `partials` must hold (negative: an error code).
 *   mas_seg_loss_fwd: partials[b] = work-group b's two sums.  mas_seg_loss_reduce: ONE work-group adds partial_pairs pairs in a fixed
 *     order -> out[0..2] = {loss, mean(bce), mse_on mean(mse)} fp32 on the device, each rounded once from fp64.
 *   mas_seg_loss_bwd: dx in x's dtype (rounded once) and x's layout; grad = the upstream gradient g, one fp32 on the device.        */
enum { MAS_SEG_NCHW = 0, MAS_SEG_NHWC = 1 };
enum { MAS_SEG_U8 = 2 };      /* target dtype beside MAS_F32 / MAS_BF16 */
int mas_seg_loss_blocks(int N, int C, int H, int W, int x_dtype, int x_layout, int t_layout);
int mas_seg_loss_fwd(const void* x, int x_dtype, int x_layout, const void* t, int t_dtype, int t_layout, const float* pos_weight,
                     int N, int C, int H, int W, int mse_on, double* partials, int partial_pairs, void* stream);
int mas_seg_loss_reduce(const double* partials, int partial_pairs, long long numel, int mse_on, float* out, void* stream);
int mas_seg_loss_bwd(const void* x, int x_dtype, int x_layout, const void* t, int t_dtype, int t_layout, const float* pos_weight,
                     int N, int C, int H, int W, int mse_on, const float* grad, void* dx, void* stream);

/* mas_seg_expand, mas_seg_loss_labels_* (additions under ABI 10): the VQ-SEG map as LABEL PLANES instead of a one-hot tensor.
 *   planes: uint8 [N, P, H, W] dense, P = n_groups + value_channels <= 8.  Plane g < n_groups is a class label: 0 sets nothing, v in
 *   1..groups[g] sets channel base_g + v - 1 to 1 (base_g = groups[0] + ... + groups[g - 1]), anything above groups[g] sets nothing.
 *   Plane n_groups + k holds the VALUE of channel sum(groups) + k as a byte.  C = sum(groups) + value_channels; 1 <= groups[g] <= 255;
 *   `groups` is a host array.  Nothing is addressed through a label: a pixel's P bytes become at most P {channel, value} pairs that the
 *   channels of the output (or of the prediction) are compared with.
 *   mas_seg_expand: the dense map, NHWC (out_layout MAS_SEG_NHWC: [N, H, W, C_pad], channels C..C_pad - 1 exact zeros, C_pad >= C) or NCHW
 *     ([N, C_pad, H, W]), fp32 or bf16; written in 16-byte units where `out` is 16-byte aligned and C_pad (NHWC) or H W (NCHW) is a
 *     multiple of the unit, one element at a time otherwise.
 *   mas_seg_loss_labels_fwd / _bwd: the loss and gradient of mas_seg_loss_fwd / _bwd (the same per-element code) with the target derived
 *     in registers from the planes; x (and dx) fp32 or bf16, dense NCHW or NHWC, element alignment only.  A work-group takes tiles of
 *     MAS_SEG_LABELS_TILE pixels of one image x all channels and reads a tile's labels once.  partials / mas_seg_loss_reduce / grad as
 *     above; mas_seg_loss_labels_blocks sizes grid and workspace (negative: an error code).  No atomics, no host synchronisation.     */
enum { MAS_SEG_LABELS_TILE = 256, MAS_SEG_MAX_PLANES = 8 };
int mas_seg_expand(const unsigned char* planes, const int* groups, int n_groups, int value_channels, int N, int H, int W, void* out,
                   int out_dtype, int out_layout, int C_pad, void* stream);
int mas_seg_loss_labels_blocks(const int* groups, int n_groups, int value_channels, int N, int H, int W, int x_dtype, int x_layout);
int mas_seg_loss_labels_fwd(const void* x, int x_dtype, int x_layout, const unsigned char* planes, const int* groups, int n_groups,
                            int value_channels, const float* pos_weight, int N, int H, int W, int mse_on, double* partials,
                            int partial_pairs, void* stream);
int mas_seg_loss_labels_bwd(const void* x, int x_dtype, int x_layout, const unsigned char* planes, const int* groups, int n_groups,
                            int value_channels, const float* pos_weight, int N, int H, int W, int mse_on, const float* grad, void* dx,
                            void* stream);

/* mas_seg_classify, mas_seg_agreement (additions under ABI 10): VQ-SEG logits BACK to the label planes above, and the integer counts that
 *   pixel accuracy and per-class IoU are made of.  planes / groups / n_groups / value_channels / C as for mas_seg_expand.
 *   mas_seg_classify: x = logits [N, C, H, W], fp32 or bf16, dense MAS_SEG_NCHW or MAS_SEG_NHWC, element alignment only -> planes uint8
 *     [N, P, H, W].  tau: HOST array of P fp32 thresholds ON THE LOGIT, tau = log(t / (1 - t)) for a probability t, -INFINITY for none
 *     (NaN: MAS_EINVAL).  Class plane g: m = the largest logit of channels base_g .. base_g + groups[g] - 1, a = the FIRST channel that
 *     holds it (torch.argmax's rule); byte = m > tau[g] ? a - base_g + 1 : 0.  Value plane: byte = x > tau ? 1 : 0.  This is the rule of
 *     reference log_utils.py:55-67 (argmax one-hot, times `sigmoid > 0.2` for face and edges: tau = {-inf, -inf, log 0.25, log 0.25}).
 *     Logits are compared as fp32 (bf16 widens exactly): the bytes are exact for every finite and infinite input; with a NaN in a group
 *     the byte is unspecified but within 0 .. groups[g].  x is read once and nothing of its size is held; 16-byte loads where x is 16-byte
 *     aligned, planes 8-byte aligned and H W a multiple of the unit (NCHW) or always, with head and tail (NHWC); 64-bit offsets.
 *   mas_seg_agreement: pred, target = two plane tensors of one layout -> counts, device int64 [3 C + P + 1], ADDED to what it holds:
 *     counts[0 .. C - 1] = inter, [C .. 2 C - 1] = pred, [2 C .. 3 C - 1] = target, per channel: for the class channel base_g + v - 1 the
 *     pixels whose pred byte / target byte / both equal v, for a value channel the pixels whose byte is > 0 (a target edge value of 2
 *     counts as set); counts[3 C + k] = the pixels where plane k of the two says the same (class planes: equal bytes after bytes above
 *     groups[k] became 0; value planes: equal `> 0`); counts[3 C + P] += N H W.  A byte addresses a counter only after 1 <= v <= groups[g].
 *     Integer sums only (LDS histograms, then 64-bit integer atomics): exact, and independent of any order.  counts 8-byte aligned.
 *   Both: no host synchronisation (they capture into a graph), grids from the shape and the CU count.  Null arguments: MAS_EINVAL.  More
 *     than MAS_SEG_MAX_PLANES planes, a group above 255, H W > 2^30, more than 4e18 logits, N H W > 2^32 (agreement): MAS_EUNSUPPORTED. */
int mas_seg_classify(const void* x, int x_dtype, int x_layout, const int* groups, int n_groups, int value_channels, const float* tau,
                     int N, int H, int W, unsigned char* planes, void* stream);
int mas_seg_agreement(const unsigned char* pred, const unsigned char* target, const int* groups, int n_groups, int value_channels,
                      int N, int H, int W, long long* counts, void* stream);

/* mas_img_bytes, mas_img_agreement*, mas_code_usage (additions under ABI 10): the VQ-IMG read-out -- float images to uint8 pictures, the
 *   squared error and SSIM between two pictures, and how often each code of the codebook is used.
 *   mas_img_bytes: x [N, C, H, W], fp32 or bf16, dense MAS_SEG_NCHW or MAS_SEG_NHWC, element alignment only, 1 <= C <=
 *     MAS_IMG_MAX_CHANNELS -> out uint8 [N, H, W, C] (interleaved).  With s = (float)(255.0 / (hi - lo)) and (float)lo, per element in fp32,
 *     every operation rounded on its own (no fused multiply-add):  t = (x - lo) * s;  t = fmin(fmax(t, 0), 255), a NaN gives 0;
 *     byte = rint(t), half to even.  lo < hi, both finite (else MAS_EINVAL).  x is read once, in 16-byte loads where it is 16-byte aligned
 *     (NCHW: and H W a multiple of the unit), with head and tail element by element (NHWC).
 *   mas_img_agreement: a, b = two pictures uint8 [N, H, W, C] ->
 *       sse[n] += sum over H W C of (a - b)^2, device int64 [N] (64-bit integer atomics: exact in any order; zero it first);
 *       partials[n][ty][tx] = the fp64 sum of the SSIM map over tile (ty, tx) of image n, device fp64 [mas_img_agreement_blocks()].
 *     SSIM is Wang et al. 2004 in its "valid" form on the bytes 0 .. 255: `window` = HOST array of MAS_IMG_SSIM_WINDOW fp64 weights g (the
 *     caller normalises exp(-(i - 5)^2 / (2 1.5^2)) to sum 1; the 2-D window is g x g), C1 = (0.01 255)^2, C2 = (0.03 255)^2, no padding:
 *     for every channel and each of the (H - 10)(W - 10) window positions mu_a, mu_b, E[a^2], E[b^2], E[ab] under the window,
 *     var_a = E[a^2] - mu_a^2, var_b likewise, cov = E[ab] - mu_a mu_b, value = (2 mu_a mu_b + C1)(2 cov + C2) / ((mu_a^2 + mu_b^2 + C1)
 *     (var_a + var_b + C2)), unclamped.  The separable sums (11 horizontal taps, then 11 vertical), the five maps and the value are fp64.
 *     A tile is MAS_IMG_SSIM_TILE x MAS_IMG_SSIM_TILE window positions; an extent below the window still has one tile per row / column
 *     (it carries the squared error).  Nothing outside the pictures is read.
 *   mas_img_agreement_blocks: the number of tiles = the fp64 sums `partials` must hold (negative: an error code).
 *   mas_img_agreement_reduce: ssim[n] = (the tiles of image n added in a fixed order) / (C (H - 10)(W - 10)), device fp64 [N]; NaN when
 *     H or W is below the window.  Tile sums and their order do not depend on the grid: the same pictures give the same bits.
 *   mas_code_usage: indices = n device integers of index_bytes 8 (int64) or 4 (int32) -> counts, device int64 [K + 1], ADDED to what it
 *     holds: counts[k] for 0 <= k < K, counts[K] = the indices outside [0, K).  The range check comes before any indexing.  Work-group
 *     histograms in LDS while K + 1 <= MAS_CODE_USAGE_LDS_BINS, global 64-bit integer atomics beyond.  n <= 2^32 - 1.
 *   All: no host synchronisation (they capture into a graph), grids from the shape and the CU count, 64-bit offsets, no float atomics.
 *     Null arguments, an empty shape: MAS_EINVAL.  C > MAS_IMG_MAX_CHANNELS, H W > 2^30: MAS_EUNSUPPORTED.  A workspace of another
 *     size than mas_img_agreement_blocks says: MAS_EWORKSPACE.  sse, partials, ssim, counts 8-byte aligned.                            */
enum { MAS_IMG_SSIM_TILE = 16, MAS_IMG_SSIM_WINDOW = 11, MAS_IMG_MAX_CHANNELS = 4, MAS_CODE_USAGE_LDS_BINS = 12288 };
int mas_img_bytes(const void* x, int x_dtype, int x_layout, int N, int C, int H, int W, double lo, double hi, unsigned char* out,
                  void* stream);
int mas_img_agreement_blocks(int N, int C, int H, int W);
int mas_img_agreement(const unsigned char* a, const unsigned char* b, int N, int C, int H, int W, const double* window, long long* sse,
                      double* partials, int n_partials, void* stream);
int mas_img_agreement_reduce(const double* partials, int n_partials, int N, int C, int H, int W, double* ssim, void* stream);
int mas_code_usage(const void* indices, int index_bytes, long long n, int K, long long* counts, void* stream);

/* mas_token_readout, mas_token_readout_accumulate (additions under ABI 10): the stage-2 validation read-out -- per token the negative
 *   log-likelihood, the entropy of the predictive distribution, the predicted token and the rank of the true one, from ONE read of the
 *   logits in their own dtype, and their accumulation per position of the token grid.
 *   mas_token_readout: logits, dtype, rows, V, inner, outer_stride, ld, target, ignore_index exactly as for mas_token_ce_fwd (fp32 or bf16,
 *     read in place, element alignment only, any V >= 1, 64-bit offsets).  Per row r, with m = max_j x_j, d_j = x_j - m, l = sum_j exp(d_j):
 *       nll[r]     fp32  = (m - x_t) + log l                           (m and log l kept apart, as in mas_token_ce_fwd)
 *       entropy[r] fp32  = log l - (sum_j exp(d_j) d_j) / l            (an entry of -inf adds 0 to both sums; 0 * inf is never formed)
 *       argmax[r]  int32 = the FIRST index of the maximum              (torch.argmax's rule)
 *       rank[r]    int32 = #{j : x_j > x_t} + #{j < t : x_j == x_t}    (the stored values compared as fp32, exact: the position of t in a
 *                                                                       stable descending sort; a hit at top-k is rank < k)
 *     target == ignore_index: the row is not read; nll = entropy = 0, argmax = rank = -1.  INVALID rows -- any other target outside
 *     [0, V) (not read either), a row that holds a NaN or +inf, a row of -inf alone: nll = entropy = NaN, argmax = -1, rank = V; the call
 *     returns normally.  x_t = -inf in an otherwise valid row is valid: nll = +inf.  No load is indexed by a target value.  Rows that start
 *     on a 16-byte boundary and hold at most 4 16-byte units per lane of the 256 (V <= 8192 bf16, 4096 fp32, tail V % unit included) are
 *     read from memory once; longer rows and unaligned rows are walked a second time for the rank.  No atomics: results repeat bit for bit.
 *   mas_token_readout_accumulate: the four per-row arrays of mas_token_readout, target, rows, ignore_index, L = the number of positions
 *     (row r belongs to position r % L; rows % L != 0: MAS_EINVAL), ks = HOST array of nk <= MAS_TOKEN_MAX_KS thresholds, each >= 1.
 *     A row COUNTS when its target is not ignore_index and it is not invalid (argmax >= 0).  ADDED to what the device accumulators hold:
 *       nll_sum, entropy_sum fp64 [L]: per position a local sum that starts at 0 and takes (double)nll[r] of the counted rows r = p, p + L,
 *         ... in increasing r, added ONCE to the held value (fixed order, no float atomics);
 *       count int64 [L]: the counted rows;  hits int64 [L][nk]: those with rank < ks[i];
 *       rank_hist int64 [MAS_TOKEN_RANK_BINS]: bin 0 = rank 0, bin b >= 1 = rank in [2^(b-1), 2^b), counted rows;
 *       invalid int64 [1]: the invalid rows.  (The last two: 64-bit integer atomics, exact in any order.)
 *   Both: no host synchronisation (they capture into a graph); every argument check precedes the launch.  Null arguments, an empty shape,
 *     a negative stride, nk outside 0 .. MAS_TOKEN_MAX_KS, a threshold below 1: MAS_EINVAL.  Another dtype: MAS_EUNSUPPORTED.          */
enum { MAS_TOKEN_MAX_KS = 8, MAS_TOKEN_RANK_BINS = 33 };
int mas_token_readout(const void* logits, int dtype, long long rows, int V, long long inner, long long outer_stride, long long ld,
                      const int64_t* target, long long ignore_index, float* nll, float* entropy, int32_t* argmax, int32_t* rank,
                      void* stream);
int mas_token_readout_accumulate(const float* nll, const float* entropy, const int32_t* argmax, const int32_t* rank, const int64_t* target,
                                 long long rows, long long ignore_index, long long L, const int* ks, int nk, double* nll_sum,
                                 double* entropy_sum, long long* count, long long* hits, long long* rank_hist, long long* invalid,
                                 void* stream);

/* mas_layernorm_pair_* (ABI v9): the sandwich LayerNorm + residual of one sub-block and the pre-LayerNorm of the next as ONE pass,
 *   xnew = residual + LN1(h),  y2 = LN2(xnew)      (reference models/transformer.py:201-203 + :205, and :207-209 + :197 of the next layer
 *   or the final LayerNorm :264) -- the row stays in registers between the two: 12 B per element instead of 16, bit for bit the values
 *   of the two separate launches.  h / dh in h_dtype, residual / xnew / dres / dskip in x_dtype, y2 / dy2 in y_dtype:
 *   (bf16, fp32, bf16) -- the autocast transformer with its fp32 residual stream -- or all fp32.  D % 4 == 0, D <= 1024.
 *   The backward is mas_layernorm_bwd_add on (xnew, dy2, dskip) followed by mas_layernorm_bwd_colsum on (h, its result): a fused form was
 *   built and lost (two waves per SIMD at 190 VGPRs: 80 us against 34 + 25).                                                         */
int mas_layernorm_pair_fwd(const void* h, const float* gamma1, const float* beta1, const void* residual, const float* gamma2,
                           const float* beta2, void* xnew, void* y2, float* mean_rstd1, float* mean_rstd2, int h_dtype, int x_dtype,
                           int y_dtype, int rows, int D, float eps1, float eps2, void* stream);

/* mas_colsum: out[c] = sum over rows of x[r][c] (fp32 accumulation, fixed summation order: bitwise run-to-run deterministic).
 *   The bias gradient of the transformer's Linear layers (torch.nn.Linear in reference models/transformer.py:31,34,125,126:
 *   grad_bias = grad_output.sum(0)) over [B*S, N] activations.  x bf16 or fp32, row stride = cols, cols % 8 == 0 (bf16) / % 4 (fp32).
 *   workspace: mas_colsum_workspace(rows, cols) bytes, caller-owned.                                                          */
size_t mas_colsum_workspace(int rows, int cols);
int mas_colsum(const void* x, int dtype, int rows, int cols, float* out, void* workspace, size_t workspace_bytes, void* stream);

/* -------------------------------------------------------------------------------------------
 * BatchNorm over [M][C] fp32 NHWC activations (ABI v8): the nn.SyncBatchNorm(embed_dim) behind quant_conv, reference models/vqvae.py:15-16
 * (torch.nn.SyncBatchNorm: batch statistics exchanged across the process group in training, running statistics in evaluation).
 * The library computes per-rank sums in a fixed order and takes GLOBAL sums back; the exchange itself (torch.distributed.all_reduce of
 * the fp64 vector) is the host side's, exactly where torch's own SyncBatchNorm has it.  C % 4 == 0, C <= 1024.
 *   mas_bn_partial_sums: sums[2 C + 1] (fp64) = { per-channel S1[C], S2[C], (double) M }:
 *       dy == NULL : S1 = sum x,  S2 = sum x^2                      (forward statistics)
 *       dy != NULL : S1 = sum dy, S2 = sum dy * (x - mean) * rstd   (backward; = dbeta, dgamma of this rank); mean_rstd [C][2] required
 *   mas_bn_finalize   : from (global) sums: mean_rstd [C][2], scale_shift [C][2] (y = x * scale + shift with gamma / beta folded in;
 *       gamma / beta NULL = 1 / 0) and the running statistics updated in place with `momentum` (unbiased variance, torch's convention;
 *       running_* may be NULL); sums == NULL: evaluation mode, the pair comes from running_mean / running_var.
 *   mas_bn_apply      : y = x * scale + shift.
 *   mas_bn_bwd_apply  : dx = gamma * rstd * (dy - S1 / n - xhat * S2 / n) with the GLOBAL backward sums and n = sums[2 C].        */
size_t mas_bn_workspace(int M, int C);
int mas_bn_partial_sums(const float* x, const float* dy, const float* mean_rstd, int M, int C, double* sums, void* workspace,
                        size_t workspace_bytes, void* stream);
int mas_bn_finalize(const double* sums, const float* gamma, const float* beta, float eps, float momentum, float* running_mean,
                    float* running_var, float* mean_rstd, float* scale_shift, int C, void* stream);
int mas_bn_apply(const float* x, const float* scale_shift, float* y, int M, int C, void* stream);
int mas_bn_bwd_apply(const float* x, const float* dy, const float* mean_rstd, const float* gamma, const double* sums, float* dx, int M,
                     int C, void* stream);
/* ABI v9: the same three passes on bf16 or fp32 storage (dtype = MAS_BF16 / MAS_F32 for x, dy, y, dx alike) with the LeakyReLU(slope) that
 * follows the normalisation fused in -- the nn.BatchNorm2d + nn.LeakyReLU(0.2) pairs of the PatchGAN discriminator, reference
 * losses/discriminator.py:26-33 (per-rank batch statistics there: no exchange).  slope == 1: no activation (the v8 entry points above
 * are these with MAS_F32 and slope 1).
 *   mas_bn_apply_act        : y = lrelu(x * scale + shift).
 *   mas_bn_partial_sums_act : backward sums of g = dy * lrelu'(u), u = x * scale + shift recomputed (scale_shift required when slope != 1).
 *   mas_bn_bwd_apply_act    : dx = gamma * rstd * (g - S1 / n - xhat * S2 / n) with the same g.                                      */
int mas_bn_partial_sums_act(const void* x, const void* dy, const float* mean_rstd, const float* scale_shift, float slope, int dtype, int M, int C,
                            double* sums, void* workspace, size_t workspace_bytes, void* stream);
int mas_bn_apply_act(const void* x, const float* scale_shift, void* y, float slope, int dtype, int M, int C, void* stream);
int mas_bn_bwd_apply_act(const void* x, const void* dy, const float* mean_rstd, const float* gamma, const float* scale_shift, float slope,
                         const double* sums, void* dx, int dtype, int M, int C, void* stream);

/* -------------------------------------------------------------------------------------------
 * FaceLoss (reference losses/face_loss.py): the face-aware term of the VQ-IMG objective, a frozen caffe-style ResNet-50 in
 * evaluation mode on <= 6 face crops of 254 x 254 (face.hip).  Activations are NHWC in `dtype` (MAS_BF16 / MAS_F32); every sum
 * runs in fp32 in a fixed order (no float atomics).  The 52 1x1 / 3x3 convolutions go through mas_conv_fwd.
 *   MasFaceRow: one face row, geometry computed on the host: image b of img (src 0) or rec (src 1), crop box (top, left, h, w),
 *     Resize(256) size rh x rw, CenterCrop(254) offsets ct, cl.
 *   MasFaceImage: a [N,3,H,W] image of any strides (elements), fp32 or bf16.
 *   mas_face_crop_fwd : out[r][y][x][c] (NHWC, out_dtype) = CenterCrop(Resize(crop(src_r))) with torch's antialiased bilinear weights
 *                       (align_corners = False); pixels of the box outside the image read 0.
 *   mas_face_crop_bwd : the exact adjoint as a gather: drec (written in full, its own strides) = sum over the rows in table order of
 *                       the rows' fp32 gradients dfaces [n_rows][254][254][3].  Every row is taken as a rec row.
 *   mas_face_stem_fwd / _dgrad : the 7x7 / stride 2 / pad 3 convolution 3 -> 64 (w fp32 OIHW) on [R,254,254,3] -> [R,127,127,64],
 *                       and its data gradient (dx fp32).
 *   mas_face_bn_fold  : the evaluation-mode affine pairs of n_items BatchNorm2d layers (items: a DEVICE table) into
 *                       scale_shift[(off + c) * 2 + {0,1}], one launch.
 *   mas_face_pool_fwd / _bwd : relu(bn(y)) -> MaxPool2d(3, 2, ceil_mode) over an [R,H,W,C] map; idx (one byte per output) holds the
 *                       window index of the first maximum; the backward writes dy = relu'(u) * scale * (gather of dz) + seed.
 *   mas_face_join_fwd : out = relu(y3 * s3 + t3 + (ssr ? r * sr + tr : r)), the Bottleneck's residual join.
 *   mas_face_join_bwd : g = [out > 0] (dout + dadd) (either may be NULL), dy3 = g * s3, dres = ssr ? g * sr : g.
 *   mas_face_relu_bn_bwd : dy = [a > 0] da * s (a = relu(bn(y)) saved by the forward).
 *   mas_face_subsample2x : y[n][h][w][c] = x[n][2h][2w][c], y [N, ceil(H/2), ceil(W/2), C] (the stride of a 1x1 / stride-2 conv).
 *   mas_face_l1_fwd   : out6[i] = alpha_i * sum |p0 - p1| / chw_i over the `half` row pairs (row q against row half + q) of feature i,
 *                       out6[5] = their sum; workspace of mas_face_l1_workspace(f) floats.  Two launches (partials, fixed-order fold).
 *   mas_face_l1_bwd   : seeds[i] [nb rows of feature i] = (dl6[i] + dl6[5]) * alpha_i * sign(p(row0 + k) - p(row0 + k - half)) / chw_i
 *                       (seeds: a HOST array of five device pointers; sign(0) = 0).
 *
 * (Additions inside ABI v10.)  The same four passes with the rows read from a DEVICE table of fixed capacity, so that launch arguments,
 * grids and every shape are the same whatever the boxes are (a captured graph replays them; the host rewrites the table before each replay):
 *   The table: MAS_FACE_TABLE_INTS int32 on the device.  Slot s of MAS_FACE_SLOTS = 6 is the MasFaceRow at ints [10 s, 10 s + 10)
 *     (its ten fields in order), valid[s] (!= 0: the slot holds a row) is int 60 + s, n_pairs int 66, int 67 is zero.  Row q < half of
 *     the reference's cat([gt], [rec])[:6] sits in slot q, row half + q in slot 3 + q: pair q is (slot q, slot 3 + q) and is valid iff
 *     q < n_pairs; every rec row sits in slots 3..5.  A slot is also taken as empty when its fields could not have passed the host's
 *     checks (b outside the images, a size <= 0, a resized side below 254, a centre crop outside the resized crop, src not 0 / 1), and
 *     n_pairs outside 0..3 is clamped.
 *   mas_face_crop_fwd_dev : mas_face_crop_fwd into out [6][254][254][3]; an empty slot's row is written as zeros.
 *   mas_face_l1_fwd_dev   : mas_face_l1_fwd over six rows per feature (f->half must be 3: p0 = rows 0..2, p1 = rows 3..5; workspace of
 *                       mas_face_l1_workspace(f) floats); the elements of an invalid pair add exactly 0.0f, and the valid pairs are
 *                       summed in the order mas_face_l1_fwd uses for half = n_pairs.
 *   mas_face_l1_bwd_dev   : seeds[i] [3 rows of feature i] for slots 3..5: mas_face_l1_bwd's value where the pair is valid and the slot
 *                       holds a rec row (src 1), zeros elsewhere.  Every element is written.
 *   mas_face_crop_bwd_dev : mas_face_crop_bwd over slots 3, 4, 5 in that order (dfaces [3][254][254][3]), taking the slots that hold a
 *                       rec row; drec is written in full (zeros without one).                                                        */
#define MAS_FACE_SIZE 254
#define MAS_FACE_MAX_ROWS 8
#define MAS_FACE_SLOTS 6
#define MAS_FACE_TABLE_INTS 68
typedef struct { int32_t src, b, top, left, h, w, rh, rw, ct, cl; } MasFaceRow;
typedef struct { void* data; int32_t dtype, N, C, H, W, pad_; int64_t sn, sc, sh, sw; } MasFaceImage;
typedef struct { const float* weight; const float* bias; const float* mean; const float* var; int32_t C, off; float eps; int32_t pad_; } MasFaceBnItem;
typedef struct { const void* p[5]; int32_t chw[5]; int32_t half; int32_t dtype; float alpha[5]; } MasFaceFeats;
int mas_face_crop_fwd(const MasFaceImage* img, const MasFaceImage* rec, const MasFaceRow* rows, int n_rows, void* out, int out_dtype,
                      void* stream);
int mas_face_crop_bwd(const float* dfaces, const MasFaceRow* rows, int n_rows, const MasFaceImage* drec, void* stream);
int mas_face_stem_fwd(const void* x, const float* w, void* y, int dtype, int R, void* stream);
int mas_face_stem_dgrad(const void* dy, const float* w, float* dx, int dtype, int R, void* stream);
int mas_face_bn_fold(const MasFaceBnItem* items, int n_items, float* scale_shift, void* stream);
int mas_face_pool_fwd(const void* y, const float* scale_shift, void* z, unsigned char* idx, int dtype, int R, int H, int W, int C, void* stream);
int mas_face_pool_bwd(const void* y, const float* scale_shift, const void* dz, const unsigned char* idx, const void* seed, void* dy, int dtype,
                      int R, int H, int W, int C, void* stream);
int mas_face_join_fwd(const void* y3, const float* ss3, const void* r, const float* ssr, void* out, int dtype, int M, int C, void* stream);
int mas_face_join_bwd(const void* dout, const void* dadd, const void* out, const float* ss3, const float* ssr, void* dy3, void* dres, int dtype,
                      int M, int C, void* stream);
int mas_face_relu_bn_bwd(const void* da, const void* a, const float* scale_shift, void* dy, int dtype, int M, int C, void* stream);
int mas_face_subsample2x(const void* x, void* y, int dtype, int N, int H, int W, int C, void* stream);
int mas_face_l1_workspace(const MasFaceFeats* f);
int mas_face_l1_fwd(const MasFaceFeats* f, float* workspace, float* out6, void* stream);
int mas_face_l1_bwd(const MasFaceFeats* f, int row0, int nb, const float* dl6, void* const* seeds, void* stream);
int mas_face_crop_fwd_dev(const MasFaceImage* img, const MasFaceImage* rec, const int32_t* table_dev, void* out, int out_dtype,
                          void* stream);
int mas_face_l1_fwd_dev(const MasFaceFeats* f, const int32_t* table_dev, float* workspace, float* out6, void* stream);
int mas_face_l1_bwd_dev(const MasFaceFeats* f, const int32_t* table_dev, const float* dl6, void* const* seeds, void* stream);
int mas_face_crop_bwd_dev(const float* dfaces, const int32_t* table_dev, const MasFaceImage* drec, void* stream);

/* -------------------------------------------------------------------------------------------
 * The object-aware term of the VQ-IMG objective (Make-A-Scene section 3.2): LPIPS-VGG16 on every object crop of a batch AT ONCE
 * (object.hip).  Every used crop (both sides >= 16 px) sits at a 16-aligned origin of one of n_canvas NHWC canvases, with a zero
 * gutter of >= 16 px after it; the real crops and the rec crops share their places in two canvas images, so one canvas batch is
 * [2 * n_canvas, H, W, C]: real canvases first.  The thirteen convolutions run through mas_conv_fwd; after each one a ReLU + mask
 * pass zeroes everything outside the crops' valid rectangles of that level l (origin >> l, size h >> l, w >> l), so each crop's
 * values are those of an isolated LPIPS on it.  Activations in `dtype` (MAS_BF16 / MAS_F32), arithmetic and sums in fp32, in a fixed
 * order (no float atomics).  Tensors of the backward are the rec half only: [n_canvas, ...].
 *   MasObjCell: one crop: canvas n, origin (oy, ox), size h x w, image b, box corner (top, left) in the image.
 *   MasObjPlan: DEVICE tables -- cells in (image, box) order; img_cell0 [n_images + 1] (the cells of image b are
 *     [img_cell0[b], img_cell0[b + 1])); tiles [n_canvas][H / 16][W / 16]: the cell whose rectangle meets the 16 x 16 tile, or -1
 *     (one at most: origins are 16-aligned and gutters >= 16 px); blk0 [5][n_cells + 1]: the first head block of every cell per
 *     level (MAS_OBJ_HEAD_PIX(C) pixels per block).  H and W are multiples of 16.
 *   mas_obj_canvas_fwd : canvas [2 * n_canvas, H, W, 8] = ScalingLayer(crop(img | rec)) inside the cells ((v - shift) / scale; a
 *                        pixel of the box outside the image is v = 0), channels 3..7 and everything outside the cells 0.
 *   mas_obj_canvas_bwd : the adjoint as a gather: drec (written in full, its own strides) = sum over the image's cells in table
 *                        order of dcanvas [n_canvas, H, W, 8] (rec side, channels 0..2) / scale.
 *   mas_obj_relu_fwd   : in place on y [N, H >> l, W >> l, C] (canvas index n % n_canvas): y = inside ? max(y, 0) : 0.
 *   mas_obj_relu_bwd   : dy = a > 0 ? da : 0 over n elements (n % 8 == 0; dy may alias da).
 *   mas_obj_pool_fwd   : y [N, H >> (l+1), W >> (l+1), C] = the 2 x 2 / stride-2 max of x [N, H >> l, W >> l, C] inside the level-(l+1)
 *                        rectangles, 0 outside.
 *   mas_obj_pool_bwd   : dy [N, H >> l, W >> l, C] = a > 0 ? seed + (dz at the pooled pixel if that pixel is inside and this one
 *                        is its window's first maximum, else 0) : 0; seed and dz may be NULL.
 *   mas_obj_head_fwd   : feat [2 * n_canvas, H >> l, W >> l, C] -> partial[blk0[l][k] .. blk0[l][k + 1]) = fixed-order partial sums
 *                        over cell k's pixels of sum_c w_c (f_c / (|f| + 1e-10) - g_c / (|g| + 1e-10))^2 (f real, g rec).
 *   mas_obj_finalize   : partial (the five levels one after the other) -> out[1 + k] = sum_l (cell k's sum at l) / (h_l w_l), the
 *                        crop's LPIPS, and out[0] = sum_b (sum of its crops' values) / (n_b + 1).  One block.
 *   mas_obj_head_bwd   : seed [n_canvas, H >> l, W >> l, C] = d out / d g at level l for dout [1 + n_cells] (device), 0 outside the
 *                        cells.                                                                                                   */
#define MAS_OBJ_ALIGN 16
#define MAS_OBJ_MIN_SIDE 16
#define MAS_OBJ_CANVAS_C 8
#define MAS_OBJ_HEAD_PIX(C) (8192 / (C))
typedef struct { int32_t n, oy, ox, h, w, b, top, left; } MasObjCell;
typedef struct {
    const MasObjCell* cells; const int32_t* img_cell0; const int32_t* tiles; const int32_t* blk0;
    int32_t n_cells, n_images, n_canvas, H, W, pad_;
} MasObjPlan;
int mas_obj_canvas_fwd(const MasFaceImage* img, const MasFaceImage* rec, const MasObjPlan* p, const float* shift, const float* scale,
                       void* canvas, int dtype, void* stream);
int mas_obj_canvas_bwd(const void* dcanvas, int dtype, const MasObjPlan* p, const float* scale, const MasFaceImage* drec, void* stream);
int mas_obj_relu_fwd(void* y, const MasObjPlan* p, int level, int N, int C, int dtype, void* stream);
int mas_obj_relu_bwd(const void* da, const void* a, void* dy, long long n, int dtype, void* stream);
int mas_obj_pool_fwd(const void* x, void* y, const MasObjPlan* p, int level, int N, int C, int dtype, void* stream);
int mas_obj_pool_bwd(const void* a, const void* seed, const void* dz, void* dy, const MasObjPlan* p, int level, int N, int C, int dtype,
                     void* stream);
int mas_obj_head_fwd(const void* feat, const float* w, const MasObjPlan* p, int level, int C, int dtype, int n_blocks, float* partial,
                     void* stream);
int mas_obj_finalize(const float* partial, const MasObjPlan* p, float* out, void* stream);
int mas_obj_head_bwd(const void* feat, const float* w, const MasObjPlan* p, int level, int C, int dtype, const float* dout, void* seed,
                     void* stream);

/* (Additions inside ABI v10.)  The same passes on an atlas of FIXED capacity, so that launch arguments, grids and every shape depend on the
 * atlas geometry alone (a captured graph replays them; the host rewrites the table before each replay).  The geometry comes by value
 * with every call -- max_cells, n_images, n_canvas, H, W (H and W multiples of 16) -- and everything about the boxes is read from
 * table_dev, mas_obj_atlas_ints(...) int32 on the device with fixed strides:
 *     header [MAS_OBJ_ATLAS_HEADER]: {n_cells, max_cells, n_images, n_canvas, H, W, 0, 0}
 *     cells [max_cells] (MasObjCell, the first n_cells used) | img_cell0 [n_images + 1] | blk0 [5][max_cells + 1] (row l valid up to
 *     blk0[l][n_cells]) | tiles [n_canvas][H / 16][W / 16]
 *   n_cells and the blk0 stride (max_cells + 1) are the table's; a header with n_cells outside [0, max_cells] makes every work-group of
 *   every kernel here return without reading or writing anything else.  The kernel bodies are mas_obj_*'s own: for the same cells on the
 *   same canvas the values are theirs bit for bit.  (The ReLU backward takes no table: mas_obj_relu_bwd.)
 *   mas_obj_atlas_ints    : the table's length in int32 (MAS_EINVAL < 0 for a geometry the library refuses).
 *   mas_obj_head_grid_dev : G_l = ceil(n_canvas (H >> l)(W >> l) / MAS_OBJ_HEAD_PIX(C_l)) + max_cells, C = 64, 128, 256, 512, 512: the
 *                           head's grid at level l.  It bounds blk0[l][n_cells] for every table: the cells' level-l rectangles are
 *                           disjoint and inside the canvases, and each cell rounds up to whole blocks once.
 *   mas_obj_canvas_fwd_dev, mas_obj_canvas_bwd_dev, mas_obj_relu_fwd_dev, mas_obj_pool_fwd_dev, mas_obj_pool_bwd_dev: as named.
 *   mas_obj_head_fwd_dev  : level l on G_l blocks; block j < blk0[l][n_cells] writes partial[off_l + j], off_l = G_0 + .. + G_(l-1)
 *                           (partial: sum of the five G_l floats); the other blocks return.  C is the level's.
 *   mas_obj_finalize_dev  : out [1 + max_cells] written in full: the loss, the n_cells crop values, zeros.  n_cells == 0: all zeros.
 *   mas_obj_head_bwd_dev  : dout [1 + max_cells]; seed written in full (all zeros for an empty table).                              */
#define MAS_OBJ_ATLAS_HEADER 8
int mas_obj_atlas_ints(int max_cells, int n_images, int n_canvas, int H, int W);
int mas_obj_head_grid_dev(int level, int max_cells, int n_canvas, int H, int W);
int mas_obj_canvas_fwd_dev(const MasFaceImage* img, const MasFaceImage* rec, const int32_t* table_dev, int max_cells, int n_images,
                           int n_canvas, int H, int W, const float* shift, const float* scale, void* canvas, int dtype, void* stream);
int mas_obj_canvas_bwd_dev(const void* dcanvas, int dtype, const int32_t* table_dev, int max_cells, int n_images, int n_canvas, int H, int W,
                           const float* scale, const MasFaceImage* drec, void* stream);
int mas_obj_relu_fwd_dev(void* y, const int32_t* table_dev, int max_cells, int n_images, int n_canvas, int H, int W, int level, int N, int C,
                         int dtype, void* stream);
int mas_obj_pool_fwd_dev(const void* x, void* y, const int32_t* table_dev, int max_cells, int n_images, int n_canvas, int H, int W, int level,
                         int N, int C, int dtype, void* stream);
int mas_obj_pool_bwd_dev(const void* a, const void* seed, const void* dz, void* dy, const int32_t* table_dev, int max_cells, int n_images,
                         int n_canvas, int H, int W, int level, int N, int C, int dtype, void* stream);
int mas_obj_head_fwd_dev(const void* feat, const float* w, const int32_t* table_dev, int max_cells, int n_images, int n_canvas, int H, int W,
                         int level, int dtype, float* partial, void* stream);
int mas_obj_finalize_dev(const float* partial, const int32_t* table_dev, int max_cells, int n_images, int n_canvas, int H, int W, float* out,
                         void* stream);
int mas_obj_head_bwd_dev(const void* feat, const float* w, const int32_t* table_dev, int max_cells, int n_images, int n_canvas, int H, int W,
                         int level, int dtype, const float* dout, void* seed, void* stream);

/* -------------------------------------------------------------------------------------------
 * Whole-image LPIPS-VGG16 (lpips.hip; mas_hip/lpips.py; losses.lpips.hip_path).  Additions inside ABI 10.  Everything of
 * losses/lpips.py:LPIPS.forward that is not one of the thirteen convolutions (those go through mas_conv_fwd), on plain NHWC maps:
 * no atlas, no tables.  One batch is [2 B, H, W, C]: the B real images first, then the B reconstructions; tensors of the backward
 * are the rec half only, [B, ...].  Activations in `dtype` (MAS_BF16 / MAS_F32), arithmetic and sums in fp32, in a fixed order (no
 * float atomics).  Nothing reads the host; every launch goes to `stream`.  Before anything is launched: null pointers, a dtype other
 * than MAS_F32 / MAS_BF16, a size < 1, C % 8 != 0 (heads: C outside {64, 128, 256, 512}) are MAS_EINVAL; more than 2^30 pixels
 * per image is MAS_EUNSUPPORTED.
 *   mas_lpips_pack_fwd : canvas [2 B, H, W, 8] = (x - shift) / scale in channels 0..2 and 0 in channels 3..7, x = real for the
 *                        first B images and fake for the rest (each fp32 or bf16, any element strides; equal N, H, W).
 *   mas_lpips_pack_bwd : the adjoint: dfake (its own dtype and strides, written in full) = dcanvas [B, H, W, 8] (rec half,
 *                        channels 0..2) / scale.
 *   mas_lpips_relu_fwd : y = y < 0 ? 0 : y in place over n elements (n % 8 == 0): a NaN stays a NaN, as in F.relu.  (Its backward is
 *                        mas_obj_relu_bwd.)
 *   mas_lpips_pool_fwd : y [N, H / 2, W / 2, C] = the 2 x 2 / stride-2 max of x [N, H, W, C] (floor: an odd last row or column is
 *                        in no window; H, W >= 2); a NaN in a window is its maximum, as in F.max_pool2d.
 *   mas_lpips_pool_bwd : dy [N, H, W, C] = a > 0 ? seed + (dz [N, H / 2, W / 2, C] at the pixel's window if this pixel is the
 *                        window's first maximum in row-major order, else 0) : 0; a is the ReLU output that was pooled; a pixel
 *                        in no window gets the seed only; seed and dz may each be NULL.
 *   mas_lpips_head_blocks : partial sums per image of one level: ceil(H W / (8192 / C)); negative on a bad argument.
 *   mas_lpips_head_fwd : feat [2 B, H, W, C] -> partial[b * nblk + j], j < nblk = mas_lpips_head_blocks(H, W, C): fixed-order sums
 *                        over 8192 / C pixels each of sum_c w_c (r_c / (|r| + 1e-10) - f_c / (|f| + 1e-10))^2 (r real, f rec); the
 *                        difference is formed before it is squared, the pixel's channels stay in registers.
 *   mas_lpips_finalize : out[b] = sum_l (sum_j partial_l[b][j]) / hw[l] over n_levels <= 8 levels, whose partials lie one level
 *                        after the other ([B][blocks[l]] each).  hw and blocks are HOST arrays of n_levels int32.  One work-group
 *                        per image; a level's sum is 256 strided chains folded by a tree (blocks[l] <= 2^18: no chain of more
 *                        than 1024 additions).
 *   mas_lpips_head_bwd : seed [B, H, W, C] = d (sum_b dout[b] out[b]) / d f at this level: coefficient dout[b] / (H W) (dout: B
 *                        device floats); mas_obj_head_bwd's formula, its rule at |f| = 0 included (the 1 / |f| term is 0).    */
int mas_lpips_pack_fwd(const MasFaceImage* real, const MasFaceImage* fake, const float* shift, const float* scale, void* canvas, int dtype,
                       void* stream);
int mas_lpips_pack_bwd(const void* dcanvas, int dtype, const float* scale, const MasFaceImage* dfake, void* stream);
int mas_lpips_relu_fwd(void* y, long long n, int dtype, void* stream);
int mas_lpips_pool_fwd(const void* x, void* y, int N, int H, int W, int C, int dtype, void* stream);
int mas_lpips_pool_bwd(const void* a, const void* seed, const void* dz, void* dy, int N, int H, int W, int C, int dtype, void* stream);
int mas_lpips_head_blocks(int H, int W, int C);
int mas_lpips_head_fwd(const void* feat, const float* w, int B, int H, int W, int C, int dtype, float* partial, void* stream);
int mas_lpips_finalize(const float* partial, int B, int n_levels, const int32_t* hw, const int32_t* blocks, float* out, void* stream);
int mas_lpips_head_bwd(const void* feat, const float* w, int B, int H, int W, int C, int dtype, const float* dout, void* seed, void* stream);

/* ---- Codebook reservoir (make-a-scene_amd/csrc/reservoir.hip; Codebook.enable_device_reservoir).  The reference's reservoir of latent
 * rows (models/modules.py:477-481: 10 random positions per image appended, then a random subset of reservoir_size rows kept), stated
 * on sets and kept wholly on the device, so that a training step holding it can be captured into a graph.  An addition inside ABI 10.
 *   z     fp32 [B, HW, D] (the NHWC latent), read only;      buf   fp32 [R, D], rows [0, c) held;
 *   state int32 {c, calls}: rows held and the number of calls so far (the Philox counter); zero both to empty the reservoir;
 *   plan  int32 [2 * 10 * B] workspace: {destination slot or -1, source row of z} per candidate, written by the first launch and read
 *         by the second;   seed: fixed by the caller for the reservoir's life.   The host reads nothing: c after k calls of batch B is
 *         min(R, 10 B k).
 * One call, with n = 10 B, m = c + n, calls = state[1]:
 *   positions   pos_j = P(j), j = 0 .. 9, P a keyed bijection of [0, HW): 10 distinct positions, the same for every image of the batch
 *               (the reference's one randperm(HW)[:10]).  Candidate i = 10 b + j is row b * HW + pos_j of z, copied bit for bit.
 *   m <= R      candidate i goes to slot c + i.
 *   m >  R      the rows Q(t), t = 0 .. m - R - 1, of the m rows {old slots 0 .. c-1, candidate i as c + i} are dropped, Q a keyed
 *               bijection of [0, m): a pseudo-random (m - R)-subset, distinct by construction.  The surviving candidates, in the order
 *               of i, take the free slots c, c + 1, .. R - 1 first and then the slots of the dropped old rows in the order of t.
 *   then        state = {min(R, m), calls + 1}, stored by the one planning work-group after a barrier behind its last read of them.
 * Keyed bijection of [0, N): h = the smallest value >= 1 with 4^h >= N; x = (l << h) | r; four balanced Feistel rounds
 *   (l, r) <- (r, l ^ (F(r, round) & (2^h - 1))), F = word x of Philox4x32-10 at counter (r, round, stream, calls) under the key
 *   (lo32(seed), hi32(seed)), stream 0 for P and 1 for Q; the result is walked round its cycle (applied again) until it is below N.
 *   Every lane computes its own index; no lane waits for another's draw.
 * Two launches on `stream`: one work-group that plans (block scans in LDS rank the survivors and the dropped slots), then 64 lanes per
 * candidate row copying with 16-byte loads and stores.  A state outside 0 <= c <= R holds nothing new and is left as it is.
 * Checked on the host before anything is launched: HW >= 10, 10 B <= R, D % 4 == 0, pointers given and z / buf 16-byte aligned
 * (MAS_EINVAL); 10 B <= MAS_RESERVOIR_MAX_CANDIDATES, R + 10 B <= 2^30, B HW <= 2^30 (MAS_EUNSUPPORTED).                          */
#define MAS_RESERVOIR_PER_IMAGE 10
#define MAS_RESERVOIR_MAX_CANDIDATES 2048
int mas_reservoir_collect(const float* z, float* buf, int32_t* state, int32_t* plan, long long seed, int R, int B, int HW, int D,
                          void* stream);

/* ---- K-means re-initialisation (make-a-scene_amd/csrc/kmeans.hip; ops.kmeans_fit, models.kmeans.kmeans_fit(on_device=True),
 * Codebook.enable_device_reservoir(device_kmeans=True)).  Lloyd's iterations of the codebook re-initialisation (reference
 * models/modules.py:487-499 through fast_pytorch_kmeans; oracle/kmeans_oracle.py states the rule) as a fixed sequence of launches: the
 * host enqueues max_iter iterations and reads nothing, the stop test runs on the device.  Additions inside ABI 10.
 *   points    fp32 [M, D], read only;      centroids fp32 [K, D]: the initial centroids on entry, the final ones on return (in place);
 *   assign    int64 [M]: the assignment of the last executed iteration, i.e. against the centroids BEFORE the last update;
 *   info      int32 {iterations run, converged};      shift  fp64 [1]: the last sum (new - old)^2;
 *   workspace mas_kmeans_workspace(M, K) bytes.
 * One iteration:
 *   assignment  mas_vq_argmin_fwd's own distance kernels (one copy of the device code): d = fl(fl(|x|^2 + |c|^2) - 2 dot), dot an
 *               exact-fp32 FMA chain, the lowest index on ties.  |x|^2 is computed once per fit, |c|^2 once per iteration.
 *   update      new centroid = sum / count of its points, an empty cluster becomes the ZERO vector.  A work-group owns 8 centroids; its
 *               four waves scan a quarter of the assignments each in position order and add into their own fp32 accumulators, which are
 *               folded in wave order: no atomics, the order is fixed, a fit repeats bit for bit.  Written in place.
 *   advance     shift = sum (new - old)^2 over all K D elements (differences in fp32, squares and the sum in fp64, fixed order);
 *               one work-group stores info = {iterations + 1, shift <= (double)tol} and shift.
 *   skip        once `converged` is set every kernel of the remaining iterations returns before its first load: nothing more is written.
 * mas_kmeans_init: centroid k = a bitwise copy of point row P(k), k = 0 .. K-1, P the keyed bijection of [0, M) of "Codebook
 *   reservoir" above with stream 2, calls = draw and the key (lo32(seed), hi32(seed)): K distinct rows by construction.  init_idx
 *   (int32 [K], may be null) receives P(k).
 * Checked on the host before anything is launched: D in {32, 64, 128, 256} and M <= 2^30 (MAS_EUNSUPPORTED); 1 <= K <= M,
 * max_iter >= 1, pointers given, points / centroids / workspace 16-byte aligned (MAS_EINVAL); the workspace size (MAS_EWORKSPACE).      */
size_t mas_kmeans_workspace(int M, int K);
int mas_kmeans_init(const float* points, int M, int K, int D, long long seed, int draw, float* centroids, int32_t* init_idx, void* stream);
int mas_kmeans_fit(const float* points, float* centroids, int M, int K, int D, int max_iter, float tol, int64_t* assign, int32_t* info,
                   double* shift, void* workspace, size_t ws_bytes, void* stream);

/* ---- Tail of the VQ-IMG objective (make-a-scene_amd/csrc/gan_loss.hip; losses.loss_img.hip_tail).  What follows the
 * decoder, LPIPS and the discriminator in reference losses/loss_img.py:56-141, with nothing read on the host: the calls capture into a
 * graph.  Additions inside ABI 10.  No atomics; every sum has one order, fixed by the shape and the CU count: results repeat bit for bit.
 * Sums: a lane adds MAS_GAN_RUN = 8 fp32 terms as a fixed pairwise tree (each term is rounded once when it is formed and passes through
 * three additions), everything beyond -- the lane's further runs, lanes, work-groups, the finalize -- is fp64, and the result is rounded
 * once to fp32: for non-negative terms the error is below (3 + 1 + 1) 2^-24 relative, inside MAS_GAN_RUN 2^-24.
 *   img, rec: [N, C, H, W], each fp32 or bf16 (MAS_F32 / MAS_BF16), each DENSE MAS_SEG_NCHW or MAS_SEG_NHWC on its own, read in place,
 *     element alignment only, fewer than 2^31 elements (MAS_EUNSUPPORTED beyond).
 *   mas_gan_l1_blocks: the work-groups of mas_gan_l1_fwd = the fp64 partial sums its workspace must hold (negative: an error code).
 *   mas_gan_l1_fwd: partials[b] = work-group b's sum of |rec - img|.  A NaN in either input makes the sum NaN.
 *   mas_gan_l1_finalize: ONE work-group -> out[0] = the sum, out[1] = sum / numel + perceptual_weight mean(perceptual[0 .. B-1])
 *     (perceptual: B fp32 on the device, or NULL: the second term is 0) = the reference's nll_loss.
 *   mas_gan_l1_bwd: coef = grad[0] / (float)numel, ONE fp32 division; drec = +coef where rec > img, -coef where rec < img, exactly 0
 *     otherwise (equal -- torch.abs's subgradient -- or unordered), cast once to rec's dtype, in rec's layout.  dperceptual (B fp32, may
 *     be NULL) = grad[0] * (perceptual_weight / (float)B).  grad: one fp32 on the device, the gradient with respect to out[1].
 *   mas_gan_logits_fwd: ONE work-group over the PatchGAN logits (fp32, contiguous; real may be NULL) -> out[0] = -mean(fake),
 *     out[1] = mean(relu(1 - real)), out[2] = mean(relu(1 + fake)), out[3] = gate 0.5 (out[1] + out[2]) before rounding, with
 *     gate = global_step[0] >= disc_start ? disc_factor : 0 read on the device (global_step: one int64, may be NULL: gate = 0), and
 *     out[4] = gate: five fp32.
 *   mas_gan_logits_bwd: grad_gen = the gradient of out[0], grad_d = that of out[3] (each one fp32 on the device, or NULL), gate = the
 *     forward's out + 4 (the counter may have moved since), all fp32:  c = (grad_d[0] * (0.5f * gate[0])) / (float)n;  dfake = (fake > -1 ? c : 0) - grad_gen[0] / (float)n_fake;  dreal = real < 1 ? -c : 0
 *     (n = the tensor's own count): zero at the hinge knees, as ATen's relu backward.
 *   mas_gan_combine_fwd: ONE work-group.  nll, g_loss, face, object: one fp32 each (face / object may be NULL); codebook: n_codebook
 *     fp32, their mean is taken here; nll_grads, g_grads: n_grads fp32 each, the two gradients of the decoder's last weight.  In fp64:
 *     d_weight = clamp(|nll_grads| / (|g_grads| + 1e-4), 0, 1e4) disc_weight, rounded to fp32; gate as above; c_g = d_weight * gate (fp32);
 *     loss = nll + c_g g_loss + codebook_weight mean(codebook) + face + object, rounded once.  out = {loss, d_weight, c_g, gate}.
 *     advance != 0: global_step[0] += 1 after it has been read.
 *   mas_gan_combine_bwd: one lane.  grads[0] = grad[0] (nll, face, object), grads[1] = grad[0] * out[2] (g_loss), grads[2] = grad[0] *
 *     (codebook_weight / (float)n_codebook) (every element of codebook); d_weight is a constant of the loss, as in the reference.
 * Null or misaligned pointers, empty shapes, unknown codes: MAS_EINVAL.                                                              */
enum { MAS_GAN_RUN = 8 };
int mas_gan_l1_blocks(int N, int C, int H, int W);
int mas_gan_l1_fwd(const void* img, int img_dtype, int img_layout, const void* rec, int rec_dtype, int rec_layout, int N, int C, int H,
                   int W, double* partials, int n_partials, void* stream);
int mas_gan_l1_finalize(const double* partials, int n_partials, long long numel, const float* perceptual, int B, float perceptual_weight,
                        float* out, void* stream);
int mas_gan_l1_bwd(const void* img, int img_dtype, int img_layout, const void* rec, int rec_dtype, int rec_layout, int N, int C, int H,
                   int W, const float* grad, void* drec, float* dperceptual, int B, float perceptual_weight, void* stream);
int mas_gan_logits_fwd(const float* fake, long long n_fake, const float* real, long long n_real, const long long* global_step,
                       long long disc_start, float disc_factor, float* out, void* stream);
int mas_gan_logits_bwd(const float* fake, long long n_fake, const float* real, long long n_real, const float* grad_gen, const float* grad_d,
                       const float* gate, float* dfake, float* dreal, void* stream);
int mas_gan_combine_fwd(const float* nll, const float* g_loss, const float* codebook, long long n_codebook, const float* face,
                        const float* object, const float* nll_grads, const float* g_grads, long long n_grads, long long* global_step,
                        long long disc_start, float disc_factor, float disc_weight, float codebook_weight, int advance, float* out,
                        void* stream);
int mas_gan_combine_bwd(const float* grad, const float* out, float codebook_weight, long long n_codebook, float* grads, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MAS_HIP_H */
