"""numpy restatement of the tail of the VQ-IMG objective (reference losses/loss_img.py:56-141; csrc/gan_loss.hip, include/mas_hip.h "Tail
of the VQ-IMG objective"): forward values in fp64, backward rules in the fp32 operations the header fixes, so that the kernels' gradients
are compared bit for bit.  Arrays are logical NCHW; nothing here knows a memory layout.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

F32 = np.float32
RUN = 8                 # MAS_GAN_RUN: fp32 terms per lane before the sum goes on in fp64
U = 2.0 ** -24          # unit roundoff of fp32


def sum_bound(abs_sum):
    """|kernel sum - fp64 sum| for terms whose absolute values add up to ``abs_sum``: a term is rounded once when it is formed, passes through
    three fp32 additions of the lane's pairwise tree over RUN = 8 terms, and the fp64 total (whose own error, ~2^-53 per addition, is far
    below) is rounded once to fp32: (1 + 2^-24)^5 - 1 < 5.01 * 2^-24 relative -- inside the RUN * 2^-24 that is asserted."""
    return RUN * U * float(abs_sum)


def bf16_round(x):
    """fp32 values rounded to bfloat16 (nearest, ties to even; NaN stays NaN), returned as fp32"""
    x = np.ascontiguousarray(x, dtype=F32)
    b = x.view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000).astype(np.uint32).view(F32)
    return np.where(np.isnan(x), x, r).astype(F32)


# ---- 1a: the L1 term ---------------------------------------------------------------------------------------------------------------------
def l1_sum(images, rec):
    return float(np.abs(rec.astype(np.float64) - images.astype(np.float64)).sum())


def nll(images, rec, perceptual=None, perceptual_weight=1.0):
    """mean(|images - rec| + perceptual_weight * perceptual[b]) = sum / numel + perceptual_weight * mean(perceptual)"""
    p = 0.0 if perceptual is None else float(perceptual_weight) * float(np.asarray(perceptual, dtype=np.float64).mean())
    return l1_sum(images, rec) / rec.size + p


def l1_backward(images, rec, g, bf16=False):
    """coef = g / float32(N), ONE fp32 division; +coef where rec > images, -coef where rec < images, 0 otherwise (equal, or a NaN); cast
    once to the dtype of ``rec`` (``bf16``: the value bfloat16 holds, as fp32)"""
    coef = F32(g) / F32(rec.size)
    r, x = rec.astype(F32), images.astype(F32)
    d = np.where(r > x, coef, np.where(r < x, -coef, F32(0))).astype(F32)
    return bf16_round(d) if bf16 else d


def perceptual_backward(g, n, perceptual_weight=1.0):
    return F32(g) * (F32(perceptual_weight) / F32(n))


# ---- 1b: the PatchGAN logit terms --------------------------------------------------------------------------------------------------------
def gate(global_step, disc_start, disc_factor=1.0):
    return float(disc_factor) if int(global_step) >= int(disc_start) else 0.0


def logit_terms(fake, real=None):
    """-> (-mean(fake), mean(relu(1 - real)) or 0.0, mean(relu(1 + fake))) in fp64"""
    f = fake.astype(np.float64)
    m_real = 0.0 if real is None else float(np.maximum(1.0 - real.astype(np.float64), 0.0).mean())
    return -float(f.mean()), m_real, float(np.maximum(1.0 + f, 0.0).mean())


def hinge_d_loss(real, fake, global_step, disc_start, disc_factor=1.0):
    _, m_real, m_fake = logit_terms(fake, real)
    return gate(global_step, disc_start, disc_factor) * 0.5 * (m_real + m_fake)


def generator_term_backward(fake, g):
    """d(-mean(fake)): 0 - g / float32(n) at every element"""
    return np.full(fake.shape, F32(0) - F32(g) / F32(fake.size), dtype=F32)


def hinge_backward(real, fake, g, global_step, disc_start, disc_factor=1.0):
    """c = (g * (0.5 * gate)) / float32(n); d fake = c where fake > -1, d real = -c where real < 1, 0 elsewhere (the knees included)"""
    hg = F32(g) * (F32(0.5) * F32(gate(global_step, disc_start, disc_factor)))
    cf, cr = hg / F32(fake.size), hg / F32(real.size)
    return (np.where(real.astype(F32) < 1, -cr, F32(0)).astype(F32), np.where(fake.astype(F32) > -1, cf, F32(0)).astype(F32))


# ---- 1c: the combine ---------------------------------------------------------------------------------------------------------------------
def adaptive_weight(nll_grads, g_grads, disc_weight=1.0):
    """clamp(|nll_grads| / (|g_grads| + 1e-4), 0, 1e4) * disc_weight"""
    a = np.sqrt((nll_grads.astype(np.float64) ** 2).sum())
    b = np.sqrt((g_grads.astype(np.float64) ** 2).sum())
    return float(np.clip(a / (b + 1e-4), 0.0, 1e4)) * float(disc_weight)


def generator_loss(nll_loss, g_loss, codebook_loss, nll_grads, g_grads, global_step, disc_start, disc_factor=1.0, disc_weight=1.0,
                   codebook_weight=1.0, face_loss=0.0, object_loss=0.0):
    """-> (loss, d_weight): loss_img.py:109-111"""
    d_w = adaptive_weight(nll_grads, g_grads, disc_weight)
    loss = float(nll_loss) + d_w * gate(global_step, disc_start, disc_factor) * float(g_loss) \
        + float(codebook_weight) * float(np.asarray(codebook_loss, dtype=np.float64).mean()) + float(face_loss) + float(object_loss)
    return loss, d_w


def combine_backward(g, c_g, codebook_weight, n_codebook):
    """the fp32 gradients of (nll / face / object, g_loss, each element of codebook_loss) for the stored coefficient c_g = d_weight * gate"""
    return F32(g), F32(g) * F32(c_g), F32(g) * (F32(codebook_weight) / F32(n_codebook))
