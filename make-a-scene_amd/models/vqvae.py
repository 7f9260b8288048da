"""``VQBASE`` behind the reference's surface (reference models/vqvae.py:8-39): same constructor
(``ddconfig, n_embed, embed_dim, init_steps, reservoir_size``), same submodule names and
``state_dict`` keys (348 entries for conf/img_config.yaml), same ``encode/decode/decode_code/forward``.
encoder -> quant_conv (1x1 conv + SyncBatchNorm) -> Codebook -> post_quant_conv -> decoder, every
convolution / norm (GroupNorm and, since round 5, the SyncBatchNorm) / lookup on the hand-written gfx950 kernels of libmas_hip.so."""
import torch
from torch import nn

from .modules import Codebook, Conv2d, Decoder, Encoder, SyncBatchNorm


class VQBASE(nn.Module):
    def __init__(self, ddconfig, n_embed, embed_dim, init_steps, reservoir_size):
        super(VQBASE, self).__init__()
        self.encoder = Encoder(**ddconfig)
        self.decoder = Decoder(**ddconfig)
        self.quantize = Codebook(n_embed, embed_dim, beta=0.25, init_steps=init_steps, reservoir_size=reservoir_size)
        # the latent tail is stored fp32 end to end: indices come from fp32 z
        qc = Conv2d(ddconfig["z_channels"], embed_dim, 1)
        qc.in_dtype = qc.out_dtype = torch.float32
        self.quant_conv = nn.Sequential(qc, SyncBatchNorm(embed_dim))
        self.post_quant_conv = Conv2d(embed_dim, ddconfig["z_channels"], 1)
        self.post_quant_conv.in_dtype = self.post_quant_conv.out_dtype = torch.float32

    def encode(self, x):
        h = self.encoder(x)
        h = self.quant_conv(h)
        quant, emb_loss, info = self.quantize(h)
        return quant, emb_loss

    @torch.no_grad()
    def encode_to_indices(self, x):
        """Frozen-VQ tokenisation for stage 2: images -> codebook indices [B, h*w] (int64), row-major over
        the latent grid -- what ``train.py:141-145`` consumes as ``img_token`` / ``seg_token``.  The reference's ``encode``
        drops the indices (vqvae.py:23-24); this is the same encoder -> quant_conv -> Codebook lookup, keeping them.  Call in
        ``eval()`` mode (SyncBatchNorm running statistics; the codebook warm-up schedule untouched)."""
        if self.training:
            raise RuntimeError("encode_to_indices: tokenise with the frozen model in eval() mode")
        h = self.quant_conv(self.encoder(x))
        _, _, idx = self.quantize(h)
        return idx.view(x.shape[0], -1)

    def decode(self, quant):
        quant = self.post_quant_conv(quant)
        dec = self.decoder(quant)
        return dec

    def decode_code(self, code_b):
        # the reference calls a method that does not exist (vqvae.py:32 `embed_code`); the intended
        # lookup is get_codebook_entry (modules.py:519) on a square token grid
        b, n = code_b.shape[0], code_b.reshape(code_b.shape[0], -1).shape[1]
        side = int(round(n ** 0.5))
        quant_b = self.quantize.get_codebook_entry(code_b.reshape(b, -1), (b, side, side, self.quantize.codebook_dim))
        return self.decode(quant_b)

    @torch.no_grad()
    def decode_to_labels(self, code_b, layout=None, thresholds=None):
        """VQ-SEG tokens -> the scene as ``mas_hip.seglabels.SegLabels``: ``decode_code`` and then the reference Visualizer's reading of the
        logits (log_utils.py:55-67; ``ops.seg_classify``).  ``layout`` / ``thresholds`` as ``SegLabels.from_logits``.  Call in ``eval()``
        mode, like ``encode_to_indices``: tokens -> scene -> tokens closes with it."""
        if self.training:
            raise RuntimeError("decode_to_labels: decode with the frozen model in eval() mode")
        from mas_hip.seglabels import SegLabels
        return SegLabels.from_logits(self.decode_code(code_b), layout, thresholds)

    @torch.no_grad()
    def reconstruct_labels(self, x, layout=None, thresholds=None):
        """a segmentation map (``SegLabels`` or dense) -> its reconstruction as ``SegLabels``: ``forward``'s logits read by
        ``SegLabels.from_logits``.  ``eval()`` mode only."""
        if self.training:
            raise RuntimeError("reconstruct_labels: reconstruct with the frozen model in eval() mode")
        from mas_hip.seglabels import SegLabels
        quant, _ = self.encode(x)
        return SegLabels.from_logits(self.decode(quant), layout, thresholds)

    @torch.no_grad()
    def decode_to_images(self, code_b, lo=-1.0, hi=1.0):
        """VQ-IMG tokens -> pictures ``uint8 [B, H, W, C]``: ``decode_code`` and then ``ops.image_bytes`` with the range ``[lo, hi]`` the
        model was trained in.  ``eval()`` mode only, like ``decode_to_labels``."""
        if self.training:
            raise RuntimeError("decode_to_images: decode with the frozen model in eval() mode")
        from mas_hip import ops
        from mas_hip.imgmetrics import byte_range
        lo, hi = byte_range(lo, hi, "decode_to_images")
        return ops.image_bytes(self.decode_code(code_b), lo, hi)

    @torch.no_grad()
    def reconstruction_metrics(self, x, lo=-1.0, hi=1.0, usage=None):
        """images ``x`` -> ``(ImageAgreement, CodeUsage)`` of their reconstruction (``mas_hip.imgmetrics``): one pass of encoder ->
        quant_conv -> lookup, keeping the indices, then post_quant_conv -> decoder; ``ops.image_agreement(reconstruction, x, lo, hi)`` and
        ``ops.code_usage(indices, n_embed, out=usage)`` -- pass the ``CodeUsage`` of the previous batch as ``usage`` to accumulate over a
        validation set.  Nothing synchronises with the host.  ``eval()`` mode only."""
        if self.training:
            raise RuntimeError("reconstruction_metrics: measure the frozen model in eval() mode")
        from mas_hip import ops
        from mas_hip.imgmetrics import CodeUsage, byte_range
        from mas_hip.seglabels import SegLabels
        if isinstance(x, SegLabels):
            raise TypeError("reconstruction_metrics: pictures only; for a segmentation map use reconstruct_labels + ops.seg_agreement")
        lo, hi = byte_range(lo, hi, "reconstruction_metrics")
        n_embed = self.quantize.codebook_size
        if usage is not None and (not isinstance(usage, CodeUsage) or usage.n_embed != n_embed):
            raise ValueError(f"reconstruction_metrics: usage must be a CodeUsage of the codebook's {n_embed} codes")
        quant, _, idx = self.quantize(self.quant_conv(self.encoder(x)))
        return ops.image_agreement(self.decode(quant), x, lo, hi), ops.code_usage(idx, n_embed, out=usage)

    def forward(self, input):
        quant, diff = self.encode(input)
        dec = self.decode(quant)
        return dec, diff
