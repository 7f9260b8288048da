"""Image prompts for ``MakeAScene.generate(img_tokens=..., keep=...)``: which image positions keep their given token while the others
are sampled.  ``border_keep_mask`` builds the mask of one image from ruDALL-E's four borders, ``common_prefix`` is the number of leading
positions every row keeps -- the part ``generate`` moves from the token loop into the prefill."""
import torch


def border_keep_mask(tokens_per_dim, up=0, down=0, left=0, right=0):
    """bool [tokens_per_dim ** 2] (row-major, the order ``generate`` samples in): True inside the kept borders, given in token rows
    (``up`` from the top, ``down`` from the bottom) and token columns (``left``, ``right``), as ruDALL-E's image prompts take them.
    Borders overlap freely; one that is at least the grid keeps everything."""
    n = int(tokens_per_dim)
    if n < 1:
        raise ValueError(f"border_keep_mask: tokens_per_dim {tokens_per_dim} must be positive")
    borders = dict(up=up, down=down, left=left, right=right)
    for name, w in borders.items():
        if isinstance(w, bool) or int(w) != w or w < 0:
            raise ValueError(f"border_keep_mask: {name}={w!r} is not a number of token rows / columns >= 0")
    up, down, left, right = (min(int(w), n) for w in (up, down, left, right))
    mask = torch.zeros((n, n), dtype=torch.bool)
    mask[:up, :] = True
    mask[n - down:, :] = True
    mask[:, :left] = True
    mask[:, n - right:] = True
    return mask.reshape(n * n)


def common_prefix(keep):
    """m = the minimum over the rows of ``keep`` (bool [B, L]) of the length of the leading all-True run, capped at L - 1 (the last
    position always goes through the sampler, so a call always ends with a token step).  Read on the host: one synchronisation when
    ``keep`` lives on a GPU, none for a CPU tensor."""
    if keep.dim() != 2 or keep.dtype != torch.bool:
        raise ValueError("common_prefix: keep is a bool tensor [B, L]")
    b, length = keep.shape
    if b == 0 or length == 0:
        return 0
    runs = keep.to("cpu").to(torch.int64).cumprod(dim=1).sum(dim=1)
    return min(int(runs.min()), length - 1)
