from .vqvae import VQBASE
from .image_prompt import border_keep_mask, common_prefix
