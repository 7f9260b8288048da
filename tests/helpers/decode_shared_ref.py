"""float64 numpy restatement of the shared-prompt decode attention (make-a-scene_amd/csrc/attn_decode_shared.hip) on top of
decode_split_ref: the states of the prompt block's key ranges, then the states of the row's own key ranges, merged by ``combine`` in
that order -- the algebra the kernel pair implements, and the GPU tests' second reference."""
import numpy as np

import decode_split_ref as R


def shared_states(q, prompt_k, prompt_v, own_k, own_v, prompt_splits, own_splits):
    """[(m, l, o)]: ``prompt_splits`` states of the prompt_len prompt keys, then ``own_splits`` states of the L_own own keys; the
    ranges of both are ``decode_split_ref.split_ranges``.  q [hd] (already scaled), prompt_k / prompt_v [prompt_len, hd],
    own_k / own_v [L_own, hd]."""
    st = [R.partial_state(q, prompt_k, prompt_v, b, e) for b, e in R.split_ranges(prompt_k.shape[0], prompt_splits)]
    return st + [R.partial_state(q, own_k, own_v, b, e) for b, e in R.split_ranges(own_k.shape[0], own_splits)]


def shared_attention(q, prompt_k, prompt_v, own_k, own_v, prompt_splits, own_splits):
    """softmax over the prompt keys followed by the own keys, computed range by range (float64)"""
    return R.combine(shared_states(q, prompt_k, prompt_v, own_k, own_v, prompt_splits, own_splits))


def plain_shared_attention(q, prompt_k, prompt_v, own_k, own_v):
    """plain softmax(qK^T)V over the concatenated keys"""
    return R.plain_attention(q, np.concatenate([prompt_k, own_k]), np.concatenate([prompt_v, own_v]))
