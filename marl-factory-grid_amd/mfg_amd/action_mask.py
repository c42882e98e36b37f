"""Action masks: which of an agent's actions would be valid if it acted now (include/mfg.h mfg_action_mask).

The engine answers with one 32-bit word per (env, agent): bit s is set exactly when s < n_actions[agent] and a step
from the env's state as it stands, with that agent executing slot s before any other agent has acted, would report
the action valid (the ev_act row 0x80 | 1). The words travel as int32 tensors (torch has no uint32 arithmetic); bit 31
is then the sign bit, which the helpers here mask off. DESIGN §8g has the rules per action class and the limit: the
mask is exact for the first agent to act and a sound filter for the others, since an earlier agent of the same step
may still toggle a door or move a blocking agent in.

This module holds the host-side views of the words; none of it needs a GPU.
"""
import numpy as np


def dense_mask(words, n_max):
    """Words [...] (int32 torch tensor or numpy array) -> bool [..., n_max]: element s is bit s of the word."""
    if isinstance(words, np.ndarray):
        w = words.astype(np.int64) & 0xFFFFFFFF
        return ((w[..., None] >> np.arange(n_max, dtype=np.int64)) & 1).astype(bool)
    import torch
    w = words.to(torch.int64) & 0xFFFFFFFF
    return ((w[..., None] >> torch.arange(n_max, device=words.device, dtype=torch.int64)) & 1).bool()


def agent_masks(row, n_actions):
    """One env's words [A] -> a list with one numpy bool array of length n_actions[a] per agent."""
    row = np.asarray(row)
    return [dense_mask(row[a:a + 1], int(n))[0] for a, n in enumerate(n_actions)]


def masked_logits(logits, words, n_act=None):
    """logits [..., n] with the entries whose bit is clear set to -inf (an action of probability 0). A row whose word
    has no bit set among the first n_act (default n) columns is left as it is: it is acted unmasked."""
    import torch
    n = logits.shape[-1]
    bits = dense_mask(words, n)
    if n_act is not None and n_act < n:
        bits = bits & (torch.arange(n, device=logits.device) < n_act)
    keep = bits | ~bits.any(-1, keepdim=True)
    return torch.where(keep, logits, torch.full_like(logits, float('-inf')))
