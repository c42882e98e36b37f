"""Plain references for the learner-side kernels of include/mfg_learn.h, in whatever dtype their inputs have: f64 on the
CPU is the reference of tests/test_gpu_learn_kernels.py, f32 on the device is the tensor code whose error the kernels'
error is measured against. tests/test_learn_ref.py pins them to torch.nn.GRUCell and to autograd without a GPU.
"""
import torch

U_LAST = 1.0 - 2.0 ** -24  # the largest f32 below 1: the top of the sampler's u range


# ---------------------------------------------------------------------------------------------------------------------
# one GRU step (gate order r, z, n), the header's formulas
# ---------------------------------------------------------------------------------------------------------------------
def gru_fwd(gi, gh0, bh, h, keep):
    """mfg_gru_fwd_step: gi, gh0 [n, 3hd], bh [3hd] or one per row [n, 3hd], h [n, hd] or None (a zero state), keep [n]
    -> (h_out, hp, r, z, n, gh_n), each [n, hd]."""
    hd = gi.shape[-1] // 3
    kp = keep[:, None]
    hp = torch.zeros_like(gi[:, :hd]) if h is None else h * kp
    gh = gh0 * kp + bh
    r = torch.sigmoid(gi[:, :hd] + gh[:, :hd])
    z = torch.sigmoid(gi[:, hd:2 * hd] + gh[:, hd:2 * hd])
    n = torch.tanh(gi[:, 2 * hd:] + r * gh[:, 2 * hd:])
    return n + z * (hp - n), hp, r, z, n, gh[:, 2 * hd:]


def gru_bwd(gi, gh, hp, dh):
    """Autograd of the forward formulas with respect to gi and gh = keep gh0 + bh (both [n, 3hd]) for an output
    gradient dh [n, hd]: (dgi, dgh, dhz = dh z)."""
    hd = gi.shape[-1] // 3
    gi, gh = gi.detach().clone().requires_grad_(), gh.detach().clone().requires_grad_()
    r = torch.sigmoid(gi[:, :hd] + gh[:, :hd])
    z = torch.sigmoid(gi[:, hd:2 * hd] + gh[:, hd:2 * hd])
    n = torch.tanh(gi[:, 2 * hd:] + r * gh[:, 2 * hd:])
    dgi, dgh = torch.autograd.grad(n + z * (hp - n), [gi, gh], dh)
    return dgi, dgh, dh * z.detach()


def gru_bwd_formulas(dh, r, z, n, ghn, hp):
    """mfg_gru_bwd_step's formulas on the saved activations: (dgi, dgh, dhz)."""
    dn = dh * (1.0 - z) * (1.0 - n * n)
    dz = dh * (hp - n) * z * (1.0 - z)
    dr = dn * ghn * r * (1.0 - r)
    return torch.cat([dr, dz, dn], -1), torch.cat([dr, dz, dn * r], -1), dh * z


def gru_inputs(n, hd, seed=0, t=3):
    """The inputs of one step in f32: gi [n, 3hd], gh0 [n, 3hd], bh [3hd], bh_rows [n, 3hd], h [n, hd], keep [n] in
    {0, 1} with both values present (n > 1), and for the backward dout, dhp_next [n, hd] and keep_next [n]. Every third
    row has |gi| and |gh0| up to 40: r and z reach exactly 0 or 1 in f32 and 1 - n^2 reaches 0."""
    g = torch.Generator().manual_seed(seed + 1000 * n + hd)
    gi, gh0 = torch.randn((n, 3 * hd), generator=g), torch.randn((n, 3 * hd), generator=g)
    big = torch.arange(n) % 3 == 0
    gi[big] = (torch.rand((int(big.sum()), 3 * hd), generator=g) * 2 - 1) * 40
    gh0[big] = (torch.rand((int(big.sum()), 3 * hd), generator=g) * 2 - 1) * 40
    keep = (torch.rand(n, generator=g) < 0.6).float()
    keep_next = (torch.rand(n, generator=g) < 0.6).float()
    if n > 1:
        keep[0], keep[1] = 1.0, 0.0
        keep_next[0], keep_next[1] = 0.0, 1.0
    return dict(gi=gi, gh0=gh0, bh=torch.randn(3 * hd, generator=g) * 0.5,
                bh_rows=torch.randn((n, 3 * hd), generator=g) * 0.5, h=torch.randn((n, hd), generator=g), keep=keep,
                dout=torch.randn((n, hd), generator=g), dhp_next=torch.randn((n, hd), generator=g),
                keep_next=keep_next)


# ---------------------------------------------------------------------------------------------------------------------
# categorical sampling by inversion
# ---------------------------------------------------------------------------------------------------------------------
def sampler_inputs(n, n_act, pad=3, seed=0):
    """logits f32 [n, n_act + pad] and u f32 [n] in [0, 1): N(0, 3^2) logits, every fifth row shifted by +80, every
    seventh row with one logit 120 below its maximum, the pad columns at +1000 (outside the distribution); u uniform
    with 0, 1 - 2^-24 and 2^-30 placed on rows 0, 1, 2 and again from row 1000 on every 997th row in turn."""
    g = torch.Generator().manual_seed(seed + 100 * n_act + (n % 97))
    lg = torch.randn((n, n_act), generator=g) * 3.0
    rows = torch.arange(n)
    lg[rows % 5 == 4] += 80.0
    low = (rows % 7 == 6).nonzero().flatten()
    if n_act > 1 and len(low):
        col = torch.randint(0, n_act, (len(low),), generator=g)
        mx = lg[low].max(-1)
        col = torch.where(col == mx.indices, (col + 1) % n_act, col)  # never the maximum itself
        lg[low, col] = mx.values - 120.0
    logits = torch.full((n, n_act + pad), 1000.0)
    logits[:, :n_act] = lg
    u = torch.rand(n, generator=g)
    special = torch.tensor([0.0, U_LAST, 2.0 ** -30])
    for j in range(min(n, 3)):
        u[j] = special[j]
    at = torch.arange(1000, max(n, 1000), 997)
    u[at] = special[torch.arange(len(at)) % 3]
    assert float(u.max()) < 1.0
    return logits, u


def cdf_pick(logits, u, margin=1e-5):
    """The inversion of the f64 CDF of softmax(logits [n, n_act]) at u [n]: (pick [n], near [n]); near marks a row
    whose u lies within `margin` of a CDF step between two actions, where f32 rounding may pick either neighbour."""
    cdf = torch.softmax(logits.double(), -1).cumsum(-1)
    ud = u.double()[:, None]
    n_act = logits.shape[-1]
    pick = (ud >= cdf).sum(-1).clamp(max=n_act - 1)
    near = ((ud - cdf[:, :-1]).abs() < margin).any(-1)
    return pick, near
