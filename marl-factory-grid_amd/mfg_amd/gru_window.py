"""The stepping core of the learners' GRU windows (layer 0 of torch.nn.GRU, gate order r, z, n): one forward and one
backward recurrence over T entries of R rows, for every layout the learners keep a window in.

A window tensor is an ``[R, T, C]`` view with unit stride in C, one row stride and one time stride, both read from the
view: batch-major buffers (``[R, T, C]``), entry-major ones (``[T, R, C].transpose(0, 1)``), a column slice of a wider
gate buffer and a single entry (``[t:t + 1]``) are the same object here. The kernels take a pointer at the entry and the
row stride (include/mfg_learn.h); ``_at`` is the only place the time index meets an address.

The recurrent weight is 2-D (one GRU for all rows: ``addmm``) or 3-D ``[G, 3hd, hd]`` (G GRUs, row block g of R / G
rows by GRU g: ``bmm`` / ``baddbmm``). On the GPU in fp32 the elementwise work of a step is one HIP kernel
(``mfg_gru_fwd_step``, ``mfg_gru_fwd_step_grouped``, ``mfg_gru_bwd_step``); everything else takes the tensor code below
(the same formulas). The window's GEMMs (input gates, weight gradients) stay with the callers: ``marl._GRUWindow``,
``marl._GRUWindowSavedT``, ``seac._GRUWindowG`` and ``marl.BatchedA2C._gru_step``.
"""
import torch

from . import learn_lib


def use_kernels(x):
    """The GRU steps run as HIP kernels on the GPU (fp32); other tensors take the tensor code. Callers look this up
    through the module, so a test that patches it reaches every window."""
    return x.is_cuda and x.dtype == torch.float32


def blin(x, w, b):
    """Per-agent x W^T + b: x [A, M, in], w [A, out, in], b [A, out] -> [A, M, out]: one baddbmm over agents on the
    GPU; on the CPU one addmm per agent, the very call of RecurrentAC's layers (a batched GEMM there rounds in another
    order, and the CPU forward is pinned bit-equal to the separate modules; the operands are copied out of the stack
    because the CPU GEMM's summation order also depends on their alignment)."""
    if not x.is_cuda:
        return torch.stack([torch.addmm(b[g].clone(), x[g].clone(), w[g].clone().t()) for g in range(x.shape[0])])
    return torch.baddbmm(b[:, None], x, w.transpose(1, 2))


def _at(v, s):
    """The address of v[:, s] for a window view v [R, T, C] or [R, T]."""
    return v.data_ptr() + s * v.stride(1) * v.element_size()


def _blocks(v, wh):
    """Rows v [R, C] as the [G, R / G, C] row blocks of a 3-D weight."""
    return v.view(wh.shape[0], -1, v.shape[-1])


def forward_steps(gi, keep, h0, wh, bh, hs, sv):
    """h_s = GRU(gi[:, s], h_{s-1} keep[:, s]) for s < T, h_{-1} = h0. gi [R, T, 3hd] = x W_ih^T + b_ih, keep [R, T]
    (0 = a restart at that entry; any strides, 0 included), h0 [R, hd] (any row stride), wh [3hd, hd] with bh [3hd], or
    wh [G, 3hd, hd] with bh [G, 3hd]. Written in place: hs [R, T, hd] and sv, five [R, T, hd] views of one row stride
    (hp, r, z, n, gh_n: the backward's inputs). Takes no copies."""
    hp_s, r_s, z_s, n_s, ghn_s = (sv[k] for k in range(5))  # (a [5, R, T, hd] tensor or a list: no unbind views)
    R, T, hd = hs.shape
    grouped, h = wh.dim() == 3, h0
    if use_kernels(gi):  # per step: the recurrent GEMM + one fused elementwise kernel
        st = learn_lib.stream(gi.device)
        whT = wh.transpose(-1, -2)
        for s in range(T):
            gh0 = torch.bmm(_blocks(h, wh), whT) if grouped else h @ whT
            head = (_at(gi, s), gi.stride(0), gh0.data_ptr(), bh.data_ptr())
            tail = (h.data_ptr(), h.stride(0), _at(keep, s), keep.stride(0), _at(hs, s), hs.stride(0), _at(hp_s, s),
                    _at(r_s, s), _at(z_s, s), _at(n_s, s), _at(ghn_s, s), hp_s.stride(0), R, hd, st)
            if grouped:  # a row's recurrent bias is its row block's
                learn_lib.call('mfg_gru_fwd_step_grouped', *head, R // wh.shape[0], *tail)
            else:
                learn_lib.call('mfg_gru_fwd_step', *head, *tail)
            h = hs[:, s]
        return
    for s in range(T):
        hp = h * keep[:, s:s + 1]
        gh = blin(_blocks(hp, wh), wh, bh).view(R, -1) if grouped else torch.addmm(bh, hp, wh.t())
        g = gi[:, s]
        r = torch.sigmoid(g[:, :hd] + gh[:, :hd])
        z = torch.sigmoid(g[:, hd:2 * hd] + gh[:, hd:2 * hd])
        ghn = gh[:, 2 * hd:]
        nn_ = torch.tanh(g[:, 2 * hd:] + r * ghn)
        h = nn_ + z * (hp - nn_)  # (1 - z) n + z h
        for dst, v in zip((hs, hp_s, r_s, z_s, n_s, ghn_s), (h, hp, r, z, nn_, ghn)):
            dst[:, s] = v


def backward_steps(dout, keep, sv, wh, dgi, dgh):
    """The chain rule of forward_steps from s = T - 1 down on its saved sv: dh_s = dout[:, s] + keep[:, s + 1] dhp_{s+1}
    (dout [R, T, hd] or None: no gradient into the outputs), written in place dgi = [dr, dz, dn] and dgh = [dr, dz,
    dn r] (both [R, T, 3hd]), then dhp_s = dh_s z + dgh[:, s] W_hh, one addmm or baddbmm. h0 gets no gradient."""
    hp_s, r_s, z_s, n_s, ghn_s = sv
    R, T, hd = hp_s.shape
    grouped = wh.dim() == 3

    def chain(acc, s):  # acc + dgh[:, s] W_hh
        if grouped:
            return torch.baddbmm(_blocks(acc, wh), _blocks(dgh[:, s], wh), wh)
        return torch.addmm(acc, dgh[:, s], wh)

    if use_kernels(hp_s):  # per step: one fused elementwise kernel + the recurrent GEMM
        st = learn_lib.stream(hp_s.device)
        dhp = None
        for s in range(T - 1, -1, -1):
            dhz = torch.empty((R, hd), dtype=hp_s.dtype, device=hp_s.device)
            learn_lib.call('mfg_gru_bwd_step', None if dout is None else _at(dout, s),
                           0 if dout is None else dout.stride(0), learn_lib.ptr(dhp),
                           None if dhp is None else _at(keep, s + 1), keep.stride(0), _at(r_s, s), _at(z_s, s),
                           _at(n_s, s), _at(ghn_s, s), _at(hp_s, s), hp_s.stride(0), _at(dgi, s), dgi.stride(0),
                           _at(dgh, s), dgh.stride(0), dhz.data_ptr(), R, hd, st)
            dhp = chain(dhz, s)
        return
    carry = torch.zeros((R, hd), dtype=hp_s.dtype, device=hp_s.device)
    for s in range(T - 1, -1, -1):
        dh = carry if dout is None else dout[:, s] + carry
        r, z, nn_, ghn, hp = r_s[:, s], z_s[:, s], n_s[:, s], ghn_s[:, s], hp_s[:, s]
        dn = dh * (1.0 - z) * (1.0 - nn_ * nn_)
        dz = dh * (hp - nn_) * z * (1.0 - z)
        dr = dn * ghn * r * (1.0 - r)
        dgi[:, s] = torch.cat([dr, dz, dn], -1)
        dgh[:, s] = torch.cat([dr, dz, dn * r], -1)
        carry = chain(dh * z, s).view(R, hd) * keep[:, s:s + 1]
