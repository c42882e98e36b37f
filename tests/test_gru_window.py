"""The stepping core of the learners' GRU windows (mfg_amd/gru_window.py): forward_steps / backward_steps driven directly
on every layout the learners hand them, against an f64 loop over tests/learn_ref.gru_fwd (the recurrent matmul in f64,
autograd through that loop for the gradients).

R = 6 rows, T in {1, 3}, hd in {5, 37}; layouts: batch-major, entry-major (views of [T, R, .] buffers), gi / dgi as
the upper column slice of an [R, T, 3 (4 + hd)] buffer, 3-D weights with G = 3 (two rows per group, distinct biases), a
stride-0 keep, dout = None, h0 with a padded row stride, and all of them at once. keep restarts rows 1 and 3 at entry 1
and row 2 at entry 0. Every written buffer has sentinel pad columns and a pad row, asserted untouched.

Criteria (the project's own):
  * CPU (the tensor path): tests/test_marl.py test_fused_gru_window_matches_cells' tolerances, forward rtol 1e-5 /
    atol 1e-6, gradients rtol 1e-4 / atol 1e-6;
  * GPU (the kernel path): tests/test_gpu_learn_kernels.py's, the kernel path's largest error against f64 is at most 4
    times the f32 tensor path's on the device, plus 1e-7, per output.
"""
from types import SimpleNamespace

import pytest
import torch

import learn_ref as R_
from mfg_amd import gru_window
from mfg_amd.marl import BatchedA2C, RecurrentAC, _GRUWindow, _GRUWindowSavedT

R, FILL, PAD = 6, -7.0, 2
LAYOUTS = {
    'batch': {},
    'entry': dict(entry=True),
    'slice': dict(lo=12),
    'grouped': dict(G=3),
    'keep0': dict(keep0=True),
    'no_dout': dict(dout=False),
    'h0_pad': dict(h0_pad=3),
    'all': dict(entry=True, lo=12, G=3, h0_pad=3),
}
CASES = [(t, hd, name) for t in (1, 3) for hd in (5, 37) for name in LAYOUTS]
SV = ('hp', 'r', 'z', 'n', 'ghn')


class Win:
    """An [R, T, c] window view (batch- or entry-major, columns lo.. of a buffer `lo` columns wider) inside a buffer
    with PAD more columns and one more row, all at a sentinel."""

    def __init__(self, t, c, dev, entry=False, lo=0, value=None):
        shape = (t, R + 1, lo + c + PAD) if entry else (R + 1, t, lo + c + PAD)
        self.buf = torch.full(shape, FILL, dtype=torch.float32, device=dev)
        self.view = (self.buf.transpose(0, 1) if entry else self.buf)[:R, :, lo:lo + c]
        self.own = torch.zeros(shape, dtype=torch.bool, device=dev)
        (self.own.transpose(0, 1) if entry else self.own)[:R, :, lo:lo + c] = True
        if value is not None:
            self.view.copy_(value)

    def intact(self):
        return bool((self.buf[~self.own] == FILL).all())


def make_case(t, hd, G=0, keep0=False, dout=True, **_):
    """The inputs in f32 on the CPU: GRU-initialised weights (uniform in +-1/sqrt(hd)), N(0, 1) gates and gradients."""
    g = torch.Generator().manual_seed(100 * t + hd + G)
    k = hd ** -0.5
    lead = (G,) if G else ()
    c = dict(t=t, hd=hd, G=G, gi=torch.randn((R, t, 3 * hd), generator=g),
             wh=(torch.rand(lead + (3 * hd, hd), generator=g) * 2 - 1) * k,
             bh=(torch.rand(lead + (3 * hd,), generator=g) * 2 - 1) * k,
             h0=torch.rand((R, hd), generator=g) * 2 - 1,
             dout=torch.randn((R, t, hd), generator=g) if dout else None)
    keep = torch.ones((R, t))
    if not keep0:
        keep[2, 0] = 0.0
        if t > 1:
            keep[1, 1] = keep[3, 1] = 0.0
    c['keep'] = keep
    return c


def reference(c):
    """hs, the five saved activations, dgi and dgh in f64: a loop over learn_ref.gru_fwd, gradients by autograd (dgh as
    the gradient of a zero added to the recurrent gates' bias at every step)."""
    t, hd, G = c['t'], c['hd'], c['G']
    d = {k: v.double() for k, v in c.items() if torch.is_tensor(v)}
    gi = d['gi'].clone().requires_grad_()
    eps = torch.zeros((R, t, 3 * hd), dtype=torch.float64, requires_grad=True)
    bh = d['bh'].repeat_interleave(R // G, 0) if G else d['bh'].expand(R, 3 * hd)
    h, cols = d['h0'], []
    for s in range(t):
        if G:
            gh0 = torch.einsum('grh,gkh->grk', h.view(G, R // G, hd), d['wh']).reshape(R, 3 * hd)
        else:
            gh0 = h @ d['wh'].t()
        out = R_.gru_fwd(gi[:, s], gh0, bh + eps[:, s], h, d['keep'][:, s])
        h = out[0]
        cols.append(out)
    ref = {k: torch.stack([col[i] for col in cols], 1).detach() for i, k in enumerate(('hs',) + SV)}
    if c['dout'] is None:
        ref['dgi'], ref['dgh'] = torch.zeros_like(gi), torch.zeros_like(gi)
    else:
        hs = torch.stack([col[0] for col in cols], 1)
        ref['dgi'], ref['dgh'] = torch.autograd.grad((hs * d['dout']).sum(), [gi, eps])
    return ref


def run(c, dev, entry=False, lo=0, h0_pad=0, keep0=False, **_):
    """forward_steps then backward_steps on the layout's views: (the outputs, every written buffer's Win)."""
    t, hd = c['t'], c['hd']
    gi = Win(t, 3 * hd, dev, entry, lo, c['gi'])
    keep = torch.ones(1, device=dev).expand(R, t) if keep0 else Win(t, 1, dev, entry, 0, c['keep'][..., None]).view[..., 0]
    h0 = torch.full((R, hd + h0_pad), FILL, device=dev)
    h0[:, :hd] = c['h0']
    wh, bh = c['wh'].to(dev), c['bh'].to(dev)
    wins = {k: Win(t, hd, dev, entry) for k in ('hs',) + SV}
    sv = [wins[k].view for k in SV]
    assert len({v.stride(0) for v in sv}) == 1
    gru_window.forward_steps(gi.view, keep, h0[:, :hd], wh, bh, wins['hs'].view, sv)
    wins['dgi'], wins['dgh'] = Win(t, 3 * hd, dev, entry, lo), Win(t, 3 * hd, dev, entry)
    dout = None if c['dout'] is None else Win(t, hd, dev, entry, 0, c['dout']).view
    gru_window.backward_steps(dout, keep, sv, wh, wins['dgi'].view, wins['dgh'].view)
    assert bool((gi.view.cpu() == c['gi']).all()) and gi.intact()  # read in place, not written
    return {k: w.view.detach().cpu().clone() for k, w in wins.items()}, wins


@pytest.mark.parametrize('t,hd,name', CASES)
def test_steps_match_f64_reference_cpu(t, hd, name):
    c = make_case(t, hd, **LAYOUTS[name])
    got, wins = run(c, 'cpu', **LAYOUTS[name])
    ref = reference(c)
    for k, w in wins.items():
        assert w.intact(), k
        rtol = 1e-4 if k in ('dgi', 'dgh') else 1e-5
        err = (got[k].double() - ref[k]).abs().max()
        assert torch.allclose(got[k].double(), ref[k], rtol=rtol, atol=1e-6), (k, float(err))


def _pair_inputs(n, t, dev='cpu'):
    torch.manual_seed(7)
    net = RecurrentAC(40, 5, 24, 8, 8, 6, 4, use_agent_embedding=False).to(dev)
    ws = [p for g in (net.gru_actor, net.gru_critic) for p in (g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0)]
    x = torch.randn(n, t, 24, device=dev)
    keep = (torch.rand(n, t, device=dev) > 0.3).float()
    return net, ws, x, keep, torch.randn(n, 8, device=dev), torch.randn(n, 6, device=dev)


def test_pair_backward_entry_major_matches_batch_major():
    """The two-GRU backward fed entry-major views (_GRUWindowSavedT, on a forward stored entry-major by forward_steps)
    against _GRUWindow on the same data batch-major: outputs and all nine gradients (not bit equality: CPU elementwise
    kernels round an element by its position in the tensor)."""
    n, t = 6, 3
    net, ws, x, keep, h0a, h0c = _pair_inputs(n, t)
    da, dc = torch.randn(n, t, 8), torch.randn(n, t, 6)
    xb = x.clone().requires_grad_()
    out_a, out_c = _GRUWindow.apply(xb, keep, h0a, h0c, *ws)
    want = torch.autograd.grad((out_a * da).sum() + (out_c * dc).sum(), [xb, *ws])
    # the same window entry-major: the input gates and the stored forward as the acting steps lay them out
    xe = x.transpose(0, 1).reshape(t * n, -1).clone().requires_grad_()
    wi, bi = torch.cat([ws[0], ws[4]], 0), torch.cat([ws[2], ws[6]], 0)
    gi = torch.addmm(bi, xe.detach(), wi.t()).view(t, n, -1).transpose(0, 1)
    saved, lo = [], 0
    for h0, wh, bh in ((h0a, ws[1], ws[3]), (h0c, ws[5], ws[7])):
        hd = wh.shape[1]
        hs, sv = torch.empty(t, n, hd), torch.empty(5, t, n, hd)
        gru_window.forward_steps(gi[:, :, lo:lo + 3 * hd], keep, h0, wh.detach(), bh.detach(), hs.transpose(0, 1),
                                 sv.transpose(1, 2))
        saved += [hs, sv]
        lo += 3 * hd
    ea, ec = _GRUWindowSavedT.apply(xe, keep.t().contiguous(), (saved[0], saved[2], saved[1], saved[3]), *ws)
    assert torch.allclose(ea.view(t, n, -1).transpose(0, 1), out_a, rtol=1e-5, atol=1e-6)
    assert torch.allclose(ec.view(t, n, -1).transpose(0, 1), out_c, rtol=1e-5, atol=1e-6)
    flat = lambda v: v.transpose(0, 1).reshape(t * n, -1)  # noqa: E731
    got = torch.autograd.grad((ea * flat(da)).sum() + (ec * flat(dc)).sum(), [xe, *ws])
    got = (got[0].view(t, n, -1).transpose(0, 1),) + got[1:]
    for i, (a, b) in enumerate(zip(got, want)):
        assert torch.allclose(a, b, rtol=1e-4, atol=1e-6), (i, float((a - b).abs().max()))


# ---------------------------------------------------------------------------------------------------------------------
# the same cases on the device, through the kernels
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('t,hd,name', CASES)
def test_steps_match_f64_reference_gpu(t, hd, name, monkeypatch):
    c = make_case(t, hd, **LAYOUTS[name])
    ref = reference(c)
    got, wins = run(c, 'cuda', **LAYOUTS[name])
    torch.cuda.synchronize()
    for k, w in wins.items():
        assert w.intact(), k
    monkeypatch.setattr(gru_window, 'use_kernels', lambda x: False)  # the f32 tensor path on the device
    f32, _ = run(c, 'cuda', **LAYOUTS[name])
    for k in got:
        e_ker, e_f32 = float((got[k].double() - ref[k]).abs().max()), float((f32[k].double() - ref[k]).abs().max())
        print(f'gru_window.{name}.t{t}.hd{hd}.{k}: kernel err = {e_ker}, f32 torch err = {e_f32}')
        assert e_ker <= 4 * e_f32 + 1e-7, (k, e_ker, e_f32)


@pytest.mark.gpu
def test_acting_step_is_forward_steps_on_one_entry():
    """BatchedA2C._gru_step at entries 0 and 1 of a T = 2, N = 6 pair of entry-major window buffers: its hs / sv slices
    are bit-equal to forward_steps over the same input gates batch-major (the same arithmetic at other addresses)."""
    n, t = 6, 2
    net, ws, x, _, h0a, h0c = _pair_inputs(n, t, 'cuda')
    a = SimpleNamespace(net=net, N=n, _one=torch.ones(1, device='cuda'), ha=h0a[:, None].clone(), hc=h0c[:, None].clone(),
                        hs_a=torch.full((t, n, 8), FILL, device='cuda'), hs_c=torch.full((t, n, 6), FILL, device='cuda'),
                        sv_a=torch.full((5, t, n, 8), FILL, device='cuda'),
                        sv_c=torch.full((5, t, n, 6), FILL, device='cuda'))
    wi, bi = torch.cat([ws[0], ws[4]], 0), torch.cat([ws[2], ws[6]], 0)
    gi = torch.empty((n, t, wi.shape[0]), device='cuda')
    with torch.no_grad():
        for s in range(t):
            BatchedA2C._gru_step(a, x[:, s].contiguous(), s)
            if s == 0:
                assert bool((a.hs_a[1] == FILL).all()) and bool((a.sv_c[:, 1] == FILL).all())  # entry 1 untouched
            a.ha, a.hc = a.hs_a[s][:, None].clone(), a.hs_c[s][:, None].clone()  # no restart
            gi[:, s] = torch.addmm(bi, x[:, s].contiguous(), wi.t())  # the step's own input-gate GEMM
        lo = 0
        for h0, wh, bh, hs_e, sv_e in ((h0a, ws[1], ws[3], a.hs_a, a.sv_a), (h0c, ws[5], ws[7], a.hs_c, a.sv_c)):
            hd = wh.shape[1]
            hs, sv = torch.empty((n, t, hd), device='cuda'), torch.empty((5, n, t, hd), device='cuda')
            gru_window.forward_steps(gi[:, :, lo:lo + 3 * hd], torch.ones((n, t), device='cuda'), h0, wh, bh, hs, sv)
            assert torch.equal(hs_e.transpose(0, 1), hs) and torch.equal(sv_e.transpose(1, 2), sv)
            lo += 3 * hd
