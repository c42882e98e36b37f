"""tests/learn_ref.py, the f64 references of tests/test_gpu_learn_kernels.py, pinned without a GPU: the GRU step against
torch.nn.GRUCell and autograd through it, the CDF sampler's left-out share on the GPU test's inputs, and the tensor-code
loss heads' answer to an infinite logit (the contract the fused heads are tested for on the device)."""
import pytest
import torch

import learn_ref as R
import mfg_amd.evaluate as EV
import mfg_amd.marl as M


def _cell(hd, n, seed):
    """A GRUCell in f64 whose input is gi itself (W_ih = I, b_ih = 0), with its inputs."""
    torch.manual_seed(seed)
    cell = torch.nn.GRUCell(3 * hd, hd).double()
    with torch.no_grad():
        cell.weight_ih.copy_(torch.eye(3 * hd))
        cell.bias_ih.zero_()
    x = R.gru_inputs(n, hd, seed)
    return cell, x['gi'].double(), x['h'].double(), x['dout'].double()


@pytest.mark.parametrize('n,hd', [(1, 1), (7, 37), (5, 128)])
def test_gru_reference_is_grucell(n, hd):
    cell, gi, h, _ = _cell(hd, n, 1)
    gh0 = h @ cell.weight_hh.t()
    out = R.gru_fwd(gi, gh0.detach(), cell.bias_hh.detach(), h, torch.ones(n, dtype=torch.float64))
    assert torch.allclose(out[0], cell(gi, h).detach(), rtol=1e-13, atol=1e-13)
    assert torch.equal(out[1], h)
    none = R.gru_fwd(gi, gh0.detach(), cell.bias_hh.detach(), None, torch.zeros(n, dtype=torch.float64))
    assert torch.allclose(none[0], cell(gi, torch.zeros_like(h)).detach(), rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize('n,hd', [(1, 1), (7, 37), (5, 128)])
def test_gru_backward_reference_is_autograd_through_the_cell(n, hd):
    """With gi the cell's input: dgi is the input gradient, dgh gives the gradients of b_hh (its column sums) and W_hh
    (dgh^T h), and the state gradient is dhz + dgh W_hh, as include/mfg_learn.h says. The formulas on the saved
    activations give the same three."""
    cell, gi, h, dh = _cell(hd, n, 2)
    gi_, h_ = gi.clone().requires_grad_(), h.clone().requires_grad_()
    dx, dh_in, dw, db = torch.autograd.grad(cell(gi_, h_), [gi_, h_, cell.weight_hh, cell.bias_hh], dh)
    gh = (h @ cell.weight_hh.t() + cell.bias_hh).detach()
    dgi, dgh, dhz = R.gru_bwd(gi, gh, h, dh)
    tol = dict(rtol=1e-12, atol=1e-12)
    assert torch.allclose(dgi, dx, **tol) and torch.allclose(dgh.sum(0), db, **tol)
    assert torch.allclose(dgh.t() @ h, dw, **tol)
    assert torch.allclose(dhz + dgh @ cell.weight_hh.detach(), dh_in, **tol)
    _, hp, r, z, nn, ghn = R.gru_fwd(gi, gh, torch.zeros(3 * hd, dtype=torch.float64), h,
                                     torch.ones(n, dtype=torch.float64))
    for a, b in zip(R.gru_bwd_formulas(dh, r, z, nn, ghn, hp), (dgi, dgh, dhz)):
        assert torch.allclose(a, b, **tol)


@pytest.mark.parametrize('n_act', [1, 2, 7, 32])
def test_cdf_sampler_leaves_out_under_one_percent(n_act):
    """On the GPU test's inputs: at most 1% of the rows lie within 1e-5 of a CDF step, and on all the others the f32
    tensor twin of the kernel (evaluate.sample_inversion) picks the f64 CDF's action; the pad columns play no part."""
    logits, u = R.sampler_inputs(20000, n_act)
    assert bool((logits[:, n_act:] == 1000.0).all()) and float(u.min()) == 0.0 and float(u.max()) == R.U_LAST
    pick, near = R.cdf_pick(logits[:, :n_act], u)
    share = float(near.double().mean())
    print(f'n_act={n_act}: left out {100 * share:.3f}% of the rows')
    assert share <= 0.01
    twin = EV.sample_inversion(logits, u, n_act).long()
    assert torch.equal(twin[~near], pick[~near])
    assert int(pick.min()) >= 0 and int(pick.max()) <= n_act - 1


def test_cdf_sampler_never_picks_a_zero_probability_edge():
    """A first action 120 below the rest has a bin of width e^-120 in f64, which holds u = 0: such a row is marked near
    (f32 has no such bin); with -inf the bin is empty in f64 too."""
    lg = torch.zeros((2, 4))
    lg[0, 0], lg[1, 3] = -120.0, -120.0
    pick, near = R.cdf_pick(lg, torch.tensor([0.0, R.U_LAST]))
    assert pick.tolist() == [0, 2] and near.tolist() == [True, True]
    assert EV.sample_inversion(lg, torch.tensor([0.0, R.U_LAST])).tolist() == [1, 2]
    lg[0, 0], lg[1, 3] = float('-inf'), float('-inf')
    assert R.cdf_pick(lg, torch.tensor([0.0, R.U_LAST]))[0].tolist() == [1, 2]
    assert EV.sample_inversion(lg, torch.tensor([0.0, R.U_LAST])).tolist() == [1, 2]


@pytest.mark.parametrize('bad', [float('-inf'), float('inf'), float('nan')])
def test_tensor_heads_give_nan_for_a_non_finite_logit(bad):
    """The tensor-code twins of the fused heads: a non-finite logit anywhere in an element makes every loss the
    element enters NaN (a -inf logit away from the action would otherwise pass as probability 0), as the fused heads
    do (include/mfg_learn.h); finite inputs stay finite."""
    g = torch.Generator().manual_seed(3)
    A, B, T, n = 3, 4, 5, 6
    acts = torch.randint(0, n - 1, (A, B, T), generator=g)  # column n - 1 is never the action
    rew, done = torch.randn((A, B, T), generator=g), torch.zeros((A, B, T))
    hyp = (0.99, 0.01, 0.5)
    # MAPPO: logits and old logits
    lg, cr = torch.randn((A * B, T, n), generator=g), torch.randn((A * B, T), generator=g)
    args = (acts.view(A * B, T), rew.view(A * B, T), done.view(A * B, T), 0.99, 0.01, 0.5, 0.2)
    assert bool(torch.isfinite(M.mappo_loss_terms(lg, cr, lg.clone(), *args)))
    spoiled = lg.clone()
    spoiled[2, 1, n - 1] = bad
    assert bool(torch.isnan(M.mappo_loss_terms(spoiled, cr, lg, *args)))
    assert bool(torch.isnan(M.mappo_loss_terms(lg, cr, spoiled, *args)))
    # IAC: only the element's own network
    lg, cr = torch.randn((A, B, T, n), generator=g), torch.randn((A, B, T + 1), generator=g)
    assert bool(torch.isfinite(M.iac_loss_terms(lg, cr, acts, rew, done, *hyp)).all())
    spoiled = lg.clone()
    spoiled[1, 2, 1, n - 1] = bad
    assert torch.isnan(M.iac_loss_terms(spoiled, cr, acts, rew, done, *hyp)).tolist() == [False, True, False]
    counts = [n, n - 1, n]  # per-agent counts: the spoiled column is outside agent 1's head
    assert bool(torch.isfinite(M.iac_loss_terms(spoiled, cr, acts.clamp(max=n - 2), rew, done, *hyp,
                                                n_act=counts)).all())
    # SEAC: network 2 on a row of agent 0 spoils loss 2; the row's own network spoils every loss (through iw)
    lg, cr = torch.randn((A, A, B, T, n), generator=g), torch.randn((A, A, B, T + 1), generator=g)
    assert bool(torch.isfinite(M.seac_loss_terms(lg, cr, acts, rew, done, *hyp)).all())
    spoiled = lg.clone()
    spoiled[2, 0, 2, 1, n - 1] = bad
    assert torch.isnan(M.seac_loss_terms(spoiled, cr, acts, rew, done, *hyp)).tolist() == [False, False, True]
    spoiled = lg.clone()
    spoiled[0, 0, 2, 1, n - 1] = bad
    assert bool(torch.isnan(M.seac_loss_terms(spoiled, cr, acts, rew, done, *hyp)).all())
