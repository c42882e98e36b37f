"""The MAPPO learner on the GPU: the two HIP calls of the PPO loss head (include/mfg_learn.h: mfg_mc_returns,
mfg_ppo_head; csrc/mfg_ppo.hip) against torch in f64, the learner against the reference's fixture
(tests/golden/marl_mappo.npz) on the device, and BatchedMAPPO on the engine.

Tolerance of the head: the test measures it. mappo_loss_terms in f32 (torch, on the device) and the kernel are both
compared with mappo_loss_terms in f64 under autograd on the same inputs; the kernel's maximum error may be at most 4
times the f32 tensor code's (it sums in another order and uses another exp), plus 1e-7 absolute on the gradients.
"""
from pathlib import Path

import numpy as np
import pytest
import torch

import mfg_amd.marl as M
from mfg_amd import learn_lib
from test_mappo import check_loss_and_grads, hyper, load_case, pack

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / 'golden' / 'marl_mappo.npz'
HYP = dict(gamma=0.99, entropy_coef=0.01, vf_coef=0.5, clip_range=0.2)
EPS = 2.0 ** -24  # half an ulp of 1 in f32


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ws():
    return torch.empty(M._PPO_WS_BYTES // 8, dtype=torch.float64, device='cuda')


def _mc(reward, done, gamma, pad=3):
    """mfg_mc_returns on reward / done [n, t] held with a padded row stride; (rc, ret [n, t], stats [2], pad cols)."""
    n, t = reward.shape
    r = torch.full((n, t + pad), 7.0, device='cuda')
    d = torch.full((n, t + pad), 7.0, device='cuda')
    r[:, :t], d[:, :t] = reward, done
    ret = torch.full((n, t + pad), -5.0, device='cuda')
    stats = torch.zeros(2, dtype=torch.float64, device='cuda')
    ws = _ws()
    rc = learn_lib.lib().mfg_mc_returns(r.data_ptr(), t + pad, d.data_ptr(), t + pad, n, t, gamma, ret.data_ptr(),
                                        t + pad, stats.data_ptr(), ws.data_ptr(), _stream())
    torch.cuda.synchronize()
    return rc, ret[:, :t].clone(), stats, ret[:, t:]


@pytest.mark.parametrize('n,t', [(2, 1), (3, 5), (257, 5), (1000, 7)])
@pytest.mark.parametrize('dones', ['mixed', 'all', 'none'])
def test_mc_returns_kernel(n, t, dones):
    """ret element by element and (mean, unbiased std) against the torch loop in f64. Bounds: the f32 scan rounds once
    per product and sum, so |ret - ref| <= 3 (t + 1) 2^-24 Rabs with Rabs the return of |reward|; mean and std move by
    at most sqrt(2) times the largest element error; against the kernel's own returns the f64 statistics agree to
    f64 rounding (1e-12 relative to the values' scale)."""
    g = torch.Generator().manual_seed(n * 10 + t)
    reward = (torch.randn((n, t), generator=g) * 0.5 + 0.3).cuda()
    done = torch.zeros((n, t))
    if dones == 'all':
        done[:] = 1
    elif dones == 'mixed':
        done = (torch.rand((n, t), generator=g) < 0.2).float()
        done[0, 0] = 1  # the first step of a row
        done[-1, -1] = 1  # and the last
    done = done.cuda()
    gamma = 0.99
    rc, ret, stats, padcols = _mc(reward, done, gamma)
    assert rc == 0
    assert bool((padcols == -5.0).all())
    ref = M.monte_carlo_returns(reward.double(), done.double(), gamma)
    rabs = M.monte_carlo_returns(reward.double().abs(), done.double(), gamma)
    err = (ret.double() - ref).abs()
    assert bool((err <= 3 * (t + 1) * EPS * rabs + 1e-30).all()), float(err.max())
    own = ret.double()
    scale = float(own.abs().max()) + 1e-30
    assert abs(float(stats[0]) - float(own.mean())) <= 1e-12 * scale
    assert abs(float(stats[1]) - float(own.std())) <= 1e-12 * scale
    tol = 2 ** 0.5 * 3 * (t + 1) * EPS * float(rabs.max()) + 1e-12 * scale
    assert abs(float(stats[0]) - float(ref.mean())) <= tol
    assert abs(float(stats[1]) - float(ref.std())) <= tol
    rc2, ret2, stats2, _ = _mc(reward, done, gamma)
    assert rc2 == 0 and torch.equal(ret, ret2) and torch.equal(stats, stats2)  # bit-identical


def test_mc_returns_refuses_a_single_element():
    one = torch.ones((1, 1), device='cuda')
    rc, _, _, _ = _mc(one, one, 0.99)
    assert rc == -1


# ---------------------------------------------------------------------------------------------------------------------
def head_inputs(n, t, n_act, seed=0):
    """Inputs over three thirds of the n t elements: (i) old_logits == logits bit for bit; (ii) the old logit of the
    taken action moved by -+1.5 and the critic placed 0.7 above / below the normalised return, cycling through the four
    combinations (ratio above / below the clip range) x (advantage sign); (iii) one logit 120 below the rest, so its
    p log p underflows to 0 in f32. n_act = 1 has one distribution only (ratio == 1, no clipped element)."""
    g = torch.Generator().manual_seed(seed + 1000 * n_act + n)
    m = n * t
    logits = torch.randn((m, n_act), generator=g) * 1.5
    act = torch.randint(0, n_act, (m,), generator=g)
    reward = torch.randn((n, t), generator=g) * 0.5
    done = (torch.rand((n, t), generator=g) < 0.15).float()
    ret = M.monte_carlo_returns(reward.double(), done.double(), HYP['gamma']).reshape(m)
    rhat = (ret - ret.mean()) / (ret.std() + 1e-8)
    critic = (rhat + torch.randn(m, generator=g).double() * 0.5).float()
    old = logits.clone()
    k = torch.arange(m)
    zone = (k * 3) // m  # 0, 1, 2
    z1 = zone == 1
    j = k - int(z1.nonzero()[0])
    if n_act > 1:
        old[z1, act[z1]] += torch.where(j[z1] % 2 == 0, 1.5, -1.5)  # old logp up: ratio < 1 - c; down: ratio > 1 + c
        critic[z1] = (rhat[z1] + torch.where((j[z1] // 2) % 2 == 0, 0.7, -0.7)).float()
        z2 = zone == 2
        low = (act + 1) % n_act  # not the taken action
        logits[z2, low[z2]] = logits[z2].max(-1).values - 120.0
        old[z2] = logits[z2]
        old[z2] += torch.randn((int(z2.sum()), n_act), generator=g) * 0.05
    return dict(logits=logits, old=old, critic=critic, act=act, reward=reward, done=done, n=n, t=t, zone=zone)


def torch_head(x, dtype, device):
    """(loss, dlogits, dcritic) of mappo_loss_terms under autograd in dtype."""
    n, t = x['n'], x['t']
    lg = x['logits'].to(device, dtype).view(n, t, -1).requires_grad_()
    cr = x['critic'].to(device, dtype).view(n, t).requires_grad_()
    loss = M.mappo_loss_terms(lg, cr, x['old'].to(device, dtype).view(n, t, -1), x['act'].to(device).view(n, t),
                              x['reward'].to(device, dtype), x['done'].to(device, dtype), **HYP)
    dl, dc = torch.autograd.grad(loss, [lg, cr])
    return loss.detach().double().cpu(), dl.double().cpu().view(n * t, -1), dc.double().cpu().view(n * t)


def kernel_head(x, pad=3, act=None, logits=None):
    """mfg_mc_returns + mfg_ppo_head on padded logit rows: (rc, loss, dlogits, dcritic, dlogits' pad columns)."""
    n, t = x['n'], x['t']
    m, n_act = x['logits'].shape
    L = learn_lib.lib()

    def padded(v, fill):
        o = torch.full((m, n_act + pad), fill, device='cuda')
        o[:, :n_act] = v
        return o
    lg = padded(x['logits'] if logits is None else logits, 9.0)
    old = torch.full((m, n_act + pad + 2), 9.0, device='cuda')  # its own stride
    old[:, :n_act] = x['old']
    cr = x['critic'].cuda()
    a = (x['act'] if act is None else act).to(torch.int32).cuda()
    rew, dn = x['reward'].cuda().contiguous(), x['done'].cuda().contiguous()
    ret = torch.empty((n, t), device='cuda')
    stats = torch.zeros(2, dtype=torch.float64, device='cuda')
    ws = _ws()
    assert L.mfg_mc_returns(rew.data_ptr(), t, dn.data_ptr(), t, n, t, HYP['gamma'], ret.data_ptr(), t,
                            stats.data_ptr(), ws.data_ptr(), _stream()) == 0
    loss = torch.zeros((), device='cuda')
    dl = padded(torch.zeros((m, n_act)), -3.0)
    dc = torch.full((m + 8,), -3.0, device='cuda')
    rc = L.mfg_ppo_head(lg.data_ptr(), n_act + pad, old.data_ptr(), n_act + pad + 2, cr.data_ptr(), a.data_ptr(),
                        ret.data_ptr(), stats.data_ptr(), m, n_act, HYP['clip_range'], HYP['vf_coef'],
                        HYP['entropy_coef'], loss.data_ptr(), dl.data_ptr(), n_act + pad, dc.data_ptr(), ws.data_ptr(),
                        _stream())
    torch.cuda.synchronize()
    assert bool((dl[:, n_act:] == -3.0).all()) and bool((dc[m:] == -3.0).all()), 'a write outside the rows'
    return rc, loss.double().cpu(), dl[:, :n_act].double().cpu(), dc[:m].double().cpu()


def head_errors(x):
    """Maximum errors against f64 of (the kernel, the f32 tensor code) for loss, dlogits, dcritic."""
    ref = torch_head(x, torch.float64, 'cpu')
    f32 = torch_head(x, torch.float32, 'cuda')
    rc, *ker = kernel_head(x)
    assert rc == 0
    e_ker = [float((a - b).abs().max()) for a, b in zip(ker, ref)]
    e_f32 = [float((a - b).abs().max()) for a, b in zip(f32, ref)]
    return e_ker, e_f32, ref, ker


@pytest.mark.parametrize('n,t', [(3, 5), (257, 5)])
@pytest.mark.parametrize('n_act', [1, 10, 64])
def test_ppo_head_kernel(n, t, n_act):
    x = head_inputs(n, t, n_act)
    m = n * t
    if n_act > 1:  # the inputs cover what they claim, by the f64 quantities
        lg, old, a = x['logits'].double(), x['old'].double(), x['act'][:, None]
        assert torch.equal(x['old'][x['zone'] == 0], x['logits'][x['zone'] == 0])
        ratio = (torch.log_softmax(lg, -1).gather(1, a) - torch.log_softmax(old, -1).gather(1, a)).squeeze(1).exp()
        ret = M.monte_carlo_returns(x['reward'].double(), x['done'].double(), HYP['gamma']).reshape(m)
        adv = (ret - ret.mean()) / (ret.std() + 1e-8) - x['critic'].double()
        c = HYP['clip_range']
        for side in (ratio > 1 + c, ratio < 1 - c):
            for sign in (adv > 0, adv < 0):
                assert bool((side & sign).any()), 'a clip side / advantage sign combination is missing'
        p = torch.softmax(x['logits'], -1)  # f32: the far-below logit's probability is 0
        assert bool((p[x['zone'] == 2].min(-1).values == 0).all())
    e_ker, e_f32, ref, ker = head_errors(x)
    print(f'ppo_head m={m} n_act={n_act}: kernel err (loss, dlogits, dcritic) = {e_ker}, f32 torch err = {e_f32}, '
          f'ratio = {[a / b if b else float("inf") if a else 0.0 for a, b in zip(e_ker, e_f32)]}')
    assert e_ker[0] <= 4 * e_f32[0], (e_ker[0], e_f32[0])
    assert e_ker[1] <= 4 * e_f32[1] + 1e-7, (e_ker[1], e_f32[1])
    assert e_ker[2] <= 4 * e_f32[2] + 1e-7, (e_ker[2], e_f32[2])
    rc, *again = kernel_head(x)
    assert rc == 0 and all(torch.equal(a, b) for a, b in zip(ker, again))  # bit-identical


def test_ppo_head_bad_inputs_give_nan_not_a_fault():
    """An action equal to n_act and a NaN logit: the kernel checks before it indexes, the loss is NaN, the bad
    element's gradients are 0 and the other elements keep finite gradients."""
    x = head_inputs(3, 5, 10)
    act = x['act'].clone()
    act[4] = 10
    rc, loss, dl, dc = kernel_head(x, act=act)
    assert rc == 0 and bool(torch.isnan(loss))
    assert bool((dl[4] == 0).all()) and float(dc[4]) == 0 and bool(torch.isfinite(dl).all())
    act[4] = -1
    rc, loss, dl, dc = kernel_head(x, act=act)
    assert rc == 0 and bool(torch.isnan(loss)) and bool(torch.isfinite(dl).all())
    logits = x['logits'].clone()
    logits[7, 3] = float('nan')
    rc, loss, dl, dc = kernel_head(x, logits=logits)
    assert rc == 0 and bool(torch.isnan(loss))
    assert bool((dl[7] == 0).all()) and bool(torch.isfinite(dl).all()) and bool(torch.isfinite(dc).all())
    rc, loss, dl, dc = kernel_head(x)
    assert rc == 0 and bool(torch.isfinite(loss))


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', [0, 1, 2])
@pytest.mark.parametrize('fused', [True, False])
def test_mappo_learner_matches_reference_on_device(i, fused):
    """The reference's fixture through project_packed + forward_emb + the loss head on the device (the fused HIP head
    and the tensor code), with the CPU replay's tolerances: the GPU learner is pinned to the reference."""
    z = np.load(GOLD)
    c, net = load_case(z, i, 'cuda')
    idx, val = pack(c['obs'], cap=64)
    dev = lambda k: torch.from_numpy(c[k]).cuda()  # noqa: E731
    acts = dev('actions').long()
    out = net.forward_emb(net.project_packed(idx.cuda(), val.cuda()), acts, dev('ha0'), dev('hc0'))
    args = (out['logits'][:, :-1], out['critic'][:, :-1], dev('old_logits'), acts[:, 1:], dev('reward'), dev('done'))
    h = hyper(c)
    if fused:
        loss = M._PPOHead.apply(*args, h['gamma'], h['entropy_coef'], h['vf_coef'], h['clip_range'])
    else:
        loss = M.mappo_loss_terms(*args, **h)
    check_loss_and_grads(c, net, loss)


def _trainer(fused_head=True, seed=0):
    from mfg_amd.factory import BatchedFactory
    f = BatchedFactory('rooms4.yaml', 32, seed_base=3)
    torch.manual_seed(seed)
    tr = M.BatchedMAPPO(f, n_steps=5, buffer_size=16, batch_size=64, n_updates=2, cap=64, fused_head=fused_head,
                        generator=torch.Generator(device='cuda').manual_seed(seed), **HYP)
    return f, tr


def _check_chunks(tr, mb):
    """No sampled chunk holds the write head or crosses an episode end, and its entries are consecutive in time."""
    slots = mb['slots']
    assert not bool((slots == tr.head).any())
    age = (tr.head - slots) % tr.R  # steps back from the write head
    assert bool((age[:, :-1] - age[:, 1:] == 1).all()) and int(age.max()) <= tr.S and int(age.min()) >= 1
    assert not bool(mb['done'][:, :-1].any())
    assert torch.equal(mb['done'], tr.done[slots, mb['rows'][:, None] // tr.A].float())


def test_batched_mappo_on_rooms4():
    f, tr = _trainer()
    w0 = {k: p.detach().clone() for k, p in tr.net.named_parameters()}
    tr.train(16)
    assert tr.filled == tr.S and tr.updates == 0  # full; the learn calls at steps 5, 10, 15 found it not full
    # alignment of observation slots, action inputs and stored states in the ring: before any weight change the chunk
    # forward from a chunk's stored states reproduces the acting logits, so ratio == 1 and the policy term is -mean(adv)
    mb = tr.minibatch(*tr.sample())
    _check_chunks(tr, mb)
    with torch.no_grad():
        out = tr.evaluate(mb)
    assert torch.allclose(out['logits'], mb['old_logits'], rtol=1e-4, atol=1e-5), \
        float((out['logits'] - mb['old_logits']).abs().max())
    ret = M.monte_carlo_returns(mb['reward'], mb['done'], tr.gamma)
    adv = (ret - ret.mean()) / (ret.std() + 1e-8) - out['critic']
    want = -float(adv.double().mean())
    tol = 1e-4 * float(adv.double().abs().mean()) + 1e-6  # |ratio - 1| <= ~1e-4 from the logits' tolerance
    args = (out['logits'], out['critic'], mb['old_logits'], mb['act'], mb['reward'], mb['done'], tr.gamma)
    assert abs(float(M.mappo_loss_terms(*args, 0.0, 0.0, tr.clip_range)) - want) <= tol
    assert abs(float(M._PPOHead.apply(*args, 0.0, 0.0, tr.clip_range)) - want) <= tol
    tr.train(9)  # learn calls at steps 20 and 25
    assert tr.updates == 4 and tr.skipped_updates == 0 and bool(torch.isfinite(tr.last_loss))
    for k, p in tr.net.named_parameters():
        if k != 'agent_emb.weight':  # not part of the network without use_agent_embedding: no gradient
            assert not torch.equal(w0[k], p.detach()), k
    e = tr.net.project_packed(tr.pobs.idx[tr.head], tr.pobs.val[tr.head])
    assert torch.allclose(e, tr.pobs.emb[tr.head], rtol=1e-5, atol=1e-5)  # re-projected with the new weights
    # on to the first episode ends (max_steps 500): the ring has wrapped many times, the buffer holds done flags
    tr.train(503 - tr.steps)
    assert float(tr.episodes) > 0 and bool(tr.done[tr.order()].any())
    for _ in range(3):
        _check_chunks(tr, tr.minibatch(*tr.sample()))
    assert bool(torch.isfinite(tr.last_loss))
    f.close()


def test_fused_head_matches_tensor_head_on_a_minibatch():
    """fused_head True / False on one fixed minibatch. Head outputs: each is within its own error of the f64 head, so
    they differ by at most (4 + 1) times the f32 tensor code's measured error against f64 (+1e-7 on gradients, the
    kernel test's bound). Parameter gradients are the same backward of two such (dlogits, dcritic): the learner
    tests' rtol 1e-4 / atol 1e-6, relative to each tensor's largest gradient."""
    f, tr = _trainer()
    tr.train(16)
    mb = tr.minibatch(*tr.sample())
    res = {}
    for fused in (True, False):
        tr.fused_head = fused
        tr.net.zero_grad()
        with torch.enable_grad():
            out = tr.evaluate(mb)
            out['logits'].retain_grad()
            out['critic'].retain_grad()
            loss = tr.loss(mb, out)
        loss.backward()
        res[fused] = (loss.detach().double().cpu(), out['logits'].grad.double().cpu(), out['critic'].grad.double().cpu(),
                      {k: p.grad.clone() for k, p in tr.net.named_parameters() if p.grad is not None}, out)
    out = res[False][4]
    n, t = mb['act'].shape
    x = dict(logits=out['logits'].detach().cpu().reshape(n * t, -1), critic=out['critic'].detach().cpu().reshape(n * t),
             old=mb['old_logits'].cpu().reshape(n * t, -1), act=mb['act'].cpu().reshape(n * t),
             reward=mb['reward'].cpu(), done=mb['done'].cpu(), n=n, t=t)
    ref = torch_head(x, torch.float64, 'cpu')
    e = [float((a - b.reshape(a.shape)).abs().max()) for a, b in zip(res[False][:3], ref)]
    d = [float((a - b).abs().max()) for a, b in zip(res[True][:3], res[False][:3])]
    print(f'fused vs tensor head on a minibatch: difference (loss, dlogits, dcritic) = {d}, f32 torch err = {e}')
    assert d[0] <= 5 * e[0] and d[1] <= 5 * e[1] + 1e-7 and d[2] <= 5 * e[2] + 1e-7, (d, e)
    assert res[True][3].keys() == res[False][3].keys()
    for k, g in res[False][3].items():
        a = res[True][3][k]
        assert float((a - g).abs().max()) <= 1e-4 * float(g.abs().max()) + 1e-6, (k, float((a - g).abs().max()))
    f.close()
