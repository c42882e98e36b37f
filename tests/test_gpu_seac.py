"""The per-agent-network learners on the GPU: the HIP calls of csrc/mfg_seac.hip (include/mfg_learn.h:
mfg_packed_project_grouped, mfg_gru_fwd_step_grouped, mfg_seac_head) against torch in f64 or the existing kernels, the
learners against the reference's fixture (tests/golden/marl_seac.npz) on the device, and BatchedIAC / BatchedSEAC on
the engine.

Tolerance of the loss head: the test measures it, as tests/test_gpu_mappo.py does. iac_loss_terms / seac_loss_terms in
f32 (torch, on the device) and the kernel are both compared with the same terms in f64 under autograd; the kernel's
largest error may be at most 4 times the f32 tensor code's, plus 1e-7 absolute on the gradients and one f32 ulp of
|loss| on a loss. With MFG_SEAC_FIGURES set to a file name the measured figures are written there as JSON
(tools/bench_seac.py folds them into profiles/seac.json).
"""
import json
import os
from pathlib import Path

import numpy as np
import pytest
import torch

import mfg_amd.marl as M
import mfg_amd.seac as S
from mfg_amd import learn_lib
from test_seac import check_loss_and_grads, forward, hyper, load_case, targets

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / 'golden' / 'marl_seac.npz'
EPS = 2.0 ** -24  # half an ulp of 1 in f32
HYP = (0.99, 0.01, 0.5)  # gamma, entropy_coef, vf_coef
FIGURES = {}


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _record(key, fig):
    FIGURES[key] = fig
    dst = os.environ.get('MFG_SEAC_FIGURES')
    if dst:
        Path(dst).write_text(json.dumps(FIGURES, indent=1))


# ---------------------------------------------------------------------------------------------------------------------
# grouped projection
# ---------------------------------------------------------------------------------------------------------------------
def _packed_rows(m, cap, k, g):
    """m packed rows with distinct indices per row (base + stride j mod k, the stride coprime to k): row 0 empty, row 1
    (if any) full, the others with a random count; a zero value sits in the middle of every row that has three or more
    entries, followed by nonzero ones."""
    full = min(cap, k)
    cnt = torch.randint(0, full + 1, (m,), generator=g)
    cnt[0] = 0
    if m > 1:
        cnt[1] = full
    j = torch.arange(cap)
    stride = torch.randint(0, max(1, (k - 1) // 2), (m, 1), generator=g) * 2 + 1  # odd: coprime to 4096; < 37 (prime)
    idx = (torch.randint(0, k, (m, 1), generator=g) + stride * j) % k
    live = j[None] < cnt[:, None]
    val = torch.randn((m, cap), generator=g)
    val = torch.where(val.abs() < 0.05, torch.ones_like(val), val) * live
    rows = (cnt >= 3).nonzero().flatten()
    val[rows, cnt[rows] // 2] = 0.0
    return idx * live, val


@pytest.mark.parametrize('G', [1, 3, 8])
@pytest.mark.parametrize('mb', [1, 7, 257])
def test_grouped_projection(G, mb):
    """Both modes against a dense f64 matmul. Bound: a term v w passes one product rounding and at most cap sum
    roundings (the bias add included), so |out - ref| <= ((1 + u)^(cap + 1) - 1) S <= (cap + 2) u S with u = 2^-24 and
    S = |bias| + sum |v| |w| of the row."""
    g = torch.Generator().manual_seed(100 * G + mb)
    L = learn_lib.lib()
    m = G * mb
    pad = 3
    for cap in (1, 32, 70):
        for E in (1, 96, 128):
            for k in (4096, 37):
                idx, val = _packed_rows(m, cap, k, g)
                if cap == 70 and m > 1 and k >= cap:  # zeros fill the whole first 64-entry chunk, nonzero entries follow
                    val[1, :64] = 0.0
                    assert bool((val[1, 64:] != 0).all())
                wt = torch.randn((G, k, E), generator=g)
                bias = torch.randn((G, E), generator=g)
                d = torch.zeros((m, k), dtype=torch.float64).scatter_add_(1, idx, val.double()).cuda()
                w64, b64 = wt.double().cuda(), bias.double().cuda()
                ref_all = (torch.einsum('rk,gke->gre', d, w64) + b64[:, None]).cpu()  # [G, m, E]
                mag_all = (torch.einsum('rk,gke->gre', d.abs(), w64.abs()) + b64.abs()[:, None]).cpu()
                ci, cv = idx.to(torch.uint16).cuda(), val.cuda()
                cw, cb = wt.cuda(), bias.cuda()
                for all_ in (0, 1):
                    rows = G * m if all_ else m
                    out = torch.full((rows, E + pad), -7.0, device='cuda')
                    rc = L.mfg_packed_project_grouped(ci.data_ptr(), cv.data_ptr(), m, cap, G, cw.data_ptr(),
                                                      cb.data_ptr(), E, k, all_, out.data_ptr(), E + pad, _stream())
                    torch.cuda.synchronize()
                    assert rc == 0
                    assert bool((out[:, E:] == -7.0).all()), 'guard columns written'
                    got = out[:, :E].double().cpu()
                    r = torch.arange(m)
                    if all_:  # out[n][r % G][r / G]
                        got = got.view(G, G, mb, E)[:, r % G, r // G]  # [G, m, E]
                        ref, mag = ref_all, mag_all
                    else:  # out[r % G][r / G] by network r % G
                        got = got.view(G, mb, E)[r % G, r // G]
                        ref, mag = ref_all[r % G, r], mag_all[r % G, r]
                    err = (got - ref).abs()
                    assert bool((err <= (cap + 2) * EPS * mag + 1e-30).all()), (cap, E, k, all_, float(err.max()))
                    # a row with no entries is the bias
                    own = got[:, 0] if all_ else got[0][None]
                    assert torch.equal(own, bias.double()[:own.shape[0]] if all_ else bias.double()[:1])


def test_grouped_projection_refuses_bad_sizes():
    L = learn_lib.lib()
    z = torch.zeros(1 << 16, device='cuda')
    out = torch.zeros(1 << 10, device='cuda')
    p, o = z.data_ptr(), out.data_ptr()
    call = lambda m, cap, G, E, k: L.mfg_packed_project_grouped(p, p, m, cap, G, p, p, E, k, 0, o, E, _stream())  # noqa
    assert call(7, 4, 3, 8, 16) == -1  # m % G
    assert call(6, 4, 3, 8, 4097) == -1  # k
    assert call(6, 4, 3, 129, 16) == -1  # E
    assert call(6, 4, 3, 8, 16) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# grouped-bias GRU step
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rpg', [5, 64])
@pytest.mark.parametrize('hd', [16, 64])
def test_grouped_gru_step_is_the_per_block_step(rpg, hd):
    """mfg_gru_fwd_step_grouped over G blocks of rows, bit-equal to mfg_gru_fwd_step called per block with that block's
    bias. (mfg_gru_bwd_step reads no bias: the grouped learner calls it over all rows unchanged.)"""
    G = 3
    n = G * rpg
    g = torch.Generator().manual_seed(rpg + hd)
    gi, gh0 = torch.randn((n, 3 * hd), generator=g).cuda(), torch.randn((n, 3 * hd), generator=g).cuda()
    bh = torch.randn((G, 3 * hd), generator=g).cuda()
    h = torch.randn((n, hd), generator=g).cuda()
    keep = (torch.rand(n, generator=g) < 0.7).float().cuda()
    L = learn_lib.lib()

    def outs():
        return [torch.full((n, hd), -3.0, device='cuda') for _ in range(6)]
    a, b = outs(), outs()
    rc = L.mfg_gru_fwd_step_grouped(gi.data_ptr(), 3 * hd, gh0.data_ptr(), bh.data_ptr(), rpg, h.data_ptr(), hd,
                                    keep.data_ptr(), 1, a[0].data_ptr(), hd, *[x.data_ptr() for x in a[1:]], hd, n, hd,
                                    _stream())
    assert rc == 0
    for q in range(G):
        r0 = q * rpg
        rc = L.mfg_gru_fwd_step(gi[r0].data_ptr(), 3 * hd, gh0[r0].data_ptr(), bh[q].data_ptr(), h[r0].data_ptr(), hd,
                                keep[r0:].data_ptr(), 1, b[0][r0].data_ptr(), hd, *[x[r0].data_ptr() for x in b[1:]],
                                hd, rpg, hd, _stream())
        assert rc == 0
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y) and bool((x != -3.0).any())
    assert L.mfg_gru_fwd_step_grouped(gi.data_ptr(), 3 * hd, gh0.data_ptr(), bh.data_ptr(), rpg + 1, h.data_ptr(), hd,
                                      keep.data_ptr(), 1, a[0].data_ptr(), hd, *[x.data_ptr() for x in a[1:]], hd, n,
                                      hd, _stream()) == -1


# ---------------------------------------------------------------------------------------------------------------------
# the loss head
# ---------------------------------------------------------------------------------------------------------------------
def head_inputs(A, B, t, n_act, cross, dones='mixed', seed=0):
    """logits [nets, A B, t+1, n_max] (nets = A for cross, else 1) with a std of 1.5 per network (so the importance
    weights spread), in a third of the elements one logit of the row's head 120 below the rest; critic near the
    rewards' scale; engine-layout targets action i32 / reward f32 [t, B, A] and done f32 [t, B]."""
    n_act = [int(n_act)] * A if np.ndim(n_act) == 0 else list(n_act)
    n_max = max(n_act)
    g = torch.Generator().manual_seed(seed + 17 * A + B + 1000 * t + n_max)
    nets = A if cross else 1
    n = A * B
    logits = torch.randn((nets, n, t + 1, n_max), generator=g) * 1.5
    act = torch.stack([torch.randint(0, n_act[a], (t, B), generator=g) for a in range(A)], 2).to(torch.int32)
    if n_max > 1:
        for j in range(nets):
            for r in range(0, n, 3):
                na = n_act[j if cross else r // B]
                a = int(act[0, r % B, r // B])
                if na > 1:
                    logits[j, r, :, (a + 1) % na] = logits[j, r, :, :na].max(-1).values - 120.0
    critic = torch.randn((nets, n, t + 1), generator=g) * 0.5
    reward = torch.randn((t, B, A), generator=g) * 0.5
    done = torch.zeros((t, B))
    if dones == 'all':
        done[:] = 1
    elif dones == 'mixed':
        done = (torch.rand((t, B), generator=g) < 0.2).float()
        done[0, 0] = 1  # a first step
        done[-1, -1] = 1  # and a last one
    return dict(A=A, B=B, t=t, n_act=n_act, n_max=n_max, cross=cross, logits=logits, critic=critic, act=act,
                reward=reward, done=done)


def torch_head(x, dtype, device, gae):
    """(loss [A], dlogits, dcritic) of the torch terms under autograd in dtype, in the kernel's layouts."""
    A, B, t = x['A'], x['B'], x['t']
    lg = x['logits'].to(device, dtype).requires_grad_()
    cr = x['critic'].to(device, dtype).requires_grad_()
    acts = x['act'].to(device).long().permute(2, 1, 0)  # [A, B, t]
    rew = x['reward'].to(device, dtype).permute(2, 1, 0)
    dn = x['done'].to(device, dtype).t()[None].expand(A, B, t)
    if x['cross']:
        loss = M.seac_loss_terms(lg.view(A, A, B, t + 1, -1)[:, :, :, :t], cr.view(A, A, B, t + 1), acts, rew, dn,
                                 *HYP, gae)
    else:
        loss = M.iac_loss_terms(lg.view(A, B, t + 1, -1)[:, :, :t], cr.view(A, B, t + 1), acts, rew, dn, *HYP, gae,
                                n_act=x['n_act'])
    dl, dc = torch.autograd.grad(loss.sum(), [lg, cr])
    return loss.detach().double().cpu(), dl.double().cpu(), dc.double().cpu()


def kernel_head(x, gae, act=None, logits=None, guard=16):
    """mfg_seac_head with guard elements around every output: (rc, loss, dlogits, dcritic)."""
    A, B, t = x['A'], x['B'], x['t']
    lg = (x['logits'] if logits is None else logits).cuda().contiguous()
    cr = x['critic'].cuda().contiguous()
    a = (x['act'] if act is None else act).cuda().contiguous()
    rew, dn = x['reward'].cuda().contiguous(), x['done'].cuda().contiguous()
    n_act = torch.tensor(x['n_act'], dtype=torch.int32, device='cuda')

    def guarded(numel):
        return torch.full((numel + 2 * guard,), -3.0, device='cuda')
    loss, dl, dc = guarded(A), guarded(lg.numel()), guarded(cr.numel())
    ws = torch.empty(S.seac_ws_bytes(A) // 8, dtype=torch.float64, device='cuda')
    rc = learn_lib.lib().mfg_seac_head(lg.data_ptr(), cr.data_ptr(), A, B, t, x['n_max'], a.data_ptr(), B * A, A, 1,
                                       rew.data_ptr(), B * A, A, 1, dn.data_ptr(), B, 1, 0, n_act.data_ptr(), HYP[0],
                                       gae, HYP[2], HYP[1], 1 if x['cross'] else 0, loss[guard:].data_ptr(),
                                       dl[guard:].data_ptr(), dc[guard:].data_ptr(), ws.data_ptr(), _stream())
    torch.cuda.synchronize()
    for o in (loss, dl, dc):
        assert bool((o[:guard] == -3.0).all()) and bool((o[-guard:] == -3.0).all()), 'a write outside the outputs'
    return (rc, loss[guard:-guard].double().cpu(), dl[guard:-guard].double().cpu().view(lg.shape),
            dc[guard:-guard].double().cpu().view(cr.shape))


def _ulp(v):
    return 2.0 ** (np.floor(np.log2(max(abs(v), 1e-30))) - 23)


SHAPES = [(2, 1, 1, 2), (3, 50, 5, 10), (8, 33, 7, 64)]
HEAD_CASES = [(s, c, gae, 'mixed') for s in SHAPES for c in (0, 1) for gae in (0.0, 0.95)] + \
             [(SHAPES[1], c, 0.95, d) for c in (0, 1) for d in ('all', 'none')] + \
             [((4, 9, 5, (4, 10, 9, 14)), 0, gae, 'mixed') for gae in (0.0, 0.95)]


@pytest.mark.parametrize('shape,cross,gae,dones', HEAD_CASES)
def test_seac_head_kernel(shape, cross, gae, dones):
    A, B, t, n_act = shape
    x = head_inputs(A, B, t, n_act, cross, dones)
    if cross and A * B * t >= 100:  # the inputs cover what they claim, by the f64 quantities
        lp = torch.log_softmax(x['logits'].double()[:, :, :t], -1)
        a = x['act'].long().permute(2, 1, 0).reshape(1, A * B, t, 1).expand(A, -1, -1, -1)
        lp = lp.gather(-1, a).squeeze(-1).view(A, A, B, t)
        iw = (lp - lp[torch.arange(A), torch.arange(A)][None]).exp()
        off = ~torch.eye(A, dtype=torch.bool)
        assert float(iw[off].min()) < 0.5 and float(iw[off].max()) > 2.0
        assert bool((torch.softmax(x['logits'], -1).min(-1).values == 0).any())  # the far-below logit: p == 0 in f32
    ref = torch_head(x, torch.float64, 'cpu', gae)
    f32 = torch_head(x, torch.float32, 'cuda', gae)
    rc, *ker = kernel_head(x, gae)
    assert rc == 0
    e_ker = [float((a - b).abs().max()) for a, b in zip(ker, ref)]
    e_f32 = [float((a - b).abs().max()) for a, b in zip(f32, ref)]
    ratio = [a / b if b else (float('inf') if a else 0.0) for a, b in zip(e_ker, e_f32)]
    key = f'A{A}_B{B}_t{t}_n{x["n_max"]}{"h" if len(set(x["n_act"])) > 1 else ""}_cross{cross}_gae{gae}_{dones}'
    print(f'seac_head {key}: kernel err (loss, dlogits, dcritic) = {e_ker}, f32 torch err = {e_f32}, ratio = {ratio}')
    _record(key, dict(kernel_err=e_ker, torch_f32_err=e_f32, ratio=ratio, elements=A * B * t * (A if cross else 1)))
    assert e_ker[0] <= 4 * e_f32[0] + _ulp(float(ref[0].abs().max())), (e_ker[0], e_f32[0])
    assert e_ker[1] <= 4 * e_f32[1] + 1e-7, (e_ker[1], e_f32[1])
    assert e_ker[2] <= 4 * e_f32[2] + 1e-7, (e_ker[2], e_f32[2])
    # entry t and the padded columns carry no gradient
    assert bool((ker[1][..., t, :] == 0).all()) and bool((ker[2][..., t] == 0).all())
    if not cross:
        for a, n in enumerate(x['n_act']):
            assert bool((ker[1][0, a * B:(a + 1) * B, :, n:] == 0).all())
    rc, *again = kernel_head(x, gae)
    assert rc == 0 and all(torch.equal(a, b) for a, b in zip(ker, again))  # bit-identical


def test_seac_head_bad_inputs_give_nan_not_a_fault():
    """An action outside the range and a NaN logit: checked before anything is indexed; NaN in exactly the losses the
    element enters, zero gradients for that element, finite everything else, guards untouched (kernel_head)."""
    A, B, t = 3, 4, 5
    for cross in (1, 0):
        x = head_inputs(A, B, t, 10, cross, 'none')
        row = 1 * B + 2  # agent 1, env 2
        for bad in (10, -1, 1 << 30):
            act = x['act'].clone()
            act[3, 2, 1] = bad
            rc, loss, dl, dc = kernel_head(x, 0.0, act=act)
            assert rc == 0
            nan = torch.isnan(loss)
            assert nan.tolist() == ([True] * A if cross else [False, True, False]), (cross, bad, loss)
            assert bool((dl[:, row, 3] == 0).all()) and bool((dc[:, row, 3] == 0).all())
            assert bool(torch.isfinite(dl).all()) and bool(torch.isfinite(dc).all())
        logits = x['logits'].clone()
        net = 2 if cross else 0
        logits[net, 2, 1, 4] = float('nan')  # network 2 (cross) on a row of agent 0; own: agent 0's row by its network
        rc, loss, dl, dc = kernel_head(x, 0.95, logits=logits)
        assert rc == 0
        assert torch.isnan(loss).tolist() == ([False, False, True] if cross else [True, False, False])
        assert bool((dl[net, 2, 1] == 0).all()) and bool(torch.isfinite(dl).all()) and bool(torch.isfinite(dc).all())
        if cross:  # a NaN in the row's own network spoils the importance weight of every network on that element
            logits = x['logits'].clone()
            logits[0, 2, 1, 4] = float('nan')
            rc, loss, dl, dc = kernel_head(x, 0.0, logits=logits)
            assert rc == 0 and bool(torch.isnan(loss).all())
            assert bool((dl[:, 2, 1] == 0).all()) and bool((dc[:, 2, 1] == 0).all())
        rc, loss, dl, dc = kernel_head(x, 0.95)
        assert rc == 0 and bool(torch.isfinite(loss).all())
    assert learn_lib.lib().mfg_seac_head(0, 0, 0, 4, 5, 10, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.99, 0.0, 0.5, 0.01,
                                         0, 0, 0, 0, 0, _stream()) == -1


# ---------------------------------------------------------------------------------------------------------------------
# the fixture on the device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('i', [0, 1, 2])
@pytest.mark.parametrize('algo', ['seac', 'iac'])
@pytest.mark.parametrize('fused', [True, False])
def test_learner_matches_reference_on_device(i, algo, fused):
    """The reference's fixture through mfg_packed_project_grouped + AgentNets (batched GEMMs, grouped GRU steps) + the
    loss head on the device, with the CPU replay's tolerances."""
    c, nets = load_case(np.load(GOLD), i, 'cuda')
    A, B, S1 = c['obs'].shape[:3]
    cross = algo == 'seac'
    out = forward(c, nets, cross, 'cuda')
    acts, rew, done = targets(c, 'cuda')
    h = hyper(c)  # gamma, entropy_coef, vf_coef, gae_coef
    if fused:
        eng = lambda v: v.permute(2, 1, 0).contiguous()  # noqa: E731  [A, B, T] -> the engine's [T, B, A]
        logits, critic = out['logits'], out['critic']
        if not cross:
            logits, critic = logits.reshape(A * B, S1, -1), critic.reshape(A * B, S1)
        n_act = torch.full((A,), int(c['n_actions']), dtype=torch.int32, device='cuda')
        st = (B * A, A, 1)
        loss = S._SEACHead.apply(logits, critic, eng(acts[:, :, 1:]).to(torch.int32), st, eng(rew), st, eng(done), st,
                                 n_act, A, B, *h, cross)
    elif cross:
        loss = M.seac_loss_terms(out['logits'].view(A, A, B, S1, -1)[:, :, :, :-1], out['critic'].view(A, A, B, S1),
                                 acts[:, :, 1:], rew, done, *h)
    else:
        loss = M.iac_loss_terms(out['logits'][:, :, :-1], out['critic'], acts[:, :, 1:], rew, done, *h)
    check_loss_and_grads(c, nets, loss, algo)


# ---------------------------------------------------------------------------------------------------------------------
# the engine
# ---------------------------------------------------------------------------------------------------------------------
def _spy(tr):
    """Keep the acting logits of every step."""
    acting, sample = [], tr._sample

    def spy(logits, t):
        acting.append(logits.clone())
        sample(logits, t)
    tr._sample = spy
    return acting


@pytest.mark.parametrize('cls', ['BatchedIAC', 'BatchedSEAC'])
@pytest.mark.parametrize('fused', [True, False])
def test_learners_on_rooms4(cls, fused):
    from mfg_amd.factory import BatchedFactory
    f = BatchedFactory('rooms4.yaml', 8, seed_base=3)
    torch.manual_seed(0)
    tr = getattr(M, cls)(f, n_steps=5, cap=64, fused_head=fused)
    A, B, T = tr.A, tr.B, tr.T
    acting = _spy(tr)
    learn, tr.learn = tr.learn, lambda: None
    for _ in range(T):
        tr.step()
    # before any weight change: the window's stored inputs and targets equal the step-by-step acting pass
    with torch.no_grad():
        lg = tr.evaluate()['logits']
    if tr.cross:
        lg = torch.stack([lg.view(A, A, B, T + 1, -1)[a, a] for a in range(A)])
    assert torch.allclose(lg[:, :, :T], torch.stack(acting, 2), rtol=1e-4, atol=1e-5)
    for s in range(T):
        d = tr.done[s].bool().view(-1, 1)
        assert torch.equal(tr.act_in[s + 1], torch.where(d, torch.full_like(tr.act_in[s + 1], -1), tr.act[s].long()))
        assert bool(((tr.act[s] >= 0) & (tr.act[s] < tr.n_max)).all())
    assert bool((tr.act_in[0] == -1).all())
    w0 = [p.detach().clone() for p in tr.nets.agent_params()]
    tr.learn = learn
    tr.learn()
    tr.train(1)
    assert tr.updates == 2 and tr.last_loss.shape == (A,) and bool(torch.isfinite(tr.last_loss).all())
    for a in range(A):  # every agent's network moved
        assert any(not torch.equal(p0[a], p.detach()[a]) for p0, p in zip(w0, tr.nets.agent_params()))
    assert float(tr.reward_sum) != 0.0
    f.close()


def test_fused_head_matches_tensor_head_on_a_window():
    """fused_head True / False on one window of the engine: parameter gradients of both heads at the learner tests'
    rtol 1e-4 / atol 1e-6, relative to each tensor's largest gradient."""
    from mfg_amd.factory import BatchedFactory
    f = BatchedFactory('rooms4.yaml', 8, seed_base=3)
    torch.manual_seed(0)
    tr = M.BatchedSEAC(f, n_steps=5, cap=64)
    tr.learn = lambda: None
    for _ in range(tr.T):
        tr.step()
    res = {}
    for fused in (True, False):
        tr.fused_head = fused
        tr.nets.zero_grad()
        loss = tr.loss()
        loss.sum().backward()
        res[fused] = (loss.detach(), [p.grad.clone() for p in tr.nets.agent_params()])
    assert torch.allclose(res[True][0], res[False][0], rtol=1e-5, atol=1e-7)
    for a, b in zip(res[True][1], res[False][1]):
        assert float((a - b).abs().max()) <= 1e-4 * float(b.abs().max()) + 1e-6
    f.close()


def test_iac_on_a_heterogeneous_team():
    """alltest16: four archetypes with different action counts. Every sampled action is inside its agent's range
    (one mfg_sample_categorical per agent block); the shared-network learner still refuses the team."""
    from mfg_amd.factory import BatchedFactory
    f = BatchedFactory('alltest16.yaml', 4, seed_base=1)
    n_act = [int(x) for x in f.spec.n_actions]
    assert len(set(n_act)) > 1
    with pytest.raises(ValueError, match='same number of actions'):
        M.BatchedA2C(f)
    with pytest.raises(ValueError, match='same number of actions'):
        M.BatchedSEAC(f)
    torch.manual_seed(0)
    tr = M.BatchedIAC(f, n_steps=5, cap=256)
    seen = []
    learn = tr.learn

    def spy_learn():
        seen.append(tr.act.clone())
        learn()
    tr.learn = spy_learn
    tr.train(2)
    assert tr.updates == 2 and bool(torch.isfinite(tr.last_loss).all())
    lim = torch.tensor(n_act, device='cuda').view(1, 1, -1)
    for act in seen:
        assert bool(((act >= 0) & (act < lim)).all())
    hi = torch.stack(seen).amax((0, 1, 2))
    assert bool((hi[torch.tensor(n_act, device='cuda') > 4] >= 4).any())  # the larger heads are used beyond the smallest one's range
    f.close()
