"""The evaluation kernels and the evaluator on the device (include/mfg_learn.h: mfg_policy_act, mfg_eval_fold;
mfg_amd/evaluate.py BatchedEvaluator).

mfg_policy_act is measured against the same formulas in torch f64, as tests/test_gpu_seac.py measures its kernels: the
f32 tensor code (torch, on the device) and the kernel are both compared with f64; the kernel's largest error on the
logits and on h' may be at most 4 times the f32 tensor code's, plus 1e-7 absolute. With MFG_EVAL_FIGURES set to a file
name the measured figures are written there as JSON.
    figures (MI355X): see profiles/eval.json "kernel_test"
The sampled action, the greedy action, the fold and the golden replay are exact checks.
"""
import json
import os
from pathlib import Path

import numpy as np
import pytest
import torch

from conftest import gpu_available
import eval_ref as R
import mfg_amd.evaluate as EV
from mfg_amd import learn_lib
from mfg_amd.marl import AgentNets, RecurrentAC

pytestmark = pytest.mark.gpu
FIGURES = {}
SIZES = [(96, 16, 64), (12, 4, 8), (37, 5, 5)]


def _need_gpu():
    if not gpu_available():
        pytest.skip('no GPU')


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _record(key, fig):
    FIGURES[key] = fig
    dst = os.environ.get('MFG_EVAL_FIGURES')
    if dst:
        Path(dst).write_text(json.dumps(FIGURES, indent=1))


# ---------------------------------------------------------------------------------------------------------------------
# mfg_policy_act against the formulas
# ---------------------------------------------------------------------------------------------------------------------
def make_weights(g, E, AE, H, n_max, gen):
    """g actors, K-major as mfg_actor_weights wants them, drawn like nn.Linear / nn.GRU draw theirs (uniform within
    1 / sqrt(fan_in)); every row of the action embedding is nonzero, row 0 included."""
    def u(*shape, fan):
        return (torch.rand(shape, generator=gen) * 2 - 1) / fan ** 0.5
    return dict(action_emb=torch.randn((g, n_max + 1, AE), generator=gen),
                w1t=u(g, E + AE, E, fan=E + AE), b1=u(g, E, fan=E + AE), w3t=u(g, E, E, fan=E), b3=u(g, E, fan=E),
                wiht=u(g, E, 3 * H, fan=H), bih=u(g, 3 * H, fan=H), whht=u(g, H, 3 * H, fan=H), bhh=u(g, 3 * H, fan=H),
                wat=u(g, H, H, fan=H), ba=u(g, H, fan=H), wbt=u(g, H, n_max, fan=H), bb=u(g, n_max, fan=H))


def make_inputs(B, A, E, H, n_act, gen):
    """Engine-order inputs: prev_done set for about a third of the envs (always for env 0 when there are several rows),
    prev_action -1 in places, otherwise within the agent's own action count."""
    emb = torch.randn((B, A, E), generator=gen)
    h = torch.randn((B, A, H), generator=gen) * 0.5
    prev_done = (torch.rand(B, generator=gen) < 0.33).to(torch.uint8)
    if B > 1:
        prev_done[0], prev_done[1] = 1, 0
    cnt = torch.tensor([n_act[i % len(n_act)] for i in range(A)])
    prev_action = (torch.rand((B, A), generator=gen) * cnt).floor().to(torch.int32)
    prev_action[torch.rand((B, A), generator=gen) < 0.2] = -1
    if B > 2:
        prev_action[B - 1, A - 1] = -1
    u = torch.rand((B, A), generator=gen)
    return emb, h, prev_action, prev_done, u


def formulas(w, emb, h, prev_action, prev_done, dtype):
    """include/mfg_learn.h's formulas in torch on the device: (logits [B, A, n_max], h' [B, A, H])."""
    dev = 'cuda'
    w = {k: v.to(device=dev, dtype=dtype) for k, v in w.items() if not k.startswith('_')}
    emb, h = emb.to(device=dev, dtype=dtype), h.to(device=dev, dtype=dtype)
    B, A, E = emb.shape
    g = w['w1t'].shape[0]
    H = w['wat'].shape[1]
    net = torch.arange(A, device=dev) % g
    fresh = prev_done.to(dev).bool()[:, None]
    a_in = torch.where(fresh, -1, prev_action.to(dev).long()) + 1  # [B, A]
    h_in = torch.where(fresh[..., None], torch.zeros_like(h), h).transpose(0, 1)  # [A, B, H]
    ae = w['action_emb'][net[None].expand(B, A), a_in]  # [B, A, AE]
    ax = torch.tanh(torch.cat([emb, ae], -1)).transpose(0, 1)  # [A, B, E + AE]

    def lin(x, wt, b):
        return torch.baddbmm(w[b][net][:, None], x, w[wt][net])

    x = lin(torch.tanh(lin(ax, 'w1t', 'b1')), 'w3t', 'b3')
    gi, gh = lin(x, 'wiht', 'bih'), lin(h_in, 'whht', 'bhh')
    r = torch.sigmoid(gi[..., :H] + gh[..., :H])
    z = torch.sigmoid(gi[..., H:2 * H] + gh[..., H:2 * H])
    n = torch.tanh(gi[..., 2 * H:] + r * gh[..., 2 * H:])
    hn = n + z * (h_in - n)
    lg = lin(torch.tanh(lin(hn, 'wat', 'ba')), 'wbt', 'bb')
    return lg.transpose(0, 1).contiguous(), hn.transpose(0, 1).contiguous()


def run_kernel(w, emb, h, prev_action, prev_done, u, n_act, layout='engine', greedy=False, guard=64, first=False):
    """One mfg_policy_act call on device copies (h, the actions and the logits inside guard words): returns
    (rc, logits [B, A, n_max], h' [B, A, H], act [B, A], guards_intact)."""
    dev = 'cuda'
    wd = {k: v.to(dev).contiguous() for k, v in w.items() if not k.startswith('_')}
    B, A, E = emb.shape
    H, n_max = w['wat'].shape[1], w['wbt'].shape[2]

    def guarded(t, fill):
        buf = torch.full((t.numel() + 2 * guard,), fill, dtype=t.dtype, device=dev)
        buf[guard:guard + t.numel()] = t.reshape(-1).to(dev)
        return buf

    if layout == 'engine':
        e_d, h_src = emb.to(dev).contiguous(), h
        es, hs = (A * E, E), (A * H, H)
    else:  # agent-major [A, B, ..]
        e_d, h_src = emb.transpose(0, 1).contiguous().to(dev), h.transpose(0, 1).contiguous()
        es, hs = (E, B * E), (H, B * H)
    hb = guarded(h_src, 777.0)
    ab = guarded(prev_action, -99)
    lb = guarded(torch.zeros(B, A, n_max), 555.0)
    hv, av, lv = hb[guard:-guard], ab[guard:-guard], lb[guard:-guard]
    rc = EV.policy_act(wd, e_d, es, B, A, torch.tensor(n_act, dtype=torch.int32, device=dev), None if first else av,
                       None if first else prev_done.to(dev), hv, hs, u.to(dev), av, lv, greedy)
    torch.cuda.synchronize()
    ok = all(bool((b[:guard] == f).all()) and bool((b[-guard:] == f).all())
             for b, f in ((hb, 777.0), (ab, -99), (lb, 555.0)))
    hn = hv.view(B, A, H) if layout == 'engine' else hv.view(A, B, H).transpose(0, 1)
    return rc, lv.view(B, A, n_max).clone(), hn.contiguous().clone(), av.view(B, A).clone(), ok


def sampler(logits, u, n_act, g):
    """mfg_sample_categorical on logits [B, A, n_max] with agent i's count n_act[i % g]."""
    B, A, n_max = logits.shape
    out = torch.zeros((B, A), dtype=torch.int32, device='cuda')
    for i in range(A):
        lg, ui = logits[:, i].contiguous(), u[:, i].contiguous().cuda()
        o = torch.zeros(B, dtype=torch.int32, device='cuda')
        assert learn_lib.lib().mfg_sample_categorical(lg.data_ptr(), n_max, n_act[i % g], ui.data_ptr(), B,
                                                      o.data_ptr(), _stream()) == 0
        out[:, i] = o
    return out


def n_acts(n_max, g):
    """Per-network action counts: the largest first; different ones when there are several networks."""
    return [n_max, (n_max + 1) // 2, 1][:g] if g > 1 else [n_max]


@pytest.mark.parametrize('sizes', SIZES)
@pytest.mark.parametrize('g', [1, 3])
def test_policy_act_against_f64(g, sizes):
    _need_gpu()
    E, AE, H = sizes
    gen = torch.Generator().manual_seed(100 * g + E)
    shapes = [(1, 1), (2, 1), (86, 3)] if g == 1 else [(1, 3), (86, 3)]  # rows 1, 2, 258 (no tile multiple); 3, 258
    for n_max in (1, 11, 32):
        n_act = n_acts(n_max, g)
        w = make_weights(g, E, AE, H, n_max, gen)
        assert bool((w['action_emb'][:, 0] != 0).all())
        for B, A in shapes:
            emb, h, pa, pd, u = make_inputs(B, A, E, H, n_act, gen)
            assert B == 1 or (bool(pd.any()) and not bool(pd.all()) and (B == 2 or bool((pa == -1).any())))
            ref_l, ref_h = formulas(w, emb, h, pa, pd, torch.float64)
            f32_l, f32_h = formulas(w, emb, h, pa, pd, torch.float32)
            e32 = (float((f32_l.double() - ref_l).abs().max()), float((f32_h.double() - ref_h).abs().max()))
            for layout in ('engine', 'agent'):
                rc, lg, hn, act, ok = run_kernel(w, emb, h, pa, pd, u, n_act, layout)
                assert rc == 0 and ok
                ek = (float((lg.double() - ref_l).abs().max()), float((hn.double() - ref_h).abs().max()))
                key = f'g{g}.E{E}.AE{AE}.H{H}.n{n_max}.B{B}.A{A}.{layout}'
                _record(key, dict(kernel_logits=ek[0], f32_logits=e32[0], kernel_h=ek[1], f32_h=e32[1]))
                print(key, ek, e32)
                assert ek[0] <= 4 * e32[0] + 1e-7, (key, ek[0], e32[0])
                assert ek[1] <= 4 * e32[1] + 1e-7, (key, ek[1], e32[1])
                # the sampled action is mfg_sample_categorical on the kernel's own logits, on every row
                assert torch.equal(act, sampler(lg, u, n_act, g)), key
                assert int(act.min()) >= 0
                # greedy: argmax over the network's own count
                rc, lg2, hn2, act2, ok = run_kernel(w, emb, h, pa, pd, u, n_act, layout, greedy=True)
                assert rc == 0 and ok and torch.equal(lg2, lg) and torch.equal(hn2, hn)  # bit-identical again
                for i in range(A):
                    assert torch.equal(act2[:, i], lg[:, i, :n_act[i % g]].argmax(-1).to(torch.int32)), key


def test_policy_act_episode_start_and_determinism():
    """prev_* NULL is prev_done set everywhere; two launch shapes of the same rows give the same bits."""
    _need_gpu()
    gen = torch.Generator().manual_seed(5)
    E, AE, H, n_max = 96, 16, 64, 11
    w = make_weights(1, E, AE, H, n_max, gen)
    emb, h, pa, pd, u = make_inputs(70, 3, E, H, [n_max], gen)
    _, lg0, h0, a0, ok0 = run_kernel(w, emb, h, pa, pd, u, [n_max], first=True)
    _, lg1, h1, a1, ok1 = run_kernel(w, emb, h, pa, torch.ones_like(pd), u, [n_max])
    assert ok0 and ok1 and torch.equal(lg0, lg1) and torch.equal(h0, h1) and torch.equal(a0, a1)
    # the rows of env 5 alone (another block, another position in the tile)
    _, lg2, h2, a2, _ = run_kernel(w, emb[5:6], h[5:6], pa[5:6], pd[5:6], u[5:6], [n_max])
    _, lg3, h3, a3, _ = run_kernel(w, emb, h, pa, pd, u, [n_max])
    assert torch.equal(lg2[0], lg3[5]) and torch.equal(h2[0], h3[5]) and torch.equal(a2[0], a3[5])


@pytest.mark.parametrize('g', [1, 3])
def test_policy_act_nan_row_gives_minus_one(g):
    _need_gpu()
    gen = torch.Generator().manual_seed(7)
    E, AE, H, n_max = 37, 5, 5, 11
    n_act = n_acts(n_max, g)
    w = make_weights(g, E, AE, H, n_max, gen)
    emb, h, pa, pd, u = make_inputs(40, 3, E, H, n_act, gen)
    _, lg, hn, act, ok = run_kernel(w, emb, h, pa, pd, u, n_act)
    bad = emb.clone()
    bad[17, 1, 3] = float('nan')
    for greedy in (False, True):
        rc, lg2, hn2, act2, ok2 = run_kernel(w, bad, h, pa, pd, u, n_act, greedy=greedy)
        assert rc == 0 and ok and ok2, 'guard words around h, the actions or the logits changed'
        assert int(act2[17, 1]) == -1 and bool(torch.isnan(lg2[17, 1]).all())
        keep = torch.ones(40, 3, dtype=torch.bool)
        keep[17, 1] = False
        assert torch.equal(lg2[keep], lg[keep]) and torch.equal(hn2[keep], hn[keep])
        if not greedy:
            assert torch.equal(act2[keep], act[keep])
    # a network whose action count is outside [1, n_max]: -1 on its rows, nothing else
    wrong = list(n_act)
    wrong[-1] = n_max + 1
    rc, _, _, act3, ok3 = run_kernel(w, emb, h, pa, pd, u, wrong)
    assert rc == 0 and ok3 and bool((act3[:, (g - 1)::g] == -1).all())


def test_policy_act_refuses_sizes_over_its_limits():
    _need_gpu()
    gen = torch.Generator().manual_seed(9)
    for E, AE, H, n_max in ((129, 16, 64, 11), (96, 33, 64, 11), (96, 16, 129, 11), (96, 16, 64, 33)):
        assert not EV.act_supported(E, AE, H, n_max)
        w = make_weights(1, E, AE, H, n_max, gen)
        emb, h, pa, pd, u = make_inputs(2, 1, E, H, [n_max], gen)
        rc, lg, hn, act, ok = run_kernel(w, emb, h, pa, pd, u, [n_max])
        assert rc == -1 and ok and bool((lg == 0).all()) and torch.equal(hn, h.cuda()) and torch.equal(act, pa.cuda())
    assert EV.act_supported(128, 32, 128, 32)
    w = make_weights(2, 12, 4, 8, 5, gen)  # two networks for three agents
    emb, h, pa, pd, u = make_inputs(2, 3, 12, 8, [5, 5], gen)
    assert run_kernel(w, emb, h, pa, pd, u, [5, 5])[0] == -1
    # the largest supported sizes run
    w = make_weights(1, 128, 32, 128, 32, gen)
    emb, h, pa, pd, u = make_inputs(33, 2, 128, 128, [32], gen)
    rc, lg, hn, act, ok = run_kernel(w, emb, h, pa, pd, u, [32])
    ref_l, ref_h = formulas(w, emb, h, pa, pd, torch.float64)
    assert rc == 0 and ok and float((lg.double() - ref_l).abs().max()) < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# mfg_eval_fold
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('A', [1, 3, 128])
@pytest.mark.parametrize('B', [1, 65])
def test_eval_fold_kernel_is_the_float32_loop(A, B):
    _need_gpu()
    gen = torch.Generator().manual_seed(A * 100 + B)
    steps, n_ep = 40, 3
    rewards = torch.randn((steps, B, A), generator=gen, dtype=torch.float64) * 0.3  # no f32 values
    dones = (torch.rand((steps, B), generator=gen) < 0.2).to(torch.uint8)
    dones[0, 0] = 1  # done on an episode's first step
    dones[:6, B - 1] = torch.tensor([0, 1, 0, 1, 1, 0])  # env B - 1 has its rows after 5 steps and keeps stepping
    dones[-1] = 1
    dev = 'cuda'
    eps, ln = torch.zeros((B, A), device=dev), torch.zeros(B, dtype=torch.int32, device=dev)
    cnt = torch.zeros(B, dtype=torch.int32, device=dev)
    guard = 32
    rb = torch.full((B * n_ep * (A + 1) + 2 * guard,), 333.0, device=dev)
    rb[guard:-guard] = 0
    rows = rb[guard:-guard].view(B, n_ep, A + 1)
    lengths, fin = torch.zeros((B, n_ep), dtype=torch.int32, device=dev), torch.zeros((), dtype=torch.int32, device=dev)
    rw, dn = rewards.to(dev), dones.to(dev)
    L = learn_lib.lib()
    for t in range(steps):
        assert L.mfg_eval_fold(rw[t].data_ptr(), dn[t].data_ptr(), B, A, n_ep, eps.data_ptr(), ln.data_ptr(),
                               cnt.data_ptr(), rows.data_ptr(), lengths.data_ptr(), fin.data_ptr(), _stream()) == 0
    ref_rows, ref_len = R.fold_loop(rewards.numpy(), dones.numpy(), n_ep)
    assert np.array_equal(rows.cpu().numpy(), ref_rows) and np.array_equal(lengths.cpu().numpy(), ref_len)
    assert bool((rb[:guard] == 333.0).all()) and bool((rb[-guard:] == 333.0).all())
    done_envs = int((dones.sum(0) >= n_ep).sum())
    assert int(fin) == done_envs and int((cnt == n_ep).sum()) == done_envs and int(cnt.max()) <= n_ep
    # the tensor fold is the same thing
    st = [torch.zeros((B, A)), torch.zeros(B, dtype=torch.int32), torch.zeros(B, dtype=torch.int32),
          torch.zeros((B, n_ep, A + 1)), torch.zeros((B, n_ep), dtype=torch.int32), torch.zeros((), dtype=torch.int32)]
    for t in range(steps):
        EV.eval_fold(rewards[t], dones[t], n_ep, *st)
    assert np.array_equal(st[3].numpy(), ref_rows) and int(st[5]) == done_envs


# ---------------------------------------------------------------------------------------------------------------------
# golden replay on the engine
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', R.CASES)
def test_golden_replay_on_the_engine(tag):
    """The reference loops' recorded actions through the HIP engine with auto-reset and the fold kernel give the
    reference frame bit for bit, with the reference's episode lengths."""
    _need_gpu()
    from mfg_amd.factory import BatchedFactory
    c = R.load_case(tag)
    f = BatchedFactory('eval_trio.yaml', 1, seed_base=int(c['py_seed']))
    ev = EV.BatchedEvaluator(f, R.case_policy(c), int(c['n_episodes']), record=True)
    ev.run(actions=torch.from_numpy(c['actions'])[:, None])
    assert ev.steps == len(c['dones']) and ev.complete()
    assert np.array_equal(ev.rewards[:, 0].cpu().numpy(), c['rewards'])
    assert np.array_equal(ev.dones[:, 0].cpu().numpy(), c['dones'])
    assert np.array_equal(ev.rows[0].double().cpu().numpy(), R.frame_rows(c))
    assert np.array_equal(ev.lengths[0].cpu().numpy(), c['lengths'])
    fr = ev.frame(env=0)
    assert np.array_equal(fr['reward'].to_numpy(), c['frame_reward'])
    assert fr['episode'].tolist() == c['frame_episode'].tolist()
    f.close()


# ---------------------------------------------------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------------------------------------------------
def _rooms4(per_agent, fused, seed=3, **kw):
    from mfg_amd.factory import BatchedFactory
    f = BatchedFactory('rooms4.yaml', 8, seed_base=seed)
    eng = f.engine
    kdim = eng.lmax * eng.obs_hw[0] * eng.obs_hw[1]
    n = int(f.spec.n_actions[0])
    torch.manual_seed(0)
    if per_agent:
        policy = AgentNets(kdim, [n] * eng.A, 96, 16, 64, 64, eng.A)
    else:
        policy = RecurrentAC(kdim, n, 96, 16, 64, 64, eng.A, use_agent_embedding=False)
    ev = EV.BatchedEvaluator(f, policy, 1, fused=fused, record=True, poll_every=50, cap=kdim,
                             generator=torch.Generator(device='cuda').manual_seed(1), **kw)
    assert ev.fused == fused
    return f, ev


def _evaluator_weights(ev):
    return {k: v.cpu() for k, v in EV.actor_weights(ev.net).items()}


@pytest.mark.parametrize('per_agent', [False, True])
@pytest.mark.parametrize('fused', [True, False])
def test_evaluator_on_rooms4(per_agent, fused):
    _need_gpu()
    f, ev = _rooms4(per_agent, fused)
    rows = ev.run(max_steps=2000).clone()
    assert ev.complete() and ev.steps % 50 == 0
    acts = ev.actions.clone()
    assert int(acts.min()) >= 0 and int(acts.max()) < ev.n_max
    ref_rows, ref_len = R.fold_loop(ev.rewards.cpu().numpy(), ev.dones.cpu().numpy(), 1)
    assert np.array_equal(rows.cpu().numpy(), ref_rows) and np.array_equal(ev.lengths.cpu().numpy(), ref_len)
    assert int(ev.lengths.min()) >= 1 and len(ev.frame()) == 8 * (ev.A + 1)
    f.close()
    # the recorded actions replayed on fresh envs of the same seeds give the same rows
    f2, ev2 = _rooms4(per_agent, fused)
    ev2.run(actions=acts)
    assert torch.equal(ev2.rows, rows) and torch.equal(ev2.rewards, ev.rewards)
    f2.close()


@pytest.mark.parametrize('per_agent', [False, True])
def test_fused_and_tensor_first_step_agree(per_agent):
    """Same envs, same weights: the first step's logits of the fused and the tensor path differ by no more than their
    two errors against f64 (kernel <= 4 f32 + 1e-7, so at most 5 f32 + 1e-7)."""
    _need_gpu()
    (fa, ea), (fb, eb) = _rooms4(per_agent, True), _rooms4(per_agent, False)
    out = []
    for ev in (ea, eb):
        ev.reset()
        lg = torch.zeros((ev.B, ev.A, ev.n_max), device='cuda')
        ev._act(True, lg)
        out.append(lg)
    emb = (eb._emb.transpose(0, 1) if per_agent else eb.pobs.emb[0]).cpu()
    B, A = eb.B, eb.A
    ref, _ = formulas(_evaluator_weights(eb), emb, torch.zeros(B, A, 64), torch.zeros((B, A), dtype=torch.int32),
                      torch.ones(B, dtype=torch.uint8), torch.float64)
    e_f, e_u = (float((x.double() - ref).abs().max()) for x in out)
    d = float((out[0] - out[1]).abs().max())
    _record(f'rooms4.first_step.per_agent{int(per_agent)}', dict(kernel_logits=e_f, f32_logits=e_u, fused_vs_tensor=d))
    print(e_f, e_u, d)
    assert e_f <= 4 * e_u + 1e-7 and d <= 5 * e_u + 1e-7
    fa.close()
    fb.close()
