"""The evaluator on the CPU (mfg_amd/evaluate.py: eval_fold, actor_step, BatchedEvaluator's loop and frame,
load_reference_checkpoint).

Golden vectors from the reference's own evaluation loops (tests/golden/marl_eval.npz, tools/gen_golden_eval.py:
LoopSNAC.eval_loop and LoopIAC.eval_loop on the reference env): the f32 reward sums of the frame are compared bit for
bit (as f64 values). The first-step logits pass obs_proj as a sum over the packed nonzero entries instead of the dense
nn.Linear (another summation order): rtol 1e-4 / atol 1e-5, the bound tests/test_mappo.py uses for the same step.
"""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import eval_ref as R
from scripted import ScriptedEngine, pack
from mfg_amd.evaluate import (BatchedEvaluator, actor_step, eval_fold, load_reference_checkpoint, natural_key,
                              sample_inversion)
from mfg_amd.marl import AgentNets, RecurrentAC


# ---------------------------------------------------------------------------------------------------------------------
# the fold against the reference frame
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('tag', R.CASES)
def test_tensor_fold_reproduces_the_reference_frame(tag):
    c = R.load_case(tag)
    A, n_ep = int(c['n_agents']), int(c['n_episodes'])
    eps, ln, cnt = torch.zeros((1, A)), torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32)
    rows, lengths = torch.zeros((1, n_ep, A + 1)), torch.zeros((1, n_ep), dtype=torch.int32)
    fin = torch.zeros((), dtype=torch.int32)
    for r, d in zip(c['rewards'], c['dones']):
        eval_fold(torch.from_numpy(r)[None], torch.tensor([d]), n_ep, eps, ln, cnt, rows, lengths, fin)
    assert int(fin) == 1 and int(cnt) == n_ep
    assert np.array_equal(rows[0].double().numpy(), R.frame_rows(c))
    assert np.array_equal(lengths[0].numpy(), c['lengths'])
    ref_rows, ref_len = R.fold_loop(c['rewards'][:, None], c['dones'][:, None], n_ep)
    assert np.array_equal(rows.numpy(), ref_rows) and np.array_equal(lengths.numpy(), ref_len)


def _replay_evaluator(c, **kw):
    eng = R.ReplayEngine(c['rewards'][:, None], c['dones'][:, None], lmax=c['obs0'].shape[1], obs_hw=c['obs0'].shape[2:])
    return eng, BatchedEvaluator(R.fake_factory(eng, int(c['n_actions'])), R.case_policy(c), int(c['n_episodes']), **kw)


@pytest.mark.parametrize('tag', R.CASES)
def test_frame_is_the_reference_frame(tag):
    c = R.load_case(tag)
    eng, ev = _replay_evaluator(c)
    ev.run(actions=torch.from_numpy(c['actions'])[:, None])
    assert ev.steps == len(c['dones']) and ev.complete()
    assert all(torch.equal(a[0], torch.from_numpy(b)) for a, b in zip(eng.seen, c['actions']))
    fr = ev.frame(env=0)
    assert list(fr.columns) == ['episode', 'agent', 'reward']
    assert [str(t) for t in fr.dtypes] == [str(t) for t in c['frame_dtypes']]
    names = [f'agent#{i}' for i in range(int(c['n_agents']))] + ['sum']
    assert fr['episode'].tolist() == c['frame_episode'].tolist()
    assert fr['agent'].tolist() == [names[i] for i in c['frame_agent']]
    assert np.array_equal(fr['reward'].to_numpy(), c['frame_reward'])
    assert np.array_equal(ev.lengths[0].numpy(), c['lengths'])
    al = ev.frame()
    assert list(al.columns) == ['env', 'episode', 'agent', 'reward'] and len(al) == len(fr)
    assert al['env'].tolist() == [0] * len(fr) and np.array_equal(al['reward'].to_numpy(), c['frame_reward'])


# ---------------------------------------------------------------------------------------------------------------------
# the loop on a scripted engine
# ---------------------------------------------------------------------------------------------------------------------
def _scripted(A=2, B=3, n_episodes=3, **kw):
    eng = ScriptedEngine(B=B, A=A)
    f = SimpleNamespace(engine=eng, spec=SimpleNamespace(n_actions=[4] * A), _created=False, seed_base=0, t=0)
    torch.manual_seed(0)
    net = RecurrentAC(4, 4, 6, 4, 5, 5, A, use_agent_embedding=False)
    return eng, BatchedEvaluator(f, net, n_episodes, record=True, generator=torch.Generator().manual_seed(1), **kw)


@pytest.mark.parametrize('A,poll', [(2, 1), (2, 5), (1, 1)])
def test_evaluator_on_the_scripted_engine(A, poll):
    """Env 2 ends an episode on its very first step (k = 1) and has its three rows at k = 15; env 0 needs until k = 21,
    so env 2 keeps stepping with nothing more to write."""
    eng, ev = _scripted(A=A, poll_every=poll)
    rows = ev.run()
    assert ev.complete() and ev.steps == (21 if poll == 1 else 25)
    assert ev.actions.shape == (ev.steps, 3, A) and ev.rewards.shape == (ev.steps, 3, A)
    assert int(ev.actions.min()) >= 0 and int(ev.actions.max()) < 4
    ref_rows, ref_len = R.fold_loop(ev.rewards.numpy(), ev.dones.numpy(), 3)
    assert np.array_equal(rows.numpy(), ref_rows) and np.array_equal(ev.lengths.numpy(), ref_len)
    assert ev.lengths[2].tolist() == [1, 7, 7] and ev.lengths[0].tolist() == [7, 7, 7]
    assert ev.count.tolist() == [3, 3, 3]
    # a second run starts over and, with the generator re-seeded, repeats itself
    first = rows.clone(), ev.actions.clone()
    ev.gen.manual_seed(1)
    ev.run()
    assert torch.equal(first[0], ev.rows) and torch.equal(first[1], ev.actions)
    # replaying the recorded actions gives the same rows
    ev.run(actions=first[1])
    assert torch.equal(first[0], ev.rows)


def test_per_agent_networks_act_on_the_cpu():
    """An AgentNets policy through the tensor path (obs_proj of the packed rows per agent, forward_emb, inversion)."""
    c = R.load_case('iac')
    steps = len(c['dones'])
    eng = R.ReplayEngine(np.repeat(c['rewards'][:, None], 2, 1), np.stack([c['dones'], np.roll(c['dones'], 3)], 1),
                         lmax=c['obs0'].shape[1], obs_hw=c['obs0'].shape[2:])
    ev = BatchedEvaluator(R.fake_factory(eng, int(c['n_actions'])), R.case_policy(c), 2, record=True, poll_every=1,
                          cap=4, generator=torch.Generator().manual_seed(2))
    assert not ev.fused and not ev.shared
    rows = ev.run(max_steps=steps)
    assert ev.complete() and ev.steps < steps
    ref_rows, ref_len = R.fold_loop(ev.rewards.numpy(), ev.dones.numpy(), 2)
    assert np.array_equal(rows.numpy(), ref_rows) and np.array_equal(ev.lengths.numpy(), ref_len)
    assert int(ev.actions.min()) >= 0 and int(ev.actions.max()) < int(c['n_actions'])
    assert len(set(ev.actions.flatten().tolist())) > 1 and all(torch.equal(a, b) for a, b in zip(eng.seen, ev.actions))
    lg = ev.first_logits  # [B, A, n]: both envs saw the same first obs
    assert torch.equal(lg[0], lg[1]) and not torch.equal(lg[0, 0], lg[0, 1])


def test_greedy_and_restart_inputs():
    """greedy takes the argmax; after a done the policy sees action -1 and a zero state (the first-step logits again for
    the same obs embedding)."""
    eng, ev = _scripted(A=2, greedy=True, poll_every=1)
    ev.run(max_steps=1)
    lg = ev.first_logits
    assert torch.equal(ev.actions[0], lg.argmax(-1).to(torch.int32))
    net = ev.net
    emb = ev.pobs.emb[0].view(ev.N, -1)
    want, h = actor_step(net, emb, torch.where(ev.done.bool()[:, None], -1, ev.act.long()).view(-1),
                         ev.h.view(ev.N, -1) * (~ev.done.bool()).float().repeat_interleave(2)[:, None])
    before = ev.h.clone()
    ev._act(False, lg2 := torch.zeros_like(lg))
    assert torch.equal(lg2.view(ev.N, -1), want) and bool(ev.done[2]) and not torch.equal(before, ev.h)
    fresh, _ = actor_step(net, emb[4:6], torch.full((2,), -1), torch.zeros(2, 5))
    assert torch.equal(lg2[2], fresh)


def test_sample_inversion_bins_and_non_finite_rows():
    lg = torch.log(torch.tensor([[0.25, 0.25, 0.5], [0.25, 0.25, 0.5], [0.25, 0.25, 0.5], [1.0, 1.0, 1.0]]))
    lg[3, 1] = float('nan')
    got = sample_inversion(lg, torch.tensor([0.1, 0.3, 0.99, 0.5]))
    assert got.tolist() == [0, 1, 2, -1] and got.dtype == torch.int32
    assert sample_inversion(lg[:3], torch.tensor([0.9, 0.9, 0.2]), n_act=2).tolist() == [1, 1, 0]


# ---------------------------------------------------------------------------------------------------------------------
# the tensor acting path
# ---------------------------------------------------------------------------------------------------------------------
def test_actor_step_is_forward_emb_restricted_to_the_actor():
    g = torch.Generator().manual_seed(3)
    c = R.load_case('snac')
    net = R.case_policy(c)
    N, E, H = 7, net.obs_proj.weight.shape[0], net.hidden_size_actor
    emb, h = torch.randn(N, E, generator=g), torch.randn(N, H, generator=g)
    a_in = torch.randint(-1, int(c['n_actions']), (N,), generator=g)
    with torch.no_grad():
        out = net.forward_emb(emb[:, None], a_in[:, None], h[:, None], torch.zeros(N, 1, net.hidden_size_critic))
        lg, hn = actor_step(net, emb, a_in, h)
    assert torch.equal(lg, out['logits'][:, 0]) and torch.equal(hn, out['hidden_actor'][:, 0])
    nets = R.case_policy(R.load_case('iac'))
    A, B = nets.A, 5
    emb, h = torch.randn(A, B, E, generator=g), torch.randn(A, B, H, generator=g)
    a_in = torch.randint(-1, int(c['n_actions']), (A, B), generator=g)
    with torch.no_grad():
        out = nets.forward_emb(emb[:, :, None], a_in[:, :, None], h, torch.randn(A, B, nets.hidden_size_critic, generator=g))
        lg, hn = actor_step(nets, emb, a_in, h)
    assert torch.equal(lg, out['logits'][:, :, 0]) and torch.equal(hn, out['hidden_actor'][:, :, 0])


def _first_logits(policy, c):
    idx, val = pack(c['obs0'][:, None], cap=64)  # [A, 1, cap]
    A = idx.shape[0]
    with torch.no_grad():
        if isinstance(policy, AgentNets):
            emb = policy.project(idx.permute(1, 0, 2)[:, None], val.permute(1, 0, 2)[:, None])[:, :, 0]  # [A, 1, E]
            return actor_step(policy, emb, torch.full((A, 1), -1), torch.zeros(A, 1, policy.hidden_size_actor))[0][:, 0]
        emb = policy.project_packed(idx, val)[:, 0]
        return actor_step(policy, emb, torch.full((A,), -1), torch.zeros(A, policy.hidden_size_actor))[0]


@pytest.mark.parametrize('tag', R.CASES)
def test_first_step_logits_match_the_reference(tag):
    c = R.load_case(tag)
    lg = _first_logits(R.case_policy(c), c)
    assert torch.allclose(lg, torch.from_numpy(c['logits0']), rtol=1e-4, atol=1e-5), (lg - torch.from_numpy(c['logits0'])).abs().max()


# ---------------------------------------------------------------------------------------------------------------------
# reference checkpoints
# ---------------------------------------------------------------------------------------------------------------------
def test_natural_key_orders_digit_runs_by_value():
    names = [f'agent#{i}.pt' for i in range(12)]
    assert sorted(sorted(names), key=natural_key) == names
    assert sorted(['b2', 'a10', 'a9', 'A1'], key=natural_key) == ['A1', 'a9', 'a10', 'b2']


def _module(seed, A):
    torch.manual_seed(seed)
    return RecurrentAC(4, 3, 6, 4, 5, 5, A, use_agent_embedding=False)


def test_checkpoint_files_load_in_natural_order(tmp_path):
    A = 11
    mods = [_module(g, A) for g in range(A)]
    for g, m in enumerate(mods):
        torch.save(m.state_dict(), tmp_path / f'agent#{g}.pt')
    nets = AgentNets(4, 3, 6, 4, 5, 5, A)
    files = load_reference_checkpoint(nets, tmp_path)
    assert [f.name for f in files] == [f'agent#{g}.pt' for g in range(A)]
    for g, d in enumerate(nets.state_dicts()):  # agent#10 is network 10, not network 2
        assert all(torch.equal(d[k], v) for k, v in mods[g].state_dict().items()), g
    # a learner-like holder works too, and fewer files than networks load the first ones (zip)
    (tmp_path / 'agent#10.pt').unlink()
    holder = SimpleNamespace(nets=AgentNets(4, 3, 6, 4, 5, 5, A))
    keep = holder.nets.state_dicts()[10]
    assert len(load_reference_checkpoint(holder, tmp_path)) == 10
    got = holder.nets.state_dicts()
    assert torch.equal(got[9]['mix.1.weight'], mods[9].state_dict()['mix.1.weight'])
    assert torch.equal(got[10]['mix.1.weight'], keep['mix.1.weight'])


def test_shared_checkpoint_needs_exactly_one_file(tmp_path):
    net = _module(0, 2)
    with pytest.raises(ValueError, match='single set of weights'):
        load_reference_checkpoint(net, tmp_path)
    torch.save(_module(1, 2).state_dict(), tmp_path / 'agent#0.pt')
    torch.save(_module(2, 2).state_dict(), tmp_path / 'agent#1.pt')
    with pytest.raises(ValueError, match='single set of weights but got 2'):
        load_reference_checkpoint(net, tmp_path)
    (tmp_path / 'agent#1.pt').unlink()
    load_reference_checkpoint(SimpleNamespace(net=net), tmp_path)
    assert torch.equal(net.mix[1].weight, _module(1, 2).mix[1].weight)
    with pytest.raises(TypeError):
        load_reference_checkpoint(object(), tmp_path)


@pytest.mark.parametrize('tag', R.CASES)
def test_loaded_fixture_weights_give_the_fixture_logits(tag, tmp_path):
    c = R.load_case(tag)
    for g, st in enumerate(R.case_states(c)):
        torch.save(st, tmp_path / f'agent#{g}.pt')
    ref = R.case_policy(c)
    if isinstance(ref, AgentNets):
        policy = AgentNets(ref.cfg['observation_size'], ref.n_act, ref.obs_emb_size, ref.action_emb_size,
                           ref.hidden_size_actor, ref.hidden_size_critic, ref.A)
    else:
        torch.manual_seed(99)
        policy = RecurrentAC(c['obs0'].shape[1:], int(c['n_actions']), ref.obs_proj.weight.shape[0], ref.action_emb_size,
                             ref.hidden_size_actor, ref.hidden_size_critic, int(c['n_agents']), use_agent_embedding=False)
    load_reference_checkpoint(policy, tmp_path)
    lg = _first_logits(policy, c)
    assert torch.allclose(lg, torch.from_numpy(c['logits0']), rtol=1e-4, atol=1e-5)
