"""The per-agent-network learners on the CPU (mfg_amd/seac.py, re-exported by mfg_amd.marl: AgentNets, iac_loss_terms,
seac_loss_terms, BatchedIAC, BatchedSEAC).

Golden vectors from the reference's own networks and losses (tests/golden/marl_seac.npz, tools/gen_golden_seac.py:
algorithms/marl/seac.py LoopSEAC.actor_critic and base_ac.py BaseActorCritic.actor_critic per agent, two "envs" per
case as the mean of two reference runs). Tolerances are tests/test_mappo.py's: loss within 1e-5 relative (+1e-7),
gradients rtol 1e-4 / atol 1e-6; the optimiser step (per-agent clip_grad_norm_(0.5) + RMSprop(3e-4, eps 1e-5) on the
stacked parameters) is pinned on the fixture's own gradients, weights within 1e-6 absolute.
"""
from pathlib import Path

import numpy as np
import pytest
import torch

from mfg_amd.marl import (AgentNets, BatchedA2C, BatchedIAC, BatchedSEAC, RecurrentAC, a2c_loss_terms, iac_loss_terms,
                          seac_loss_terms)
from scripted import ScriptedEngine, factory, pack

GOLD = Path(__file__).resolve().parent / 'golden' / 'marl_seac.npz'
CASES = [0, 1, 2]


def load_case(z, i, device='cpu'):
    """(c, nets): the case's arrays and an AgentNets holding its per-network weights."""
    c = {k.split('.', 1)[1]: z[k] for k in z.files if k.startswith(f's{i}.')}
    A = int(c['n_agents'])
    dicts = [{k[len(f'w.{g}.'):]: torch.from_numpy(v) for k, v in c.items() if k.startswith(f'w.{g}.')}
             for g in range(A)]
    d0 = dicts[0]
    nets = AgentNets(int(np.prod(c['obs'].shape[3:])), int(c['n_actions']), d0['obs_proj.weight'].shape[0],
                     d0['action_emb.weight'].shape[1], d0['gru_actor.weight_hh_l0'].shape[1],
                     d0['gru_critic.weight_hh_l0'].shape[1], A)
    nets.load_state_dicts(dicts)
    return c, nets.to(device)


def hyper(c):
    return tuple(float(c[k]) for k in ('gamma', 'entropy_coef', 'vf_coef', 'gae_coef'))


def packed_window(c, cap=32, device='cpu'):
    """The case's observations [A, B, T+1, ...] as a packed window in engine order [T+1, B, A, cap]."""
    A, B, S = c['obs'].shape[:3]
    idx, val = pack(c['obs'].reshape((A * B, S) + c['obs'].shape[3:]), cap)
    idx = idx.view(torch.int16).view(A, B, S, cap).permute(2, 1, 0, 3).contiguous().view(torch.uint16)
    return idx.to(device), val.view(A, B, S, cap).permute(2, 1, 0, 3).contiguous().to(device)


def targets(c, device='cpu'):
    acts = torch.from_numpy(c['actions']).long().to(device)  # [A, B, T+1]: entry 0 = the action before the window
    return acts, torch.from_numpy(c['reward']).to(device), torch.from_numpy(c['done']).to(device)


def forward(c, nets, cross, device='cpu'):
    """The window's forward: logits [A, n, T+1, n_act], critic [A, n, T+1], n = B (own) or A B (cross)."""
    A, B, S = c['obs'].shape[:3]
    idx, val = packed_window(c, device=device)
    acts, _, _ = targets(c, device)
    emb = nets.project(idx, val, all_=cross)
    ha, hc = torch.from_numpy(c['ha0']).to(device), torch.from_numpy(c['hc0']).to(device)
    if cross:
        emb = emb.view(A, A * B, S, -1)
        acts = acts[None].expand(A, A, B, S).reshape(A, A * B, S)
        ha, hc = (h[None].expand(A, *h.shape).reshape(A, A * B, -1) for h in (ha, hc))
    return nets.forward_emb(emb, acts, ha, hc)


def torch_loss(c, nets, algo, device='cpu', terms=False):
    A, B, S = c['obs'].shape[:3]
    out = forward(c, nets, algo == 'seac', device)
    acts, rew, done = targets(c, device)
    if algo == 'seac':
        return seac_loss_terms(out['logits'].view(A, A, B, S, -1)[:, :, :, :-1], out['critic'].view(A, A, B, S),
                               acts[:, :, 1:], rew, done, *hyper(c), terms=terms)
    return iac_loss_terms(out['logits'][:, :, :-1], out['critic'], acts[:, :, 1:], rew, done, *hyper(c), terms=terms)


def check_loss_and_grads(c, nets, loss, algo):
    A = nets.A
    for g in range(A):
        ref = float(c[f'{algo}.loss.{g}'])
        assert abs(loss[g].item() - ref) <= 1e-5 * abs(ref) + 1e-7, (algo, g, loss[g].item(), ref)
    nets.zero_grad()
    loss.sum().backward()
    for k, p in nets.P.items():
        for g in range(A):
            got = (p.grad[g] if p.grad is not None else torch.zeros_like(p[g])).cpu()
            gr = torch.from_numpy(c[f'{algo}.g.{g}.{k}'])
            assert torch.allclose(got, gr, rtol=1e-4, atol=1e-6), (algo, g, k, (got - gr).abs().max())


@pytest.mark.parametrize('algo', ['seac', 'iac'])
@pytest.mark.parametrize('i', CASES)
def test_loss_matches_reference(i, algo):
    c, nets = load_case(np.load(GOLD), i)
    check_loss_and_grads(c, nets, torch_loss(c, nets, algo), algo)


def check_step(c, nets, algo):
    """Per-agent clip + one RMSprop step on the stacked parameters from the fixture's own gradients."""
    opt = torch.optim.RMSprop(nets.agent_params(), lr=3e-4, eps=1e-5)
    for k, p in nets.P.items():
        p.grad = torch.stack([torch.from_numpy(c[f'{algo}.g.{g}.{k}']) for g in range(nets.A)]).to(p.device)
    norms = nets.clip_grad_norm_per_agent(0.5)
    assert norms.shape == (nets.A,)
    opt.step()
    for k, p in nets.P.items():
        for g in range(nets.A):
            ref = torch.from_numpy(c[f'{algo}.a.{g}.{k}'])
            assert torch.allclose(p.detach()[g].cpu(), ref, rtol=0, atol=1e-6), (algo, g, k)


@pytest.mark.parametrize('algo', ['seac', 'iac'])
@pytest.mark.parametrize('i', CASES)
def test_clip_and_rmsprop_step_match_reference(i, algo):
    c, nets = load_case(np.load(GOLD), i)
    check_step(c, nets, algo)


def test_fixture_importance_weights_spread():
    z = np.load(GOLD)
    for i in (0, 1):
        lo, hi = z[f's{i}.iw_range']
        assert lo < 0.5 and hi > 2.0
    assert np.allclose(z['s2.iw_range'], 1.0, atol=1e-6)


def test_identical_networks_make_seac_terms_the_a2c_terms():
    """s2: iw == 1 everywhere, so every network's policy and value terms are the IAC terms over all rows."""
    c, nets = load_case(np.load(GOLD), 2)
    with torch.no_grad():
        sp, sv, se = torch_loss(c, nets, 'seac', terms=True)
        ip, iv, ie = torch_loss(c, nets, 'iac', terms=True)
    for j in range(nets.A):
        assert abs(float(sp[j]) - float(ip.mean())) <= 1e-6
        assert abs(float(sv[j]) - float(iv.mean())) <= 1e-6
        assert abs(float(se[j]) - float(ie[j])) <= 1e-6  # the entropy stays the network's own agent's


def _hetero(seed=0):
    torch.manual_seed(seed)
    return AgentNets(75, [4, 10, 9, 14], 10, 3, 7, 5, 4)


def test_state_dict_round_trip_is_bit_equal():
    nets = _hetero()
    mods = nets.to_modules()
    assert [m.n_actions for m in mods] == [4, 10, 9, 14]
    assert all(isinstance(m, RecurrentAC) for m in mods)
    back = AgentNets.from_modules(mods)
    for k, p in nets.P.items():
        assert torch.equal(p, back.P[k]), k
    fresh = _hetero(seed=5)
    fresh.load_state_dicts(nets.state_dicts())
    for k, p in nets.P.items():
        assert torch.equal(p, fresh.P[k]), k
    n, T = 5, 4
    g = torch.Generator().manual_seed(1)
    emb = torch.randn((4, n, T, 10), generator=g)
    acts = torch.randint(-1, 4, (4, n, T), generator=g)
    ha, hc = torch.randn((4, n, 7), generator=g), torch.randn((4, n, 5), generator=g)
    starts = torch.rand((4, n, T), generator=g) < 0.3
    with torch.no_grad():
        out = nets.forward_emb(emb, acts, ha, hc, starts=starts)
        for a, m in enumerate(mods):
            ref = m.forward_emb(emb[a], acts[a], ha[a][:, None], hc[a][:, None], starts=starts[a])
            assert torch.equal(out['logits'][a][..., :m.n_actions], ref['logits'])
            assert bool((out['logits'][a][..., m.n_actions:] == 0).all())
            assert torch.equal(out['critic'][a], ref['critic'])
            assert torch.equal(out['hidden_actor'][a], ref['hidden_actor'])
            assert torch.equal(out['hidden_critic'][a], ref['hidden_critic'])


def test_padded_action_heads_get_no_gradient():
    nets = _hetero()
    mods = nets.to_modules()
    A, B, T = 4, 3, 4
    g = torch.Generator().manual_seed(2)
    emb = torch.randn((A, B, T + 1, 10), generator=g)
    acts = torch.stack([torch.randint(0, n, (B, T + 1), generator=g) for n in nets.n_act])
    rew, done = torch.randn((A, B, T), generator=g), (torch.rand((A, B, T), generator=g) < 0.2).float()
    ha, hc = torch.zeros(A, B, 7), torch.zeros(A, B, 5)
    out = nets.forward_emb(emb, acts, ha, hc)
    loss = iac_loss_terms(out['logits'][:, :, :-1], out['critic'], acts[:, :, 1:], rew, done, 0.99, 0.01, 0.5, 0.95,
                          n_act=nets.n_act)
    loss.sum().backward()
    P = nets.P
    for a, n in enumerate(nets.n_act):
        assert bool((P['action_head.2.weight'].grad[a, n:] == 0).all())
        assert bool((P['action_head.2.bias'].grad[a, n:] == 0).all())
        assert bool((P['action_emb.weight'].grad[a, n + 1:] == 0).all())
        assert bool((P['action_emb.weight'].grad[a, 0] == 0).all())  # the padding row
        assert bool((P['action_head.2.weight'].grad[a, :n] != 0).any())
        # every agent's loss is the shared-network A2C loss of its own module on its own rows
        o = mods[a].forward_emb(emb[a], acts[a], ha[a][:, None], hc[a][:, None])
        ref = a2c_loss_terms(o['logits'][:, :-1], o['critic'], acts[a], rew[a], done[a], 0.99, 0.01, 0.5, 0.95)
        assert abs(float(loss[a].detach()) - float(ref.detach())) <= 1e-6
    with pytest.raises(ValueError, match='use_agent_embedding'):
        AgentNets(75, 4, 10, 3, 7, 5, 2, use_agent_embedding=True)


# ---------------------------------------------------------------------------------------------------------------------
# the loop, on the scripted engine (tests/scripted.py)
# ---------------------------------------------------------------------------------------------------------------------
class _ScriptedPacked(ScriptedEngine):
    """The scripted engine rendering packed entries only: the per-agent learners build PackedObs without the fused
    projection."""

    def _render(self, obs):
        assert obs.emb is None and obs.wt is None
        super()._render(obs)


def _scripted(cls, n_actions=(4, 4), **kw):
    eng = _ScriptedPacked()
    f = factory(eng, n_actions)
    args = dict(n_steps=3, cap=2, obs_emb_size=6, action_emb_size=4, hidden_size=5,
                generator=torch.Generator().manual_seed(0))
    args.update(kw)
    torch.manual_seed(0)
    return eng, cls(f, **args)


@pytest.mark.parametrize('cls,n_actions', [(BatchedIAC, (4, 4)), (BatchedIAC, (3, 5)), (BatchedSEAC, (4, 4))])
def test_window_alignment_on_the_scripted_engine(cls, n_actions):
    eng, tr = _scripted(cls, n_actions)
    A, B, T = tr.A, tr.B, tr.T
    acting, windows = [], []
    sample, learn = tr._sample, tr.learn

    def spy_sample(logits, t):
        acting.append(logits.clone())
        sample(logits, t)

    def spy_learn():
        k0 = eng.k - T  # the step that rendered entry 0 of this window
        for s in range(T + 1):
            assert torch.equal(tr.pobs.val[s, :, :, 0], eng.code(k0 + s))
        for s in range(T):
            assert torch.equal(tr.rew[s], eng.code(k0 + s + 1).double() + 0.5)
            d = (k0 + s + 1 + 3 * torch.arange(B)) % eng.period == 0
            assert torch.equal(tr.done[s].bool(), d)
            want = torch.where(d.view(-1, 1), torch.full((B, A), -1), tr.act[s].long())
            assert torch.equal(tr.act_in[s + 1], want)
            for a, n in enumerate(n_actions):
                assert bool(((tr.act[s, :, a] >= 0) & (tr.act[s, :, a] < n)).all())
        # no weight has changed since the window's first step: the learner's forward reproduces the acting logits
        with torch.no_grad():
            lg = tr.evaluate()['logits']
        if tr.cross:
            lg = torch.stack([lg.view(A, A, B, T + 1, -1)[a, a] for a in range(A)])
        assert torch.allclose(lg[:, :, :T], torch.stack(acting[-T:], 2), rtol=1e-4, atol=1e-5)
        w0 = [p.detach().clone() for p in tr.nets.agent_params()]
        learn()
        windows.append(1)
        assert bool(torch.isfinite(tr.last_loss).all()) and tr.last_loss.shape == (A,)
        for a in range(A):  # every agent's network moved
            assert any(not torch.equal(p0[a], p.detach()[a]) for p0, p in zip(w0, tr.nets.agent_params()))
        assert torch.equal(tr.pobs.val[0], tr.pobs.val[T]) and torch.equal(tr.act_in[0], tr.act_in[T])

    tr._sample, tr.learn = spy_sample, spy_learn
    tr.train(4)
    assert len(windows) == 4 and tr.updates == 4
    assert eng.defer == [True, True, False] * 4  # the replay is deferred to the window's last step
    ks = range(1, 4 * T + 1)
    assert float(tr.episodes) == float(sum((k + 3 * b) % eng.period == 0 for k in ks for b in range(B)))
    assert float(tr.reward_sum) == float(sum((eng.code(k).double() + 0.5).sum() for k in ks))


def test_constructor_errors():
    with pytest.raises(ValueError, match='same number of actions'):
        _scripted(BatchedSEAC, (4, 5))
    _scripted(BatchedIAC, (4, 5))  # independent networks take different counts
    f = factory(_ScriptedPacked(), [4, 5])
    with pytest.raises(ValueError, match='same number of actions'):
        BatchedA2C(f)  # the shared-network learner still refuses such a team
    with pytest.raises(ValueError, match='use_agent_embedding'):
        _scripted(BatchedIAC, use_agent_embedding=True)
    with pytest.raises(ValueError, match='check_cap'):
        _scripted(BatchedIAC, check_cap=False, cap=2)


def test_activation_bytes_scale_with_the_networks():
    _, iac = _scripted(BatchedIAC)
    _, seac = _scripted(BatchedSEAC)
    assert iac.activation_bytes() > 0
    assert seac.activation_bytes() == iac.A * iac.activation_bytes()
