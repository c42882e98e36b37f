#!/usr/bin/env python3
"""Golden vectors for the per-agent-network learners (mfg_amd.marl.BatchedIAC / BatchedSEAC): runs the REFERENCE
networks and losses (algorithms/marl/networks.py RecurrentAC, algorithms/marl/seac.py LoopSEAC.actor_critic,
algorithms/marl/base_ac.py BaseActorCritic.actor_critic as iac.py:50-57 calls it per agent) on small synthetic windows
and stores inputs, per-network weights, losses, gradients and the weights after clip_grad_norm_(0.5) per network + one
RMSprop(3e-4, eps 1e-5) step (iac.py:18-20,53-57; seac.py:49-54).

It needs a checkout of the reference project (read only), named by the MFG_REFERENCE environment variable:
    MFG_REFERENCE=/path/to/marl-factory-grid python tools/gen_golden_seac.py
Output: tests/golden/marl_seac.npz (data only). tests/test_seac.py and tests/test_gpu_seac.py replay it.

The reference runs one env. Every case holds B = 2 "envs": the reference runs twice on different data, from the same
weights, and the stored loss is the mean of both runs (so are the gradients: one backward of the mean).

Cases (T = 5, 10 actions):
  s0  A = 3, gae_coef 0, no dones
  s1  A = 3, gae_coef 0.95, dones on a row's first step, on another row's last step, and two in one row
  s2  A = 2 networks with identical weights, gae_coef 0.95, one done: every importance weight is 1
Each network's last action-head layer is drawn from N(0, 1), so that the off-diagonal importance weights spread:
asserted to reach below 0.5 and above 2 in s0 and s1.
"""
import os
import sys
import types
from pathlib import Path

import numpy as np
import torch

REPO = Path(__file__).resolve().parent.parent
if 'MFG_REFERENCE' not in os.environ:
    raise SystemExit('set MFG_REFERENCE to a checkout of the reference project')
sys.path[:0] = [str(REPO / 'tools' / 'standins'), os.environ['MFG_REFERENCE']]

from marl_factory_grid.algorithms.marl.networks import RecurrentAC  # noqa: E402
from marl_factory_grid.algorithms.marl.base_ac import BaseActorCritic  # noqa: E402
from marl_factory_grid.algorithms.marl.seac import LoopSEAC  # noqa: E402

VALUES = np.array([1.0, 2.0, 0.6666, 0.4444, 0.37, 3.0])
HYPER = dict(gamma=0.99, entropy_coef=0.01, vf_coef=0.5)
T, L, D, N_ACTIONS, B = 5, 3, 5, 10, 2
EMB, AEMB, HA, HC = 12, 4, 8, 12  # small layers: the file holds five copies of every network


def make_nets(seed, A, identical):
    torch.manual_seed(seed)
    nets = []
    for g in range(A):
        net = RecurrentAC(observation_size=(L, D, D), n_actions=N_ACTIONS, obs_emb_size=EMB, action_emb_size=AEMB,
                          hidden_size_actor=HA, hidden_size_critic=HC, n_agents=A, use_agent_embedding=False)
        with torch.no_grad():
            net.action_head[2].weight.normal_(0.0, 1.0)
        if identical and g:
            net.load_state_dict(nets[0].state_dict())
        nets.append(net)
    return nets


def memory(obs, actions, reward, done, ha, hc, rows):
    """What actor_critic reads of a memory: [rows, T+1, ...] tensors whose reward / done carry a leading dummy entry."""
    pad = np.zeros((len(rows), 1), dtype=np.float32)
    return types.SimpleNamespace(
        observation=torch.from_numpy(obs[rows]), action=torch.from_numpy(actions[rows]),
        reward=torch.from_numpy(np.concatenate([pad, reward[rows]], 1)),
        done=torch.from_numpy(np.concatenate([pad, done[rows]], 1)),
        hidden_actor=torch.from_numpy(ha[rows])[:, None], hidden_critic=torch.from_numpy(hc[rows])[:, None])


def snapshot(nets, losses):
    """Per network: backward of its loss, the gradients, then clip + one RMSprop step; restores nothing."""
    out = []
    for net, loss in zip(nets, losses):
        opt = torch.optim.RMSprop(net.parameters(), lr=3e-4, eps=1e-5)  # iac.py:18-20
        opt.zero_grad()
        loss.backward()
        grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().numpy().copy()
                 for k, p in net.named_parameters()}
        torch.nn.utils.clip_grad_norm_(net.parameters(), 0.5)
        opt.step()
        out.append((float(loss.item()), grads, {k: p.detach().numpy().copy() for k, p in net.named_parameters()}))
    return out


def case(seed, A, gae_coef, dones, identical=False, need_iw=False):
    rng = np.random.default_rng(seed)
    obs = np.zeros((A, B, T + 1, L, D, D))
    mask = rng.random(obs.shape) < 0.06
    obs[mask] = rng.choice(VALUES, mask.sum())
    actions = rng.integers(0, N_ACTIONS, (A, B, T + 1))
    actions[:, :, 0] = rng.choice([-1, 3], (A, B))
    reward = rng.normal(0, 0.3, (A, B, T)).astype(np.float32)
    done = np.zeros((A, B, T), dtype=np.float32)
    if dones == 'many':
        done[0, 0, 0] = done[1, 0, T - 1] = 1.0  # a row's first step, another row's last
        done[2, 1, 1] = done[2, 1, 3] = 1.0  # two in one row
    elif dones == 'one':
        done[1, 1, 2] = 1.0
    ha = rng.normal(0, 0.5, (A, B, 1, HA)).astype(np.float32)
    hc = rng.normal(0, 0.5, (A, B, 1, HC)).astype(np.float32)
    state = [{k: v.detach().numpy().copy() for k, v in n.state_dict().items()} for n in make_nets(seed, A, identical)]
    owner = types.SimpleNamespace(compute_advantages=BaseActorCritic.compute_advantages)
    hyper = dict(HYPER, gae_coef=gae_coef)
    res = {}
    iw_lo, iw_hi = np.inf, 0.0
    for algo in ('seac', 'iac'):
        nets = make_nets(seed, A, identical)
        runs = []
        for b in range(B):
            sel = lambda x: x[:, b]  # noqa: E731
            if algo == 'seac':
                tm = memory(sel(obs), sel(actions), sel(reward), sel(done), sel(ha), sel(hc), list(range(A)))
                runs.append(LoopSEAC.actor_critic(owner, tm, nets, **hyper))
                with torch.no_grad():  # the importance weights' spread (the reference's own quantities)
                    outs = [n(tm.observation, tm.action, tm.hidden_actor[:, 0], tm.hidden_critic[:, 0]) for n in nets]
                    lp = torch.stack([torch.log_softmax(o['logits'][:, :-1], -1).gather(
                        -1, tm.action[:, 1:, None]).squeeze(-1) for o in outs])  # [net, agent, T]
                    for j in range(A):
                        for i in range(A):
                            if i != j:
                                iw = (lp[j, i] - lp[i, i]).exp()
                                iw_lo, iw_hi = min(iw_lo, float(iw.min())), max(iw_hi, float(iw.max()))
            else:
                runs.append([BaseActorCritic.actor_critic(
                    owner, memory(sel(obs), sel(actions), sel(reward), sel(done), sel(ha), sel(hc), [g]), nets[g],
                    **hyper) for g in range(A)])
        losses = [sum(r[g] for r in runs) / B for g in range(A)]
        for g, (loss, grads, after) in enumerate(snapshot(nets, losses)):
            res[f'{algo}.loss.{g}'] = np.float64(loss)
            for k, v in grads.items():
                res[f'{algo}.g.{g}.{k}'] = v
            for k, v in after.items():
                res[f'{algo}.a.{g}.{k}'] = v
    if need_iw:
        assert iw_lo < 0.5 and iw_hi > 2.0, f'importance-weight coverage: {iw_lo} .. {iw_hi}'
    if identical:
        assert abs(iw_lo - 1.0) < 1e-6 and abs(iw_hi - 1.0) < 1e-6
    res.update(obs=obs, actions=actions, reward=reward, done=done, ha0=ha[:, :, 0], hc0=hc[:, :, 0],
               n_actions=np.int32(N_ACTIONS), n_agents=np.int32(A), gae_coef=np.float64(gae_coef),
               iw_range=np.array([iw_lo, iw_hi]))
    for k, v in HYPER.items():
        res[k] = np.float64(v)
    for g, st in enumerate(state):
        for k, v in st.items():
            res[f'w.{g}.{k}'] = v
    print(f'seed {seed}: A {A} gae {gae_coef} iw {iw_lo:.3f} .. {iw_hi:.3f} '
          f'seac {[round(float(res[f"seac.loss.{g}"]), 5) for g in range(A)]}')
    return res


def main():
    out = {}
    cases = [dict(seed=0, A=3, gae_coef=0.0, dones='none', need_iw=True),
             dict(seed=1, A=3, gae_coef=0.95, dones='many', need_iw=True),
             dict(seed=2, A=2, gae_coef=0.95, dones='one', identical=True)]
    for i, kw in enumerate(cases):
        for k, v in case(**kw).items():
            out[f's{i}.{k}'] = v
    dst = REPO / 'tests' / 'golden' / 'marl_seac.npz'
    np.savez_compressed(dst, **out)
    print('wrote', dst, dst.stat().st_size, 'bytes')


if __name__ == '__main__':
    main()
