#!/usr/bin/env python3
"""Golden vectors for the MAPPO learner (mfg_amd.marl.BatchedMAPPO): runs the REFERENCE network, loss and chunk
whitelist (algorithms/marl/networks.py RecurrentAC, algorithms/marl/mappo.py LoopMAPPO.mappo + monte_carlo_returns,
algorithms/marl/memory.py ExperienceChunks.whitelist) on small synthetic batches and stores inputs, weights, returns,
loss, gradients and the weights after clip_grad_norm_(0.5) + one Adam(3e-4, eps 1e-5) step (mappo.py:14-28).

It needs a checkout of the reference project (read only), named by the MFG_REFERENCE environment variable:
    MFG_REFERENCE=/path/to/marl-factory-grid python tools/gen_golden_mappo.py
Output: tests/golden/marl_mappo.npz (data only). tests/test_mappo.py and tests/test_gpu_mappo.py replay it through mfg_amd.marl.

Cases (6 or 12 rows, T = 5, 10 actions):
  c0  old logits = a no-grad forward of the same network: every element sits in the tie surr1 == surr2
  c1  perturbed old logits: both clip sides bind, each with positive and negative advantages (asserted)
  c2  done flags, one on the first and one on the last step of a row
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
from marl_factory_grid.algorithms.marl.mappo import LoopMAPPO  # noqa: E402
from marl_factory_grid.algorithms.marl.memory import ExperienceChunks  # noqa: E402

VALUES = np.array([1.0, 2.0, 0.6666, 0.4444, 0.37, 3.0])
HYPER = dict(gamma=0.99, entropy_coef=0.01, vf_coef=0.5, clip_range=0.2)


def case(seed, old, dones, N=6):
    rng = np.random.default_rng(seed)
    T, L, d, n_actions = 5, 4, 5, 10
    obs = np.zeros((N, T + 1, L, d, d))
    mask = rng.random(obs.shape) < 0.06
    obs[mask] = rng.choice(VALUES, mask.sum())
    actions = rng.integers(0, n_actions, (N, T + 1))
    actions[:, 0] = rng.choice([-1, 3], N)
    reward = rng.normal(0, 0.3, (N, T)).astype(np.float32)
    done = np.zeros((N, T), dtype=np.float32)
    if dones:
        done[0, 0] = done[1, T - 1] = done[2, 2] = 1.0
        done[3, 0] = done[3, T - 1] = 1.0
    ha = rng.normal(0, 0.5, (N, 1, 16)).astype(np.float32)
    hc = rng.normal(0, 0.5, (N, 1, 24)).astype(np.float32)
    torch.manual_seed(seed)
    net = RecurrentAC(observation_size=(L, d, d), n_actions=n_actions, obs_emb_size=24, action_emb_size=8,
                      hidden_size_actor=16, hidden_size_critic=24, n_agents=N, use_agent_embedding=False)
    state = {k: v.detach().numpy().copy() for k, v in net.state_dict().items()}
    t_obs, t_act = torch.from_numpy(obs), torch.from_numpy(actions)
    t_ha, t_hc = torch.from_numpy(ha), torch.from_numpy(hc)
    with torch.no_grad():
        fwd = net(t_obs, t_act, t_ha, t_hc)
    own = fwd['logits'][:, :-1].clone()
    if old == 'own':
        old_logits = own
    else:
        old_logits = own + torch.from_numpy(rng.normal(0, old, own.shape).astype(np.float32))
    batch = dict(observation=t_obs, action=t_act, hidden_actor=t_ha, hidden_critic=t_hc,
                 reward=torch.from_numpy(reward), done=torch.from_numpy(done), logits=old_logits)
    owner = types.SimpleNamespace()
    owner.monte_carlo_returns = types.MethodType(LoopMAPPO.monte_carlo_returns, owner)
    returns = LoopMAPPO.monte_carlo_returns(owner, batch['reward'], batch['done'], HYPER['gamma'])
    if old != 'own' and not dones:
        # both clip sides must bind with both advantage signs (the reference's own quantities, no grad)
        with torch.no_grad():
            idx = t_act[:, 1:].unsqueeze(-1)
            ratio = (torch.log_softmax(own, -1).gather(-1, idx) - torch.log_softmax(old_logits, -1).gather(-1, idx)
                     ).squeeze(-1).exp()
            rn = (returns - returns.mean()) / (returns.std() + 1e-8)
            adv = rn - fwd['critic'][:, :-1]
            c = HYPER['clip_range']
            for side in (ratio > 1 + c, ratio < 1 - c):
                assert bool((side & (adv > 0)).any()) and bool((side & (adv < 0)).any()), 'clip coverage'
    loss = LoopMAPPO.mappo(owner, batch, net, **HYPER)
    opt = torch.optim.Adam(net.parameters(), lr=3e-4, eps=1e-5)  # mappo.py:16
    opt.zero_grad()
    loss.backward()
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().numpy().copy()
             for k, p in net.named_parameters()}
    torch.nn.utils.clip_grad_norm_(net.parameters(), 0.5)  # mappo.py:27
    opt.step()
    after = {k: p.detach().numpy().copy() for k, p in net.named_parameters()}
    out = {'obs': obs, 'actions': actions, 'reward': reward, 'done': done, 'ha0': ha, 'hc0': hc,
           'old_logits': old_logits.numpy().copy(), 'returns': returns.numpy().copy(),
           'loss': np.float64(loss.item()), 'n_actions': np.int32(n_actions)}
    for k, v in HYPER.items():
        out[k] = np.float64(v)
    for k, v in state.items():
        out['w.' + k] = v
    for k, v in grads.items():
        out['g.' + k] = v
    for k, v in after.items():
        out['a.' + k] = v
    return out


class _Memory:
    """What ExperienceChunks.whitelist reads of an ActorCriticMemory: the done flags [1, S] and the length."""

    def __init__(self, done):
        self.done = torch.from_numpy(done).float().unsqueeze(0)

    def __len__(self):
        return self.done.shape[1]


def whitelists():
    rng = np.random.default_rng(7)
    pats = []
    for S in (8, 12, 16):
        z = np.zeros(S, dtype=np.float32)
        first, last, both = z.copy(), z.copy(), z.copy()
        first[0] = last[-1] = both[0] = both[-1] = 1
        pats += [z, first, last, both]
    adj = np.zeros(12, dtype=np.float32)
    adj[5] = adj[6] = 1
    pats += [np.ones(8, dtype=np.float32), adj]
    for S, p in ((12, 0.1), (12, 0.3), (16, 0.1), (16, 0.2), (16, 0.5), (9, 0.2)):
        pats.append((rng.random(S) < p).astype(np.float32))
    out = {'wl.n': np.int32(len(pats))}
    for i, d in enumerate(pats):
        out[f'wl.{i}.done'] = d
        for cl in (1, 3, 5):
            wl = ExperienceChunks(_Memory(d), cl, 1).whitelist
            out[f'wl.{i}.cl{cl}'] = np.asarray(wl, dtype=np.float32)
    return out


def main():
    res = {}
    for i, (seed, old, dones, rows) in enumerate([(0, 'own', False, 6), (1, 1.0, False, 12), (2, 0.1, True, 6)]):
        for k, v in case(seed, old, dones, rows).items():
            res[f'c{i}.{k}'] = v
    res.update(whitelists())
    dst = REPO / 'tests' / 'golden' / 'marl_mappo.npz'
    np.savez_compressed(dst, **res)
    print('wrote', dst, dst.stat().st_size, 'bytes')


if __name__ == '__main__':
    main()
