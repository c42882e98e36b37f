"""Shared by tests/test_eval.py and tests/test_gpu_eval.py: the evaluator fixture (tests/golden/marl_eval.npz,
tools/gen_golden_eval.py), a plain numpy float32 statement of eval_loop's bookkeeping (base_ac.py:160-177), and a
stand-in engine that replays recorded rewards and done flags."""
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import torch

GOLD = Path(__file__).resolve().parent / 'golden' / 'marl_eval.npz'
CASES = ('snac', 'iac')


def load_case(tag):
    z = np.load(GOLD)
    return {k[len(tag) + 1:]: z[k] for k in z.files if k.startswith(tag + '.')}


def case_states(c):
    """The fixture's state dicts, one per network."""
    n = 1 + max(int(k.split('.')[1]) for k in c if k.startswith('w.'))
    return [{k.split('.', 2)[2]: torch.from_numpy(v) for k, v in c.items() if k.startswith(f'w.{g}.')} for g in range(n)]


def case_policy(c):
    """The fixture's networks: a RecurrentAC (one state dict) or an AgentNets."""
    from mfg_amd.marl import AgentNets, RecurrentAC
    mods = []
    for st in case_states(c):
        m = RecurrentAC(observation_size=c['obs0'].shape[1:], n_actions=int(c['n_actions']),
                        obs_emb_size=st['obs_proj.weight'].shape[0], action_emb_size=st['action_emb.weight'].shape[1],
                        hidden_size_actor=st['gru_actor.weight_hh_l0'].shape[1],
                        hidden_size_critic=st['gru_critic.weight_hh_l0'].shape[1], n_agents=int(c['n_agents']),
                        use_agent_embedding=False)
        m.load_state_dict(st)
        mods.append(m)
    return mods[0] if len(mods) == 1 else AgentNets.from_modules(mods)


def fold_loop(rewards, dones, n_episodes):
    """rewards [steps, B, A] (f64), dones [steps, B] -> (rows f32 [B, n_episodes, A + 1], lengths i32 [B, n_episodes]):
    eps_rew (f32) += f32(reward) per step; at a done the agents' sums, then ((0 + e_0) + e_1) + ... in f32."""
    rewards, dones = np.asarray(rewards, dtype=np.float64), np.asarray(dones)
    steps, B, A = rewards.shape
    rows = np.zeros((B, n_episodes, A + 1), np.float32)
    lengths = np.zeros((B, n_episodes), np.int32)
    for b in range(B):
        e, n, k = np.zeros(A, np.float32), 0, 0
        for t in range(steps):
            e = (e + rewards[t, b].astype(np.float32)).astype(np.float32)
            n += 1
            if dones[t, b]:
                if k < n_episodes:
                    s = np.float32(0.0)
                    for i in range(A):
                        s = np.float32(s + e[i])
                    rows[b, k, :A], rows[b, k, A], lengths[b, k] = e, s, n
                    k += 1
                e, n = np.zeros(A, np.float32), 0
    return rows, lengths


def frame_rows(c):
    """The reference frame's values as rows [n_episodes, A + 1] (f64), from its melted columns."""
    out = np.zeros((int(c['n_episodes']), int(c['n_agents']) + 1), np.float64)
    out[c['frame_episode'], c['frame_agent']] = c['frame_reward']
    return out


class ReplayEngine:
    """Stands in for mfg_amd.engine.Engine on the CPU: step k hands out rewards[k] / dones[k] ([steps, B, A] /
    [steps, B]) whatever the actions, renders one packed entry per row, and records the actions it was given."""

    def __init__(self, rewards, dones, lmax=1, obs_hw=(2, 2)):
        self.torch = torch
        self.rewards, self.dones = torch.as_tensor(rewards, dtype=torch.float64), torch.as_tensor(dones).to(torch.uint8)
        self.B, self.A = self.rewards.shape[1:]
        self.device = torch.device('cpu')
        self.lmax, self.obs_hw = lmax, obs_hw
        self.k = 0
        self.seen = []

    def _render(self, obs):
        obs.idx[0].zero_()
        obs.val[0].zero_()
        obs.idx[0, :, :, 0] = (torch.arange(self.A) % 4).to(torch.uint16)
        obs.val[0, :, :, 0] = float(self.k % 5 + 1)
        obs.count[0].fill_(1)
        if obs.emb is not None:
            obs.emb[0].copy_(obs.bias + obs.val[0, :, :, :1] * obs.wt[torch.arange(self.A) % 4][None])

    def reset(self, obs=None, init=False, seed_base=0):
        self.k = 0
        self.seen = []
        self._render(obs)

    def step(self, K, actions=None, reward=None, done=None, obs=None, auto_reset=True, step_base=0):
        assert K == 1 and auto_reset
        self.seen.append(actions.clone())
        reward.copy_(self.rewards[self.k])
        done.copy_(self.dones[self.k])
        self.k += 1
        self._render(obs)


def fake_factory(engine, n_actions):
    return SimpleNamespace(engine=engine, spec=SimpleNamespace(n_actions=[n_actions] * engine.A), _created=False,
                           seed_base=0, t=0)
