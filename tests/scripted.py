"""A scripted stand-in for mfg_amd.engine.Engine on the CPU, for the learners' loops (tests/test_marl.py,
tests/test_mappo.py, tests/test_seac.py, tests/test_eval.py): what every step renders, rewards and ends is a closed form
of the step number, so a test can say what each slot of a window or ring must hold. And ``pack``, the packed rows of a
dense observation.
"""
from types import SimpleNamespace

import torch


def pack(obs, cap):
    """Dense [N, T, ...] -> (idx u16, val f32) [N, T, cap] of the nonzero entries of obs.float()."""
    flat = torch.as_tensor(obs).reshape(obs.shape[0], obs.shape[1], -1).float()
    N, T, K = flat.shape
    idx = torch.zeros((N, T, cap), dtype=torch.uint16)
    val = torch.zeros((N, T, cap), dtype=torch.float32)
    for n in range(N):
        for t in range(T):
            nz = torch.nonzero(flat[n, t]).flatten()
            assert len(nz) <= cap
            idx[n, t, :len(nz)] = nz.to(torch.uint16)
            val[n, t, :len(nz)] = flat[n, t, nz]
    return idx, val


class ScriptedEngine:
    """Step k (0 = the reset) renders for env b, agent a the one packed entry (index a, value code(k, b, a)), rewards
    code + 0.5 and ends env b's episode when (k + 3 b) % period == 0. With a PackedObs that carries a projection the
    fused emb is rendered too. ``defer`` records the deferred-replay flag of every step."""

    def __init__(self, B=3, A=2, period=7):
        self.torch = torch
        self.B, self.A, self.period = B, A, period
        self.device = torch.device('cpu')
        self.lmax, self.obs_hw = 1, (2, 2)
        self.k = 0
        self.defer = []

    def code(self, k):
        b = torch.arange(self.B).view(-1, 1)
        a = torch.arange(self.A).view(1, -1)
        return (1000 * k + 10 * b + a + 1).float()

    def _render(self, obs):
        v = self.code(self.k)
        obs.idx[0].zero_()
        obs.val[0].zero_()
        obs.idx[0, :, :, 0] = torch.arange(self.A).to(torch.uint16)
        obs.val[0, :, :, 0] = v
        obs.count[0].fill_(1)
        if obs.wt is not None:
            obs.emb[0].copy_(obs.bias + v[..., None] * obs.wt[torch.arange(self.A)][None])

    def reset(self, obs=None, init=False, seed_base=0):
        self.k = 0
        self._render(obs)

    def step(self, K, actions=None, reward=None, done=None, obs=None, auto_reset=True, step_base=0,
             defer_replay=False):
        assert K == 1 and auto_reset
        self.defer.append(bool(defer_replay))
        self.k += 1
        reward.copy_(self.code(self.k).double() + 0.5)
        done.copy_(((self.k + 3 * torch.arange(self.B)) % self.period == 0).to(torch.uint8))
        self._render(obs)


def factory(eng, n_actions):
    """What the learners read of a BatchedFactory, around a scripted engine."""
    return SimpleNamespace(engine=eng, spec=SimpleNamespace(n_actions=list(n_actions)), _created=False, seed_base=0,
                           t=0)
