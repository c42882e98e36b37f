"""Host side of the action masks (mfg_amd/action_mask.py, evaluate.sample_inversion / BatchedEvaluator._pick, the
adapters' opt-in): CPU only."""
import numpy as np
import torch

import mfg_amd.evaluate as EV
from mfg_amd.action_mask import agent_masks, dense_mask, masked_logits


def _words(gen, shape, n):
    """Random words with bits only below n, as the int32 tensors the engine hands out."""
    bits = torch.rand(shape + (n,), generator=gen) < 0.5
    w = (bits.long() << torch.arange(n)).sum(-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32), bits


def test_dense_expansion():
    gen = torch.Generator().manual_seed(0)
    for n in (1, 5, 31, 32):
        w, bits = _words(gen, (6, 3), n)
        assert torch.equal(dense_mask(w, n), bits)
        assert np.array_equal(dense_mask(w.numpy(), n), bits.numpy())
    # bit 31 travels as the sign bit
    w = torch.tensor([[-2 ** 31, -1, 0, 5]], dtype=torch.int32)
    d = dense_mask(w, 32)
    assert d[0, 0].tolist() == [False] * 31 + [True] and bool(d[0, 1].all()) and not bool(d[0, 2].any())
    assert d[0, 3].nonzero().flatten().tolist() == [0, 2]
    # columns past the word's bits are False; one array per agent of its own action count
    assert dense_mask(torch.tensor([3], dtype=torch.int32), 4).tolist() == [[True, True, False, False]]
    per_agent = agent_masks(np.array([5, 2, -1], np.int32), [3, 2, 32])
    assert [m.tolist() for m in per_agent[:2]] == [[True, False, True], [False, True]]
    assert per_agent[2].dtype == bool and per_agent[2].shape == (32,) and per_agent[2].all()


def test_sample_inversion_mask_is_minus_inf_fill():
    gen = torch.Generator().manual_seed(1)
    for n_max, n_act in ((11, 11), (11, 6), (32, 32), (1, 1)):
        logits = torch.randn((40, 3, n_max), generator=gen)
        u = torch.rand((40, 3), generator=gen)
        w, bits = _words(gen, (40, 3), n_max)
        bits = bits[..., :n_act]
        w[0, 0] = 0  # an all-zero row: unmasked
        bits[0, 0] = True
        w[1, 1] = -1  # every bit: unmasked as well
        bits[1, 1] = True
        empty = ~bits.any(-1)  # a word with bits only at or past n_act: unmasked
        filled = torch.where(bits | empty[..., None], logits[..., :n_act], torch.tensor(float('-inf')))
        got = EV.sample_inversion(logits, u, n_act, mask=w)
        assert torch.equal(got, EV.sample_inversion(filled, u))
        assert torch.equal(masked_logits(logits[..., :n_act], w), filled)
        plain = EV.sample_inversion(logits, u, n_act)
        assert int(got[0, 0]) == int(plain[0, 0]) and int(got[1, 1]) == int(plain[1, 1])
        assert torch.equal(got[empty], plain[empty])
        # a masked pick is a set bit wherever the row has one
        has = ~empty
        assert bool(torch.gather(bits, -1, got.long()[..., None])[..., 0][has].all())
    zero = torch.zeros((40, 3), dtype=torch.int32)
    assert torch.equal(EV.sample_inversion(logits, u, mask=zero), EV.sample_inversion(logits, u))


class _Pick:
    """BatchedEvaluator._pick alone, on the CPU."""
    _pick = EV.BatchedEvaluator._pick

    def __init__(self, n_act, B, greedy):
        self.n_act, self.A, self.B, self.N, self.greedy = n_act, len(n_act), B, B * len(n_act), greedy
        self.act = torch.zeros((B, self.A), dtype=torch.int32)
        self.dev = torch.device('cpu')


def test_evaluator_pick_with_a_mask():
    gen = torch.Generator().manual_seed(2)
    for n_act in ([7, 7, 7], [7, 4, 1]):
        B, n_max = 50, max(n_act)
        logits = torch.randn((B, len(n_act), n_max), generator=gen)
        u = torch.rand((B, len(n_act)), generator=gen)
        w, bits = _words(gen, (B, len(n_act)), n_max)
        w[3] = 0
        for greedy in (False, True):
            p, q = _Pick(n_act, B, greedy), _Pick(n_act, B, greedy)
            p._pick(logits, u, w)
            q._pick(logits, u)
            assert torch.equal(p.act[3], q.act[3])  # all-zero rows: the unmasked pick
            for i, n in enumerate(n_act):
                d = dense_mask(w[:, i], n)
                has = d.any(-1)
                assert bool(torch.gather(d, -1, p.act[:, i].long()[:, None])[:, 0][has].all())
                assert torch.equal(p.act[:, i][~has], q.act[:, i][~has])
                if greedy:  # the lowest-index argmax over the set bits
                    f = torch.where(d, logits[:, i, :n], torch.tensor(float('-inf')))
                    assert torch.equal(p.act[:, i][has], f.argmax(-1).to(torch.int32)[has])
            assert int(p.act.min()) >= 0


# ---- the adapters' opt-in ----
class _Spec:
    n_agents, d = 2, 3
    obs_hw = (3, 3)
    n_layers = [2, 2]
    n_actions = [5, 3]
    agent_names = ['a0', 'a1']
    rules = []


class _Batched:
    """BatchedFactory's I/O contract with a fixed mask."""

    def __init__(self, B=3):
        self.torch, self.B, self.device, self.seed_base, self._created, self.spec = torch, B, torch.device('cpu'), 0, False, _Spec
        self.mask_calls = 0

    def reset(self, mask=None):
        self._created = True
        return torch.zeros((self.B, 2, 2, 3, 3))

    def step(self, actions):
        ev_misc = torch.zeros((self.B, 16), dtype=torch.int32)
        return (torch.zeros((self.B, 2, 2, 3, 3)), torch.zeros((self.B, 2), dtype=torch.float64),
                torch.zeros(self.B, dtype=torch.uint8), (None, None, ev_misc))

    def action_mask(self, dense=False):
        self.mask_calls += 1
        w = torch.tensor([[21, 5]] * self.B, dtype=torch.int32)
        return dense_mask(w, 5) if dense else w

    def close(self):
        pass


def test_vector_and_sb3_opt_in():
    from mfg_amd.vec import SB3VecFactory, VectorFactory
    env = _Batched()
    v = VectorFactory(None, None, env=env)
    _, infos = v.reset()
    assert infos == {}
    assert 'action_mask' not in v.step(torch.zeros((3, 2), dtype=torch.int32))[4] and env.mask_calls == 0
    v = VectorFactory(None, None, env=env, action_mask=True)
    _, infos = v.reset()
    assert infos['action_mask'].tolist() == [[21, 5]] * 3
    infos = v.step(torch.zeros((3, 2), dtype=torch.int32))[4]
    assert infos['action_mask'].dtype == torch.int32 and infos['action_mask'].shape == (3, 2) and env.mask_calls == 2
    s = SB3VecFactory(None, None, venv=VectorFactory(None, None, env=env))
    s.reset()
    m = s.action_masks()
    assert m.dtype == bool and m.shape == (3, 8)
    assert m[0].tolist() == [True, False, True, False, True] + [True, False, True]


class _Single:
    """Factory's contract for ParallelFactory."""
    spec = _Spec

    def reset(self):
        return {'Agent[a0]': np.zeros((2, 3, 3)), 'Agent[a1]': np.zeros((2, 3, 3))}

    def step(self, acts):
        return None, [np.zeros((2, 3, 3))] * 2, [0.0, 0.0], False, {'step': 1}

    _ev_m = torch.zeros((1, 16), dtype=torch.int32)

    def action_mask(self):
        return agent_masks(np.array([21, 5], np.int32), _Spec.n_actions)


def test_parallel_opt_in():
    from mfg_amd.vec import ParallelFactory
    acts = {'Agent[a0]': 0, 'Agent[a1]': 0}
    p = ParallelFactory(None, env=_Single())
    _, infos = p.reset()
    assert infos == {'Agent[a0]': {}, 'Agent[a1]': {}}
    assert all('action_mask' not in i for i in p.step(acts)[4].values())
    p = ParallelFactory(None, env=_Single(), action_mask=True)
    _, infos = p.reset()
    assert infos['Agent[a0]']['action_mask'].tolist() == [True, False, True, False, True]
    infos = p.step(acts)[4]
    assert infos['Agent[a1]']['action_mask'].tolist() == [True, False, True] and infos['Agent[a1]']['step'] == 1
