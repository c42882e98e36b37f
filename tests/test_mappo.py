"""The MAPPO learner on the CPU (mfg_amd/marl.py: monte_carlo_returns, mappo_loss, chunk_starts, BatchedMAPPO's ring).

Golden vectors from the reference's own network, loss and chunk whitelist (tests/golden/marl_mappo.npz,
tools/gen_golden_mappo.py: algorithms/marl/mappo.py LoopMAPPO.mappo + monte_carlo_returns, memory.py
ExperienceChunks.whitelist). The same f32 ops as the A2C replay (tests/test_marl.py) in another summation order: loss
within 1e-5 relative (+1e-7), gradients rtol 1e-4 / atol 1e-6. The optimiser step is pinned on the fixture's own
gradients (Adam's first step divides by |g| + eps, which amplifies gradient rounding where |g| ~ eps): weights within
1e-6 absolute.
"""
from pathlib import Path

import numpy as np
import pytest
import torch

from mfg_amd.marl import (BatchedMAPPO, RecurrentAC, chunk_starts, mappo_loss, monte_carlo_returns)
from scripted import ScriptedEngine, factory, pack  # noqa: F401 (pack: tests/test_gpu_mappo.py takes it from here)

GOLD = Path(__file__).resolve().parent / 'golden' / 'marl_mappo.npz'


def load_case(z, i, device='cpu'):
    c = {k.split('.', 1)[1]: z[k] for k in z.files if k.startswith(f'c{i}.')}
    st = {k[2:]: torch.from_numpy(v) for k, v in c.items() if k.startswith('w.')}
    net = RecurrentAC(observation_size=c['obs'].shape[2:], n_actions=int(c['n_actions']),
                      obs_emb_size=st['obs_proj.weight'].shape[0], action_emb_size=st['action_emb.weight'].shape[1],
                      hidden_size_actor=st['gru_actor.weight_hh_l0'].shape[1],
                      hidden_size_critic=st['gru_critic.weight_hh_l0'].shape[1], n_agents=c['actions'].shape[0],
                      use_agent_embedding=False)
    net.load_state_dict(st)
    return c, net.to(device)


def hyper(c):
    return {k: float(c[k]) for k in ('gamma', 'entropy_coef', 'vf_coef', 'clip_range')}


def check_loss_and_grads(c, net, loss):
    ref = float(c['loss'])
    assert abs(loss.item() - ref) <= 1e-5 * abs(ref) + 1e-7, (loss.item(), ref)
    net.zero_grad()
    loss.backward()
    for k, p in net.named_parameters():
        g = (p.grad if p.grad is not None else torch.zeros_like(p)).cpu()
        gr = torch.from_numpy(c['g.' + k])
        assert torch.allclose(g, gr, rtol=1e-4, atol=1e-6), (k, (g - gr).abs().max())


@pytest.mark.parametrize('i', [0, 1, 2])
def test_mappo_loss_matches_reference(i):
    z = np.load(GOLD)
    c, net = load_case(z, i)
    idx, val = pack(c['obs'], cap=64)
    acts = torch.from_numpy(c['actions']).long()
    out = net.forward_emb(net.project_packed(idx, val), acts, torch.from_numpy(c['ha0']), torch.from_numpy(c['hc0']))
    loss = mappo_loss(out, torch.from_numpy(c['old_logits']), acts, torch.from_numpy(c['reward']),
                      torch.from_numpy(c['done']), **hyper(c))
    check_loss_and_grads(c, net, loss)


@pytest.mark.parametrize('i', [0, 1, 2])
def test_adam_step_matches_reference(i):
    """clip_grad_norm_(0.5) + one Adam(3e-4, eps 1e-5) step from the fixture's own gradients (mappo.py:16,27-28)."""
    z = np.load(GOLD)
    c, net = load_case(z, i)
    opt = torch.optim.Adam(net.parameters(), lr=3e-4, eps=1e-5)
    for k, p in net.named_parameters():
        p.grad = torch.from_numpy(c['g.' + k]).clone()
    torch.nn.utils.clip_grad_norm_(net.parameters(), 0.5)
    opt.step()
    for k, p in net.named_parameters():
        assert torch.allclose(p.detach(), torch.from_numpy(c['a.' + k]), rtol=0, atol=1e-6), k


@pytest.mark.parametrize('i', [0, 1, 2])
def test_monte_carlo_returns_match_reference(i):
    z = np.load(GOLD)
    r = monte_carlo_returns(torch.from_numpy(z[f'c{i}.reward']), torch.from_numpy(z[f'c{i}.done']), 0.99)
    assert torch.equal(r, torch.from_numpy(z[f'c{i}.returns']))


def _patterns(z):
    for i in range(int(z['wl.n'])):
        yield i, torch.from_numpy(z[f'wl.{i}.done'])


def test_chunk_starts_reference_rule_is_the_whitelist():
    z = np.load(GOLD)
    assert int(z['wl.n']) >= 20
    for i, d in _patterns(z):
        for cl in (1, 3, 5):
            got = chunk_starts(d[None], cl, rule='reference')[0]
            assert got.dtype == torch.bool
            assert torch.equal(got, torch.from_numpy(z[f'wl.{i}.cl{cl}']) != 0), (i, cl)
    # several rows at once are the rows one by one
    rows = torch.stack([d for _, d in _patterns(z) if d.numel() == 16])
    both = chunk_starts(rows, 5, rule='reference')
    for r in range(rows.shape[0]):
        assert torch.equal(both[r], chunk_starts(rows[r:r + 1], 5, rule='reference')[0])


def test_chunk_starts_episode_rule_by_brute_force():
    z = np.load(GOLD)
    n_valid = n_invalid = 0
    for i, d in _patterns(z):
        for cl in (1, 3, 5):
            got = chunk_starts(d[None], cl)[0]  # 'episode' is the default
            assert got.shape == (d.numel() - cl,)
            for s in range(d.numel() - cl):
                crosses = bool(d[s:s + cl - 1].any())  # a done flag before the chunk's last entry
                assert bool(got[s]) == (not crosses), (i, cl, s)
                n_valid += not crosses
                n_invalid += crosses
    assert n_valid and n_invalid
    with pytest.raises(ValueError):
        chunk_starts(torch.zeros(1, 8), 3, rule='other')


# ---------------------------------------------------------------------------------------------------------------------
# the ring, on the scripted engine (tests/scripted.py)
# ---------------------------------------------------------------------------------------------------------------------
def _scripted(**kw):
    eng = ScriptedEngine()
    f = factory(eng, [4] * eng.A)
    args = dict(n_steps=3, buffer_size=8, batch_size=64, n_updates=1, cap=2, obs_emb_size=6, action_emb_size=4,
                hidden_size=5, generator=torch.Generator().manual_seed(0))
    args.update(kw)
    torch.manual_seed(0)
    return eng, BatchedMAPPO(f, **args)


@pytest.mark.parametrize('rule', ['episode', 'reference'])
def test_ring_chunks_hold_what_was_pushed(rule):
    eng, tr = _scripted(chunk_rule=rule)
    seen_wrap = False
    tr.learn = lambda: None  # the buffer alone: no update, the weights stay
    for step in range(31):  # 9 ring slots: more than three wraps
        tr.step()
        if tr.filled < tr.S:
            continue
        picked = tr.sample()
        assert picked is not None
        mb = tr.minibatch(*picked)
        rows, slots = mb['rows'], mb['slots']
        assert not bool((slots == tr.head).any()), 'a chunk holds the pending entry at the write head'
        # the chunk's entries are consecutive steps: entry j of a chunk was pushed at step k0 + j
        k = (mb['val'][:, :, 0] / 1000).floor().long()
        assert torch.equal(k, k[:, :1] + torch.arange(tr.T)), 'a chunk is not consecutive in time'
        assert int(k.max()) < eng.k and int(k.min()) >= eng.k - tr.S
        seen_wrap |= bool((slots[:, 1:] < slots[:, :-1]).any())
        b, a = rows // tr.A, rows % tr.A
        code = (1000 * k + 10 * b[:, None] + a[:, None] + 1).float()
        assert torch.equal(mb['val'][:, :, 0], code) and torch.equal(mb['idx'][:, :, 0].long(), a[:, None].expand_as(k))
        assert torch.equal(mb['reward'], 1000.0 + code + 0.5)  # the reward of the step after entry k
        done = ((k + 1 + 3 * b[:, None]) % eng.period == 0).float()
        assert torch.equal(mb['done'], done)
        if rule == 'episode':
            assert not bool(done[:, :-1].any())
        else:
            assert not bool(done.any())
        # inputs: the previous entry's action (-1 after an episode end), and the stored states and logits
        prev_done = ((k + 3 * b[:, None]) % eng.period == 0) & (k > 0)
        assert bool((mb['act_in'][prev_done] == -1).all())
        flat = lambda t: t.reshape(tr.R, tr.N, *t.shape[3:])  # noqa: E731
        prev = flat(tr.act)[(slots - 1) % tr.R, rows[:, None]].long()
        first_ever = k == 0
        assert torch.equal(mb['act_in'][~prev_done & ~first_ever], prev[~prev_done & ~first_ever])
        assert torch.equal(mb['act'], flat(tr.act)[slots, rows[:, None]].long())
        assert torch.equal(mb['ha'][:, 0], tr.ha_in[slots[:, 0], rows])
        # no weight has changed: the chunk forward from the stored states reproduces the acting logits
        with torch.no_grad():
            out = tr.evaluate(mb)
        assert torch.allclose(out['logits'], mb['old_logits'], rtol=1e-4, atol=1e-5)
    assert seen_wrap, 'no sampled chunk crossed the physical end of the ring'


def test_batched_mappo_learns_on_the_scripted_engine():
    eng, tr = _scripted(n_updates=2)
    w0 = {k: p.detach().clone() for k, p in tr.net.named_parameters()}
    tr.train(8)
    assert tr.updates == 0 and tr.filled == 8  # full after 8 steps; the learn call falls on step 9
    tr.train(4)
    assert tr.updates == 4 and tr.skipped_updates == 0  # learn calls at steps 9 and 12
    assert bool(torch.isfinite(tr.last_loss))
    assert any(not torch.equal(w0[k], p.detach()) for k, p in tr.net.named_parameters())
    # the engine projects with the new weights, and the pending observation was re-projected
    assert torch.equal(tr.pobs.wt, tr.net.obs_proj.weight.detach().t())
    e = tr.net.project_packed(tr.pobs.idx[tr.head], tr.pobs.val[tr.head])
    assert torch.allclose(e, tr.pobs.emb[tr.head], rtol=1e-5, atol=1e-5)
    assert float(tr.episodes) == float(sum(((k + 3 * b) % eng.period == 0) for k in range(1, 13) for b in range(eng.B)))
    assert eng.defer == [False] * 12  # the ring never defers the engine's floor-shuffle replay


def test_no_valid_start_skips_the_update():
    eng, tr = _scripted(chunk_rule='reference', buffer_size=4, n_updates=3)
    eng.period = 2  # an episode end every other step: the reference rule leaves no start
    tr.train(9)
    assert tr.updates == 0 and tr.skipped_updates == 3 * 2  # learn calls at steps 6 and 9 (full after 4)


def test_constructor_errors():
    with pytest.raises(ValueError, match='buffer_size'):
        _scripted(buffer_size=3, n_steps=3)
    f = factory(ScriptedEngine(), [4, 5])
    with pytest.raises(ValueError, match='same number of actions'):
        BatchedMAPPO(f)
