"""The action mask on the device (include/mfg.h mfg_action_mask, csrc/mfg_kernels.h k_action_mask) and masked acting
(include/mfg_act.h mfg_policy_act_masked, BatchedEvaluator(mask_invalid=True)). Every check is exact.

Two yardsticks for the mask, both older than it: the C oracle through the replay checker (tests/action_mask_ref.py), and
the engine's own step: the record of one env copied into one row per (agent, slot), one step in which row (a, s) has
agent a play s and every other agent its Noop; the step's ev_act valid bits are the mask.
"""
import ctypes

import numpy as np
import pytest
import torch

from conftest import gpu_available
import action_mask_ref as M
import mfg_amd.evaluate as EV
from mfg_amd import abi, learn_lib
from mfg_amd.action_mask import dense_mask, masked_logits
from mfg_amd.engine import Engine, HDR, HDR_N, RecordView

pytestmark = pytest.mark.gpu


def _need_gpu():
    if not gpu_available():
        pytest.skip('no GPU')


def _u32(t):
    return t.cpu().numpy().astype(np.int64) & 0xFFFFFFFF


def _header(eng, state, key):
    """Header slot `key` of every env of an exported state [B, size] as a numpy array."""
    o = eng.layout['o_hdr']
    return state[:, o:o + 4 * HDR_N].contiguous().cpu().numpy().view(np.int32)[:, HDR[key]]


# ---------------------------------------------------------------------------------------------------------------------
# against the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cfg', ['dense', 'rooms4.yaml', 'logic_stress.yaml'])
def test_mask_against_the_oracle(cfg):
    _need_gpu()
    spec = M.spec_of(cfg)
    B, A, base, steps = 3, spec.n_agents, 11, 20
    eng = Engine(spec, B)
    eng.reset(init=True, seed_base=base)
    rng = np.random.default_rng(5)
    acts = [[[int(rng.integers(0, k)) for k in spec.n_actions] for _ in range(B)] for _ in range(steps)]
    done = torch.zeros((1, B), dtype=torch.uint8, device='cuda')
    ev_misc = torch.zeros((1, B, abi.EV_MISC_N), dtype=torch.int32, device='cuda')
    alive, crashed = [True] * B, np.zeros(B, bool)
    compared = 0
    for t in range(steps):
        if t % 3 == 0:
            got = _u32(eng.action_mask())
            for b in range(B):
                if alive[b]:
                    want = M.mask_of_state(spec, base + b, [acts[k][b] for k in range(t)])
                    assert np.array_equal(got[b], want.astype(np.int64)), (cfg, t, b, got[b], want)
                    assert all((int(got[b][a]) >> spec.n_actions[a]) == 0 for a in range(A))
                    compared += 1
                elif crashed[b]:
                    assert not got[b].any()  # a crashed env has no valid action
        a_t = torch.tensor(acts[t], dtype=torch.int32, device='cuda')
        eng.step(1, actions=a_t, done=done, ev_misc=ev_misc, auto_reset=False)
        crashed = ((ev_misc[0, :, abi.EVM_FLAGS] >> 1) & 1).cpu().numpy().astype(bool)
        for b in range(B):  # the oracle has no auto-reset: an env is compared until its episode ends
            alive[b] = alive[b] and not bool(done[0, b]) and not crashed[b]
    assert compared >= 12, 'the episodes ended too early for the comparison to mean anything'
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# against the step itself: one row per (agent, slot)
# ---------------------------------------------------------------------------------------------------------------------
def _fan_rows(spec):
    rows = [(a, s) for a in range(spec.n_agents) for s in range(spec.n_actions[a])]
    noop = M.noop_slots(spec)
    acts = np.tile(np.asarray(noop, np.int32), (len(rows), 1))
    for r, (a, s) in enumerate(rows):
        acts[r, a] = s
    return rows, torch.from_numpy(acts).cuda()


def _fan_out(eng, spec, record):
    """Every row of the engine becomes `record` (uint8 [size], device); returns (mask words of row 0 as u32 ints [A],
    the same from the step's ev_act valid bits). The engine's state is the stepped one afterwards."""
    rows, acts = _fan_rows(spec)
    assert eng.B == len(rows)
    eng.import_state(record[None].expand(eng.B, -1).contiguous())
    got = _u32(eng.action_mask())
    assert (got == got[0]).all(), 'equal records gave different masks'
    ev_act = torch.zeros((eng.B, spec.n_agents), dtype=torch.uint8, device='cuda')
    eng.step(1, actions=acts, ev_act=ev_act, auto_reset=False)
    ev = ev_act.cpu().numpy()
    want = np.zeros(spec.n_agents, np.int64)
    for r, (a, s) in enumerate(rows):
        if ev[r, a] & 0x81 == 0x81:
            want[a] |= 1 << s
    return got[0], want


def _stepped_engine(cfg, n_pre, seed_base=3):
    spec = M.spec_of(cfg)
    B = sum(spec.n_actions)
    eng = Engine(spec, B)
    eng.reset(init=True, seed_base=seed_base)
    gen = torch.Generator().manual_seed(17)
    counts = torch.tensor(spec.n_actions)
    for _ in range(n_pre):
        a = (torch.rand((B, spec.n_agents), generator=gen) * counts).floor().to(torch.int32).cuda()
        eng.step(1, actions=a, auto_reset=False)
    return spec, eng


@pytest.mark.parametrize('cfg', ['dense', 'cap_groups.yaml', 'agents81.yaml', 'cap_dest81.yaml'])
def test_mask_against_the_step(cfg):
    _need_gpu()
    spec, eng = _stepped_engine(cfg, 9)
    assert eng.layout  # (cap_groups: groups above 64 slots, agents81 / cap_dest81: more than 64 agents -> NW = 2)
    state = eng.export_state()
    live = np.nonzero(_header(eng, state, 'crashed') == 0)[0]
    assert len(live) >= 3
    seen = set()
    for b in live[:3]:  # three different states after nine random steps
        got, want = _fan_out(eng, spec, state[int(b)].clone())
        assert np.array_equal(got, want), (cfg, int(b), got, want)
        seen.update(int(x) for x in got)
    assert len(seen) > 1, 'every agent of every state had the same mask'
    eng.close()


def test_mask_against_the_step_with_low_batteries():
    """Charge's valid branch and its two-agents-on-the-pod branch: on a fresh episode the battery starts at 1.0 and only
    rises, so the exported records get their battery f64s lowered (nothing else is edited) before the fan-out."""
    _need_gpu()
    spec, eng = _stepped_engine('dense', 16)  # (of these 60 envs' states, 40 have an agent alone on a pod, 3 two on one)
    A, L = spec.n_agents, eng.layout
    state = eng.export_state()
    ob = L['o_battery']
    bat = torch.full((eng.B, A), 0.5, dtype=torch.float64, device='cuda')
    state[:, ob:ob + 8 * A] = bat.view(torch.uint8).view(eng.B, 8 * A)
    host = state.cpu().numpy()
    ok = (_header(eng, state, 'crashed') == 0)
    charge = [M.slot_ops(spec)[a].index(abi.ACT_CHARGE) for a in range(A)]
    alone = shared = None
    for b in np.nonzero(ok)[0]:
        v = RecordView(host[b], L, spec)
        assert (v.battery() == 0.5).all()
        pods = v.group('pods')
        pod_cells = set(int(w & 0xFFFF) for w in pods if w & 0x10000)
        pos = [int(p) for p in v.agent_pos()]
        on = [a for a in range(A) if pos[a] in pod_cells]
        if alone is None and any(pos.count(pos[a]) == 1 for a in on):
            alone = (int(b), [a for a in on if pos.count(pos[a]) == 1])
        if shared is None and any(pos.count(pos[a]) > 1 for a in on):
            shared = (int(b), [a for a in on if pos.count(pos[a]) > 1])
    assert alone is not None and shared is not None, 'the probed states miss one of Charge\'s two branches'
    for (b, agents), valid in ((alone, True), (shared, False)):
        got, want = _fan_out(eng, spec, state[b].clone())
        assert np.array_equal(got, want), (b, got, want)
        for a in agents:
            assert bool((got[a] >> charge[a]) & 1) == valid, (b, a, valid)
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# agent 0 over a rollout with auto-reset
# ---------------------------------------------------------------------------------------------------------------------
def test_agent0_over_a_rollout():
    _need_gpu()
    spec = M.spec_of('large8.yaml')
    B, A, steps = 64, spec.n_agents, 100
    eng = Engine(spec, B)
    eng.reset(init=True, seed_base=40)
    gen = torch.Generator().manual_seed(23)
    counts = torch.tensor(spec.n_actions)
    ev_act = torch.zeros((B, A), dtype=torch.uint8, device='cuda')
    done = torch.zeros(B, dtype=torch.uint8, device='cuda')
    mask = torch.zeros((B, A), dtype=torch.int32, device='cuda')
    checked = episodes = valid = 0
    for t in range(steps):
        crashed = torch.from_numpy(_header(eng, eng.export_state(), 'crashed') != 0).cuda()
        assert eng.action_mask(out=mask) is mask
        a = (torch.rand((B, A), generator=gen) * counts).floor().to(torch.int32).cuda()
        eng.step(1, actions=a, ev_act=ev_act, done=done, auto_reset=True, step_base=t)
        bit = (mask[:, 0].long() >> a[:, 0].long()) & 1
        ev = ev_act[:, 0].long()
        keep = ~crashed
        assert torch.equal(bit[keep], (ev & 1)[keep]), t
        assert bool(((ev & 0x80) != 0)[keep].all())
        checked += int(keep.sum())
        valid += int(bit[keep].sum())
        episodes += int(done.sum())
    assert checked >= B * steps * 9 // 10 and 0 < valid < checked
    print(f'agent 0: {valid} of {checked} random actions valid, {episodes} episode ends')
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# masked acting
# ---------------------------------------------------------------------------------------------------------------------
def _act(w, emb, h, pa, pd, u, n_act, mask='plain', greedy=False):
    """One acting call on device copies, engine layout. mask 'plain': mfg_policy_act; None: mfg_policy_act_masked with a
    NULL mask; else the int32 words [B, A]. Returns (logits [B, A, n_max], h' [B, A, H], act [B, A])."""
    import test_gpu_eval as G
    wd = {k: v.cuda().contiguous() for k, v in w.items() if not k.startswith('_')}
    B, A, E = emb.shape
    H, n_max = w['wat'].shape[1], w['wbt'].shape[2]
    e_d, h_d, a_d = emb.cuda().contiguous(), h.cuda().contiguous().clone(), pa.cuda().contiguous().clone()
    lg = torch.zeros((B, A, n_max), device='cuda')
    n_d = torch.tensor(n_act, dtype=torch.int32, device='cuda')
    pd_d, u_d = pd.cuda(), u.cuda()
    if isinstance(mask, str):
        rc = EV.policy_act(wd, e_d, (A * E, E), B, A, n_d, a_d, pd_d, h_d, (A * H, H), u_d, a_d, lg, greedy)
    elif mask is None:
        g, k_in, e_dim = wd['w1t'].shape
        rc = learn_lib.lib().mfg_policy_act_masked(
            e_d.data_ptr(), A * E, E, B, A, g, e_dim, k_in - e_dim, H, n_max, ctypes.byref(EV._weights_struct(wd)),
            n_d.data_ptr(), a_d.data_ptr(), pd_d.data_ptr(), h_d.data_ptr(), A * H, H, u_d.data_ptr(),
            1 if greedy else 0, None, a_d.data_ptr(), lg.data_ptr(), G._stream())
    else:
        rc = EV.policy_act(wd, e_d, (A * E, E), B, A, n_d, a_d, pd_d, h_d, (A * H, H), u_d, a_d, lg, greedy,
                           mask=mask.cuda().contiguous())
    torch.cuda.synchronize()
    assert rc == 0
    return lg, h_d, a_d


def _filled(lg, words, n_act, g):
    """The raw logits with the masked entries of each agent's own first n_act columns set to -inf."""
    out = lg.clone()
    for i in range(lg.shape[1]):
        n = n_act[i % g]
        out[:, i, :n] = masked_logits(lg[:, i, :n], words[:, i].cuda())
    return out


@pytest.mark.parametrize('g', [1, 3])
def test_masked_acting(g):
    _need_gpu()
    import test_gpu_eval as G
    for E, AE, H in G.SIZES:
        gen = torch.Generator().manual_seed(300 * g + E)
        shapes = [(1, 1), (86, 3)] if g == 1 else [(1, 3), (86, 3)]
        for n_max in (1, 11, 32):
            n_act = G.n_acts(n_max, g)
            w = G.make_weights(g, E, AE, H, n_max, gen)
            for B, A in shapes:
                emb, h, pa, pd, u = G.make_inputs(B, A, E, H, n_act, gen)
                key = (g, E, n_max, B, A)
                base = _act(w, emb, h, pa, pd, u, n_act)
                cnt = torch.tensor([n_act[i % g] for i in range(A)])
                exact = ((1 << cnt.long()) - 1).expand(B, A)
                exact = torch.where(exact >= 2 ** 31, exact - 2 ** 32, exact).to(torch.int32)
                # a NULL mask, every bit set, exactly the agent's own bits set: mfg_policy_act's bits
                for m in (None, torch.full((B, A), -1, dtype=torch.int32), exact):
                    for x, y in zip(_act(w, emb, h, pa, pd, u, n_act, m), base):
                        assert torch.equal(x, y), key
                # a random mask with all-zero words in places
                bits = torch.rand((B, A, 32), generator=gen) < 0.4
                words = (bits.long() << torch.arange(32)).sum(-1)
                words = torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32)
                words[torch.rand((B, A), generator=gen) < 0.15] = 0
                words[0, 0] = 0
                lg, hn, act = _act(w, emb, h, pa, pd, u, n_act, words)
                assert torch.equal(lg, base[0]) and torch.equal(hn, base[1]), key  # raw logits, the same state
                filled = _filled(lg, words, n_act, g)
                assert torch.equal(act, G.sampler(filled, u, n_act, g)), key
                own = torch.stack([dense_mask(words[:, i], 32)[:, :n_max] & (torch.arange(n_max) < n_act[i % g])
                                   for i in range(A)], 1)
                has = own.any(-1)
                picked = torch.gather(own, -1, act.cpu().long().clamp(min=0)[..., None])[..., 0]
                assert int(act.min()) >= 0 and bool(picked[has].all()), key
                assert torch.equal(act.cpu()[~has], base[2].cpu()[~has]), key  # all-zero rows: the unmasked pick
                # greedy: the lowest-index argmax over the set bits; an all-zero row: over all
                lg2, hn2, act2 = _act(w, emb, h, pa, pd, u, n_act, words, greedy=True)
                assert torch.equal(lg2, lg) and torch.equal(hn2, hn)
                for i in range(A):
                    n = n_act[i % g]
                    assert torch.equal(act2[:, i], filled[:, i, :n].argmax(-1).to(torch.int32)), key


# ---------------------------------------------------------------------------------------------------------------------
# the evaluator
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('per_agent', [False, True])
def test_masked_fused_and_tensor_first_step_agree(per_agent):
    """tests/test_gpu_eval.py's test_fused_and_tensor_first_step_agree with mask_invalid=True: the raw logits of the two
    paths stay within their two errors against f64, and each path's actions are the masked sample of its own logits."""
    _need_gpu()
    import test_gpu_eval as G
    (fa, ea), (fb, eb) = G._rooms4(per_agent, True, mask_invalid=True), G._rooms4(per_agent, False, mask_invalid=True)
    out = []
    for ev in (ea, eb):
        ev.reset()
        lg = torch.zeros((ev.B, ev.A, ev.n_max), device='cuda')
        ev._act(True, lg)
        out.append(lg)
        assert torch.equal(ev.mask, ev.f.engine.action_mask())
        n = ev.n_act[0]
        want = G.sampler(masked_logits(lg[..., :n], ev.mask).contiguous(), ev._u, [n], 1)
        assert torch.equal(ev.act, want)
        d = dense_mask(ev.mask, n)
        assert bool(d.any(-1).all()) and not bool(d.all())  # Noop is always there; something is masked
        assert bool(torch.gather(d, -1, ev.act.long()[..., None]).all())
    assert torch.equal(ea.mask, eb.mask)
    emb = (eb._emb.transpose(0, 1) if per_agent else eb.pobs.emb[0]).cpu()
    B, A = eb.B, eb.A
    ref, _ = G.formulas(G._evaluator_weights(eb), emb, torch.zeros(B, A, 64), torch.zeros((B, A), dtype=torch.int32),
                        torch.ones(B, dtype=torch.uint8), torch.float64)
    e_f, e_u = (float((x.double() - ref).abs().max()) for x in out)
    d = float((out[0] - out[1]).abs().max())
    print(e_f, e_u, d)
    assert e_f <= 4 * e_u + 1e-7 and d <= 5 * e_u + 1e-7
    fa.close()
    fb.close()


@pytest.mark.parametrize('fused', [True, False])
def test_masked_evaluator_agent0_is_never_invalid(fused):
    """A short masked run on rooms4: agent 0 acts first, so its masked action is always valid."""
    _need_gpu()
    import test_gpu_eval as G
    f, ev = G._rooms4(False, fused, mask_invalid=True)
    ev.reset()
    eng = f.engine
    ev_act = torch.zeros((ev.B, ev.A), dtype=torch.uint8, device='cuda')
    later_invalid = 0
    for t in range(40):
        ev._act(t == 0)
        acts = ev.act.clone()
        assert int(acts.min()) >= 0
        eng.step(1, actions=acts, reward=ev.rew, done=ev.done, obs=ev.pobs, ev_act=ev_act, auto_reset=True,
                 step_base=f.t)
        f.t += 1
        assert bool(((ev_act[:, 0] & 0x81) == 0x81).all()), t
        later_invalid += int(((ev_act[:, 1:] & 0x81) == 0x80).sum())
    print(f'invalid actions of agents 1..: {later_invalid} of {40 * ev.B * (ev.A - 1)}')
    f.close()
