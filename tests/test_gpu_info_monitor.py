"""GPU: the device episode monitor (k_info_step through engine.InfoMonitor / monitor.BatchedEnvMonitor) against the
pinned torch path (BatchedFactory.info_columns), against itself across fused and single-step calls, and against the
reference's recorded infos; its finished-episode buffer at capacity; masked resets; the VectorFactory wrapping."""
import numpy as np
import pytest

from conftest import gpu_available
import info_fold as F

pytestmark = pytest.mark.gpu

FLAGS, CRASH_BIT = 6, 2  # MFG_EVM_FLAGS, its crashed bit


def _need_gpu():
    if not gpu_available():
        pytest.skip('no GPU')
    import torch
    return torch


def _acts(torch, seed, B, t, spec, device):
    from philox import synthetic_actions
    return torch.tensor(synthetic_actions(seed, np.arange(B), t, spec.n_actions), dtype=torch.int32, device=device)


@pytest.mark.parametrize('cfg,B,kpl', [('alltest16.yaml', 67, 4), ('maint_rooms.yaml', 67, None),
                                       ('eight_puzzle.yaml', 67, None), ('qquad_doors.yaml', 67, None),
                                       ('cap_dest81.yaml', 5, 0)])
def test_step_columns_equal_torch_columns(cfg, B, kpl, min_maint_slot=None):
    """60 steps of explicit Philox-derived actions: every step, the kernel's columns and presence equal
    BatchedFactory.info_columns bit for bit over all envs (crashed envs: the kernel's rows are 0). B = 67 is more
    than one wave of envs and no multiple of the waves per workgroup; alltest16 has several keys per lane in
    registers, cap_dest81 (81 agents: two-pass row staging) runs the LDS-accumulator kernel. min_maint_slot: the run
    must hold a step in which the kernel's column of a maintainer slot >= it is present and non-zero."""
    torch = _need_gpu()
    from mfg_amd.factory import BatchedFactory
    from mfg_amd.monitor import BatchedEnvMonitor
    bf = BatchedFactory(cfg, B, seed_base=40)
    mon = BatchedEnvMonitor(bf)
    Kc = mon.monitor.Kc
    want_kpl = 1 if Kc <= 64 else 2 if Kc <= 128 else 4 if Kc <= 256 else 0
    assert mon.monitor.keys_per_lane == want_kpl and (kpl is None or kpl == want_kpl)
    assert mon.monitor.lds_bytes <= 64 * 1024 and 1 <= mon.monitor.waves_per_block <= 4
    mon.reset()
    bad, live, maint_hit = [], 0, min_maint_slot is None
    for t in range(60):
        at = _acts(torch, 11, B, t, bf.spec, bf.device)
        mon.step(at)
        names, vals, pres = mon.step_columns()
        rnames, rvals, rpres = bf.info_columns(at)
        assert names == rnames
        if not maint_hit:
            upper = [k for k, n in enumerate(names) if n.startswith('Maintainer[slot ')
                     and int(n[len('Maintainer[slot '):n.index(']')]) >= min_maint_slot]
            assert upper, f'{cfg} has no column of a maintainer slot >= {min_maint_slot}'
            maint_hit = bool((pres[:, upper] & (vals[:, upper] != 0)).any())
        ok = (bf.ev_misc[:, FLAGS] & CRASH_BIT) == 0
        live += int(ok.sum())
        if not (torch.equal(vals[ok], rvals[ok]) and torch.equal(pres[ok], rpres[ok])):
            bad.append(t)
        assert not vals[~ok].any() and not pres[~ok].any()
    mon.close()
    assert not bad and live > 0, (cfg, bad[:10])
    assert maint_hit, f'{cfg}: no maintainer column of a slot >= {min_maint_slot} was ever present and non-zero'


def _stagger_masks(torch, B, device):
    return [torch.tensor([1 if b % 3 == g else 0 for b in range(B)], dtype=torch.uint8, device=device) for g in (1, 2)]


def _rooms4_run(torch, K, n_calls, B=67, pseed=5, base=300):
    """rooms4 ends every episode at max_steps = 500, so two masked resets after steps 0 and 1 move a third of the
    envs each by one and two steps. Those two single steps are common to every run; then n_calls calls of K fused
    steps with the on-device Philox actions in the engine and in the monitor. -> (drained rows, done u8 [T, B])."""
    from mfg_amd.spec import compile_spec
    from mfg_amd.engine import Engine, InfoMonitor, EV_MISC
    from mfg_amd.info_program import compile_info_program
    spec = compile_spec('rooms4.yaml')
    eng = Engine(spec, B)
    dev, A = eng.device, spec.n_agents
    mon = InfoMonitor(compile_info_program(spec), B, device=dev)
    bufs = lambda k: dict(reward=torch.zeros((k, B, A), dtype=torch.float64, device=dev),
                          done=torch.zeros((k, B), dtype=torch.uint8, device=dev),
                          ev_act=torch.zeros((k, B, A), dtype=torch.uint8, device=dev),
                          ev_watch=torch.zeros((k, B, A), dtype=torch.uint8, device=dev),
                          ev_misc=torch.zeros((k, B, EV_MISC), dtype=torch.int32, device=dev))
    eng.reset(init=True, seed_base=base)
    dones, t = [], 0
    one = bufs(1)
    for mask in _stagger_masks(torch, B, dev):
        eng.step(1, philox_seed=pseed, env_base=base, step_base=t, auto_reset=True, **one)
        mon.step(1, philox_seed=pseed, env_base=base, step_base=t, **one)
        dones.append(one['done'].clone())
        eng.reset(mask=mask, seed_base=base)
        mon.reset(mask)
        t += 1
    kb = bufs(K)
    for _ in range(n_calls):
        eng.step(K, philox_seed=pseed, env_base=base, step_base=t, auto_reset=True, **kb)
        mon.step(K, philox_seed=pseed, env_base=base, step_base=t, **kb)
        dones.append(kb['done'].clone())
        t += K
    rows = mon.drain()
    mon.close()
    eng.close()
    return rows, torch.cat(dones).cpu().numpy()


def test_fused_steps_with_episode_ends_inside_the_call():
    """K = 3 fused calls (Philox actions recomputed in the kernel, auto-reset) against K = 1 calls of the same
    seeds: the drained rows are equal with ==, and episodes ended at k = 0, 1 and 2 of a fused call."""
    torch = _need_gpu()
    n_calls = 168  # steps 2 .. 505: past the staggered episode ends at steps 499, 500 and 501
    (h1, s1, c1, d1), done1 = _rooms4_run(torch, 1, 3 * n_calls)
    (h3, s3, c3, d3), done3 = _rooms4_run(torch, 3, n_calls)
    assert np.array_equal(done1, done3)
    ks = {(int(t) - 2) % 3 for t, b in zip(*np.nonzero(done1)) if t >= 2}
    assert ks == {0, 1, 2}, ks
    assert d1 == d3 == 0 and len(h1) == int(done1.sum()) >= 67
    assert np.array_equal(h1, h3) and np.array_equal(c1, c3) and np.array_equal(s1, s3)
    # the masked resets moved the episode starts: a first episode's length counts from the env's reset, not step 0
    first = {int(e): int(n) for e, i, n in zip(h1[:, 0], h1[:, 1], h1[:, 2]) if i == 0}
    ends = {b: int(np.nonzero(done1[:, b])[0][0]) for b in range(67)}
    assert all(ends[b] >= 2 and first[b] == ends[b] + 1 - (b % 3) for b in range(67))


def _fixture_rows(torch, tag, seed):
    """The fixture's recorded actions through the engine at B = 1 (as tests/test_gpu_parity.py replays it), every
    step folded by the monitor. -> (program, drained rows, reference fold of the recorded infos)."""
    from mfg_amd.spec import compile_spec
    from mfg_amd.engine import Engine, InfoMonitor, EV_MISC
    from mfg_amd.info_program import compile_info_program
    import golden_compare as G
    rec, _ = G.load(tag, seed)
    spec = compile_spec(f'{tag}.yaml')
    prog = compile_info_program(spec)
    eng = Engine(spec, 1)
    dev, A = eng.device, spec.n_agents
    mon = InfoMonitor(prog, 1, device=dev)
    rew = torch.zeros((1, A), dtype=torch.float64, device=dev)
    done = torch.zeros(1, dtype=torch.uint8, device=dev)
    ev_a = torch.zeros((1, A), dtype=torch.uint8, device=dev)
    ev_w = torch.zeros((1, A), dtype=torch.uint8, device=dev)
    ev_m = torch.zeros((1, EV_MISC), dtype=torch.int32, device=dev)
    steps = []
    for r in rec['steps']:
        if r['step'] == 0:
            eng.reset(init=(r['t'] == 0), seed_base=rec['py_seed'])
            continue
        act = torch.tensor([r['actions']], dtype=torch.int32, device=dev)
        eng.step(1, actions=act, reward=rew, done=done, ev_act=ev_a, ev_watch=ev_w, ev_misc=ev_m, auto_reset=False)
        mon.step(1, ev_a, ev_w, ev_m, rew, done, actions=act)
        steps.append(dict(fixture_crashed=bool(r.get('crashed')), fixture_done=bool(r['done']), info=r['info']))
    rows = mon.drain()
    mon.close()
    eng.close()
    return prog, rows, F.fold_reference(steps)


@pytest.mark.parametrize('tag,seed', [('maint_rooms', 0), ('large8', 1)])
def test_single_env_rows_equal_reference_fold(tag, seed):
    """B = 1 on the fixture's actions: the drained episode rows == the Python fold of the reference's recorded info
    dicts: sums, counts, lengths, and the maintainer keys named from the row's maint_base."""
    torch = _need_gpu()
    from mfg_amd.info_program import HDR_EP_INDEX, HDR_LENGTH, HDR_CRASHED
    prog, (hdr, sums, counts, dropped), ref = _fixture_rows(torch, tag, seed)
    assert dropped == 0 and len(hdr) == len(ref) >= 2
    if tag == 'maint_rooms':
        assert any(k.startswith('Maintainer[') for ep in ref for k in ep['sum'])
    for i, ep in enumerate(ref):
        s, c = F.row_dicts(prog, hdr, sums, counts, i)
        assert s == ep['sum'] and c == ep['count'], (tag, i, sorted(set(s.items()) ^ set(ep['sum'].items()))[:6])
        assert (hdr[i][HDR_EP_INDEX], hdr[i][HDR_LENGTH], hdr[i][HDR_CRASHED]) == (i, ep['length'], ep['crashed'])


def test_capacity_drops_rows_and_keeps_counting():
    """ep_capacity = 4 on eight_puzzle at B = 64 (max_steps = 200: every env has finished by step 200): exactly 4
    rows are kept, each one a row the uncapped monitor also has; the counter equals the dones seen; drain reports the
    rest as dropped and restarts the counter; later episodes land again."""
    torch = _need_gpu()
    from mfg_amd.engine import InfoMonitor
    from mfg_amd.factory import BatchedFactory
    from mfg_amd.monitor import BatchedEnvMonitor
    B = 64
    bf = BatchedFactory('eight_puzzle.yaml', B, seed_base=7)
    mon = BatchedEnvMonitor(bf, ep_capacity=4)
    full = InfoMonitor(mon.program, B, device=bf.device, ep_capacity=16384)
    mon.reset()
    n_done = torch.zeros((), dtype=torch.int64, device=bf.device)

    def run(t0, t1):
        for t in range(t0, t1):
            at = _acts(torch, 3, B, t, bf.spec, bf.device)
            mon.step(at)
            full.step(1, bf.ev_act, bf.ev_watch, bf.ev_misc, bf.reward, bf.done, actions=at)
            n_done.add_(bf.done.sum())

    run(0, 201)
    seen = int(n_done)
    assert seen >= B > 4 and mon.monitor.episodes() == seen
    d = mon.drain()
    assert d['dropped'] == seen - 4 and len(d['env']) == 4 and mon.monitor.episodes() == 0
    fh, fs, fc, fdrop = full.drain()
    assert fdrop == 0 and len(fh) == seen
    where = {(int(h[0]), int(h[1])): i for i, h in enumerate(fh)}
    for j in range(4):
        i = where[(int(d['env'][j]), int(d['episode'][j]))]
        assert int(d['length'][j]) == fh[i][2] > 0
        assert np.array_equal(d['sum'][j].numpy(), fs[i]) and np.array_equal(d['count'][j].numpy(), fc[i])
    n_done.zero_()
    run(201, 402)  # every env finishes again by max_steps
    again = int(n_done)
    assert again >= B and mon.monitor.episodes() == again
    d2 = mon.drain()
    assert len(d2['env']) == 4 and d2['dropped'] == again - 4 and (d2['episode'] >= 1).all()
    assert mon.dropped == seen + again - 8 and len(mon.frame()) == 8
    full.close()
    mon.close()


def test_masked_reset_clears_exactly_the_masked_envs():
    """maint_rooms at B = 16: after 40 steps the odd envs are reset (env and monitor). Every finished episode's
    length and step_reward sum equal a bookkeeping that restarts at each done and, for the masked envs, at the reset:
    the masked envs count from the reset, the others keep what they had."""
    torch = _need_gpu()
    from mfg_amd.factory import BatchedFactory
    from mfg_amd.monitor import BatchedEnvMonitor
    B = 16
    bf = BatchedFactory('maint_rooms.yaml', B, seed_base=21)
    mon = BatchedEnvMonitor(bf)
    mon.reset()
    mask = torch.tensor([b % 2 for b in range(B)], dtype=torch.uint8, device=bf.device)
    length = torch.zeros(B, dtype=torch.int64, device=bf.device)
    ret = torch.zeros(B, dtype=torch.float64, device=bf.device)
    want, at_reset = [], None
    for t in range(345):  # max_steps = 300: every env, reset at step 40 or not, finishes an episode
        if t == 40:
            at_reset = length.cpu().tolist()
            mon.reset(mask=mask)
            length[mask.bool()] = 0
            ret[mask.bool()] = 0.0
        mon.step(_acts(torch, 9, B, t, bf.spec, bf.device))
        _, vals, _ = mon.step_columns()
        length += 1
        ret = ret + vals[:, -2]
        d = bf.done.bool()
        for b in d.nonzero().flatten().tolist():
            want.append((b, int(length[b]), float(ret[b])))
        length[d] = 0
        ret[d] = 0.0
    assert any(at_reset[b] > 0 for b in range(1, B, 2))  # the reset fell inside running episodes
    rows = mon.drain()
    got = sorted(zip(rows['env'].tolist(), rows['episode'].tolist(), rows['length'].tolist(),
                     rows['sum'][:, -2].tolist()))
    want_rows, n_ep = [], {}
    for b, n, r in want:
        want_rows.append((b, n_ep.get(b, 0), n, r))
        n_ep[b] = n_ep.get(b, 0) + 1
    assert rows['dropped'] == 0 and got == sorted(want_rows) and set(n_ep) == set(range(B))
    mon.close()


def test_vector_factory_wrapping_and_episode_log():
    """The monitor over a VectorFactory gives the rows it gives over the BatchedFactory alone; frame()['length']
    equals BatchedEpisodeLog's per (env, episode); and the episode's step_reward sum == the episode return of the
    agent-summed reward, both left-to-right f64 sums of the same rewards (per step over the agents, then over the
    steps), for every episode that did not crash. BatchedEpisodeLog's return_sum adds the other way round (per agent over the steps, then over the agents):
    each of the two is within gamma_n sum|r| of the exact sum (n = T A additions, gamma_n = n u / (1 - n u),
    u = 2^-53), so they agree within 2 gamma_n sum|r|."""
    torch = _need_gpu()
    from mfg_amd.factory import BatchedFactory
    from mfg_amd.monitor import BatchedEnvMonitor, BatchedEpisodeLog
    from mfg_amd.vec import VectorFactory
    cfg, B, T = 'maint_rooms.yaml', 32, 320
    vf = VectorFactory(cfg, B, seed_base=5)
    A = vf.n_agents
    mon = BatchedEnvMonitor(vf)
    log = BatchedEpisodeLog()
    mon.reset()
    ret = torch.zeros(B, dtype=torch.float64, device=vf.env.device)
    mag = torch.zeros(B, dtype=torch.float64, device=vf.env.device)
    ends = []
    for t in range(T):
        obs, rew, term, trunc, infos = mon.step(_acts(torch, 2, B, t, vf.spec, vf.env.device))
        log.update(infos)
        s = torch.zeros(B, dtype=torch.float64, device=rew.device)
        for a in range(A):
            s = s + rew[:, a]
        ret = ret + s
        mag = mag + rew.abs().sum(dim=1)
        d = term | trunc
        for b in d.nonzero().flatten().tolist():
            ends.append((b, float(ret[b]), float(mag[b])))
        ret[d] = 0.0
        mag[d] = 0.0
    df = mon.frame()
    rows_v = (np.concatenate(mon._hdr), np.concatenate(mon._sum), np.concatenate(mon._cnt))
    mon.close()

    bf = BatchedFactory(cfg, B, seed_base=5)
    mon_b = BatchedEnvMonitor(bf)
    mon_b.reset()
    for t in range(T):
        mon_b.step(_acts(torch, 2, B, t, bf.spec, bf.device))
    mon_b.drain()
    rows_b = (np.concatenate(mon_b._hdr), np.concatenate(mon_b._sum), np.concatenate(mon_b._cnt))
    mon_b.close()
    assert len(rows_v[0]) >= B and all(np.array_equal(x, y) for x, y in zip(rows_v, rows_b))

    lf = log.frame()
    lf['episode'] = lf.groupby('env').cumcount()
    a = df.sort_values(['env', 'episode']).reset_index(drop=True)
    b = lf.sort_values(['env', 'episode']).reset_index(drop=True)
    assert len(a) == len(b) == len(ends)
    assert list(a['env']) == list(b['env']) and list(a['length']) == list(b['length'])
    n_ep, want = {}, {}
    for env, r, m in ends:
        want[(env, n_ep.get(env, 0))] = (r, m)
        n_ep[env] = n_ep.get(env, 0) + 1
    crashed = {(int(h[0]), int(h[1])) for h in rows_v[0] if h[3]}
    assert len(crashed) < len(a)
    for i in range(len(a)):
        key = (int(a['env'][i]), int(a['episode'][i]))
        if key in crashed:  # a crashed step has no info dict: its reward row is in the env's return only
            continue
        r, m = want[key]
        assert a['step_reward'][i] == r, (i, key, a['step_reward'][i], r)
        nu = int(a['length'][i]) * A * 2.0 ** -53
        bound = 2 * nu / (1 - nu) * m
        assert abs(b['return_sum'][i] - r) <= bound, (i, b['return_sum'][i], r, bound)


@pytest.mark.parametrize('n_keys,wpb', [(2000, 2), (4096, 1)])
def test_wide_programs_run_with_fewer_waves_per_block(n_keys, wpb):
    """More columns than four waves' LDS slices hold: the LDS-accumulator kernel runs with 2 waves per workgroup at
    2,002 columns and 1 at the 4,098-column bound. A hand-written program on random event rows (no engine), K = 2,
    B = 7, one crashed step and dones at both k: columns and rows == the host evaluation and its fold."""
    torch = _need_gpu()
    from mfg_amd import abi
    from mfg_amd.engine import InfoMonitor
    from mfg_amd.info_program import InfoProgram, OP_DTYPE, KIND, eval_host
    A, B, K = 3, 7, 2
    recs, key_off = [], [0]
    for k in range(n_keys):
        recs.append((k, KIND['watch_bit'], k % A, 1 << (k % 8), 0, 0.5 + k))
        if k % 5 == 0:
            recs.append((k, KIND['done_bit'], 0, k % 32, 0, -1.0))
        key_off.append(len(recs))
    prog = InfoProgram([f'k{k}' for k in range(n_keys)] + ['step_reward', 'step'], np.array(recs, OP_DTYPE), key_off,
                       np.zeros((A, 32, 5)), [4] * A, 0.0, 0)
    mon = InfoMonitor(prog, B, ep_capacity=64)
    assert (mon.Kc, mon.keys_per_lane, mon.waves_per_block) == (n_keys + 2, 0, wpb) and mon.lds_bytes <= 64 * 1024
    rng = np.random.default_rng(n_keys)
    acts = rng.integers(0, 4, (K, B, A)).astype(np.int32)
    ea = rng.integers(0, 256, (K, B, A)).astype(np.uint8)
    ew = rng.integers(0, 256, (K, B, A)).astype(np.uint8)
    em = rng.integers(-2 ** 31, 2 ** 31, (K, B, abi.EV_MISC_N)).astype(np.int32)
    em[:, :, abi.EVM_FLAGS] &= ~2
    em[1, 4, abi.EVM_FLAGS] |= 2  # env 4 crashes at k = 1
    rw = rng.standard_normal((K, B, A))
    dn = np.zeros((K, B), np.uint8)
    dn[0, 1] = dn[1, 1] = dn[1, 2] = dn[0, 5] = 1
    dev = mon.device
    t = lambda x: torch.from_numpy(x).to(dev)
    vals = torch.zeros((K, B, mon.Kc), dtype=torch.float64, device=dev)
    pres = torch.zeros((K, B, mon.Kc), dtype=torch.uint8, device=dev)
    mon.step(K, t(ea), t(ew), t(em), t(rw), t(dn), actions=t(acts), vals=vals, pres=pres)
    hdr, sums, counts, dropped = mon.drain()
    vals, pres = vals.cpu().numpy(), pres.cpu().numpy()
    want = []
    for b in range(B):
        steps = []
        for k in range(K):
            v, p = eval_host(prog, acts[k, b], ea[k, b], ew[k, b], em[k, b], rw[k, b])
            assert np.array_equal(vals[k, b], v) and np.array_equal(pres[k, b], p), (k, b)
            steps.append(dict(vals=v, pres=p, done=bool(dn[k, b]), crashed=bool(em[k, b, abi.EVM_FLAGS] & 2),
                              misc=em[k, b]))
        h, s, c = F.fold_host(prog, steps)
        h[:, 0] = b
        want.append((h, s, c))
    assert pres.any() and dropped == 0 and len(hdr) == 5
    assert np.array_equal(hdr, np.concatenate([w[0] for w in want]))
    assert np.array_equal(sums, np.concatenate([w[1] for w in want]))
    assert np.array_equal(counts, np.concatenate([w[2] for w in want]))
    mon.close()
