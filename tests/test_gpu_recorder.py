"""GPU: the batched state recorder (k_record_rows / k_record_occ through engine.StateRecorder and
monitor.BatchedEnvRecorder). The expected records and occupancy come from the C oracle (views_compare.oracle_snapshot,
pinned to the reference's summarize_state fixtures), never from the code under test: records per env and episode,
device rows against the host row reference, the split step against the auto-reset step, the occupancy map on its LDS
and its global path, the row ring at capacity and the episode filter.

Everywhere: actions are philox.synthetic_actions(11, env ids, t, n_actions), seed_base = 40, oracle env b is
OracleEnv(spec, 40 + b), reset when done."""
import functools

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = pytest.mark.gpu

SEED, BASE = 11, 40


def _need_gpu():
    if not gpu_available():
        pytest.skip('no GPU')
    import torch
    return torch


@functools.lru_cache(maxsize=None)
def _spec(cfg):
    from mfg_amd.spec import compile_spec
    return compile_spec(cfg)


@functools.lru_cache(maxsize=None)
def _actions(cfg, B, steps):
    """int32 [steps, B, A] (numpy, read-only)."""
    from philox import synthetic_actions
    a = np.stack([synthetic_actions(SEED, np.arange(B), t, _spec(cfg).n_actions) for t in range(steps)])
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _oracle(cfg, B, steps, summarized):
    """The oracle's run of envs 0 .. B - 1: {'episodes': {b: [{'steps', 'episode_nr'}]} for b in `summarized`,
    'n_episodes': {b: resets done}, 'occ': int64 [H, W] histogram of every agent's cell over every env and step}.
    Computed once, never changed."""
    import oracle as O
    import views_compare as V
    from mfg_amd import views
    spec, acts = _spec(cfg), _actions(cfg, B, steps)
    occ = np.zeros(spec.H * spec.W, np.int64)
    episodes, n_episodes = {}, {}
    for b in range(B):
        env = O.OracleEnv(spec, BASE + b)
        env.reset()
        eps, cur, nr = [], [], 1
        for t in range(steps):
            _, done, ev = env.step(acts[t, b], with_obs=False)
            assert not ev.crashed, f'{cfg}: oracle env {b} crashed at step {t}'
            np.add.at(occ, env.agents()[0], 1)
            if b in summarized:
                cur.append(views.summarize_state(spec, V.oracle_snapshot(env)))
            if done:
                if cur:
                    eps.append({'steps': cur, 'episode_nr': nr})
                cur, nr = [], nr + 1
                env.reset()
        if cur:
            eps.append({'steps': cur, 'episode_nr': nr})
        if b in summarized:
            episodes[b], n_episodes[b] = eps, nr
        env.close()
    return {'episodes': episodes, 'n_episodes': n_episodes, 'occ': occ.reshape(spec.H, spec.W)}


def _run(torch, cfg, B, steps, envs, obs_dtype='float32', **kw):
    """A BatchedEnvRecorder over a fresh BatchedFactory, reset and stepped `steps` times."""
    from mfg_amd.factory import BatchedFactory
    from mfg_amd.monitor import BatchedEnvRecorder
    bf = BatchedFactory(cfg, B, seed_base=BASE, obs_dtype=obs_dtype)
    rec = BatchedEnvRecorder(bf, envs, **kw)
    rec.reset()
    if steps:
        acts = torch.from_numpy(_actions(cfg, B, steps).copy()).to(bf.device)
        for t in range(steps):
            rec.step(acts[t])
    return rec


RECORD_CASES = [('eval_trio.yaml', 67, 60, (66, 0, 33)), ('alltest16.yaml', 67, 120, (1, 33)),
                ('logic_stress.yaml', 5, 120, (0, 1, 2)), ('agents81.yaml', 3, 40, (2,))]


@pytest.mark.parametrize('cfg,B,steps,envs', RECORD_CASES)
def test_records_equal_oracle(cfg, B, steps, envs):
    """records(env=b)['episodes'] == the oracle's per-step summarize_state split at its dones, dict for dict."""
    torch = _need_gpu()
    ref = _oracle(cfg, B, steps, frozenset(envs))
    want = ref['episodes']
    rec = _run(torch, cfg, B, steps, list(envs))
    try:
        assert rec.recorder.config['row_words'] == rec.recorder.row_words > 4
        for b in envs:
            r = rec.records(env=b)
            assert list(r) == ['episodes', 'n_episodes', 'metadata', 'header', 'crashed_steps']
            got = r['episodes']
            assert [e['episode_nr'] for e in got] == [e['episode_nr'] for e in want[b]], (cfg, b)
            for ge, we in zip(got, want[b]):
                assert len(ge['steps']) == len(we['steps']), (cfg, b, we['episode_nr'])
                for t, (gs, ws) in enumerate(zip(ge['steps'], we['steps'])):
                    assert gs == ws, (cfg, b, we['episode_nr'], t, [k for k in ws if gs.get(k) != ws[k]])
            assert r['crashed_steps'] == 0 and rec.dropped == 0
            assert r['n_episodes'] == ref['n_episodes'][b] and 'rec_step' in r['header']
            if cfg == 'eval_trio.yaml':
                assert len(want[b]) >= 3  # several episode ends per env: the split at dones is exercised
            assert sum(len(e['steps']) for e in want[b]) == steps
            assert rec.trajectory(b, want[b][0]['episode_nr']).shape == (len(want[b][0]['steps']), rec.spec.n_agents, 2)
    finally:
        rec.close()


@pytest.mark.parametrize('cfg,B,steps,envs', [('alltest16.yaml', 67, 40, (66, 1, 33)), ('agents81.yaml', 3, 20, (2, 0))])
def test_device_rows_equal_pack_row(cfg, B, steps, envs):
    """The engine stepped by hand: after each auto_reset=False step, the device rows are pack_row of export_state(),
    bit for bit (agents81: 81 agents and 65 doors, more than one 64-lane pass per row)."""
    torch = _need_gpu()
    from mfg_amd.engine import Engine, EV_MISC, RecordView, StateRecorder
    from mfg_amd.record_rows import pack_row, row_layout
    spec = _spec(cfg)
    eng = Engine(spec, B)
    dev, A = eng.device, spec.n_agents
    sr = StateRecorder(eng, list(envs), capacity=steps, occupancy=False)
    assert sr.row_words == row_layout(spec, eng.layout)['words']
    rew = torch.zeros((1, B, A), dtype=torch.float64, device=dev)
    done = torch.zeros((1, B), dtype=torch.uint8, device=dev)
    ev_a = torch.zeros((1, B, A), dtype=torch.uint8, device=dev)
    ev_w = torch.zeros((1, B, A), dtype=torch.uint8, device=dev)
    ev_m = torch.zeros((1, B, EV_MISC), dtype=torch.int32, device=dev)
    acts = torch.from_numpy(_actions(cfg, B, steps).copy()).to(dev)
    eng.reset(init=True, seed_base=BASE)
    want = {b: [] for b in envs}
    for t in range(steps):
        eng.step(1, actions=acts[t], reward=rew, done=done, ev_act=ev_a, ev_watch=ev_w, ev_misc=ev_m, auto_reset=False,
                 step_base=t)
        sr.step(acts[t], ev_a, ev_w, ev_m, done)
        state = eng.export_state().cpu().numpy()
        a, w, m, d = ev_a[0].cpu().numpy(), ev_w[0].cpu().numpy(), ev_m[0].cpu().numpy(), done[0].cpu().numpy()
        for b in envs:
            want[b].append(pack_row(RecordView(state[b], eng.layout, spec), b, _actions(cfg, B, steps)[t, b], a[b], w[b],
                                    m[b], d[b]))
        eng.reset(mask=done, init=0)
    rows, counts = sr.drain()
    sr.close()
    eng.close()
    assert list(counts) == [steps] * len(envs)
    for s, b in enumerate(envs):
        bad = [t for t in range(steps) if not np.array_equal(rows[s, t], want[b][t])]
        assert not bad, (cfg, b, bad[:5])


def _obs_parts(obs):
    return (obs,) if not hasattr(obs, 'idx') else (obs.idx, obs.val, obs.count)


@pytest.mark.parametrize('obs_dtype', ['float32', 'packed'])
@pytest.mark.parametrize('cfg,B,steps', [('eval_trio.yaml', 67, 60), ('alltest16.yaml', 67, 120)])
def test_split_step_equals_auto_reset_step(cfg, B, steps, obs_dtype):
    """BatchedEnvRecorder.step against a twin BatchedFactory.step with the same actions: obs, reward, done and the
    three event rows are equal (torch.equal) at every step over all envs."""
    torch = _need_gpu()
    from mfg_amd.factory import BatchedFactory
    rec = _run(torch, cfg, B, 0, [0], obs_dtype=obs_dtype)
    twin = BatchedFactory(cfg, B, seed_base=BASE, obs_dtype=obs_dtype)
    o0 = twin.reset()
    bad = [('reset', i) for i, (x, y) in enumerate(zip(_obs_parts(rec.obs), _obs_parts(o0))) if not torch.equal(x, y)]
    acts = torch.from_numpy(_actions(cfg, B, steps).copy()).to(twin.device)
    n_done = 0
    for t in range(steps):
        o1, r1, d1, e1 = rec.step(acts[t])
        o2, r2, d2, e2 = twin.step(acts[t])
        pairs = list(zip(_obs_parts(o1), _obs_parts(o2))) + [(r1, r2), (d1, d2)] + list(zip(e1, e2))
        bad += [(t, i) for i, (x, y) in enumerate(pairs) if not torch.equal(x, y)]
        n_done += int(d2.sum())
    rec.close()
    twin.close()
    assert not bad and n_done > 0, (cfg, obs_dtype, bad[:10], n_done)


@pytest.mark.parametrize('cfg,B,steps', [('eval_trio.yaml', 67, 60), ('agents81.yaml', 3, 40)])
def test_occupancy_equals_oracle_on_both_paths(cfg, B, steps):
    """occupation_map() == the histogram of the oracle agents' cells over every env and step, with the builder's
    choice (the LDS histogram) and with occ_lds_cells=1 (straight to global memory, and no env selected); the two
    maps are equal and mfg_record_config reports the path taken."""
    torch = _need_gpu()
    from mfg_amd.engine import OCC_GLOBAL, OCC_LDS
    summarized = {c: frozenset(e) for c, _, _, e in RECORD_CASES}[cfg]  # the records test's oracle run, shared
    want = _oracle(cfg, B, steps, summarized)['occ']
    a = _run(torch, cfg, B, steps, [0])
    b = _run(torch, cfg, B, steps, [], occ_lds_cells=1)
    try:
        ca, cb = a.recorder.config, b.recorder.config
        assert ca['occ_path'] == OCC_LDS and ca['occ_lds_bytes'] == 4 * want.size
        assert cb['occ_path'] == OCC_GLOBAL and cb['occ_lds_bytes'] == 0 and cb['n_sel'] == 0 and cb['row_grid'] == 0
        assert ca['occ_grid'] == cb['occ_grid'] == -(-B // ca['occ_envs']) and (B < 64 or ca['occ_grid'] > 1)
        ma, mb = a.occupation_map(), b.occupation_map()
        assert ma.dtype == np.int64 and ma.shape == want.shape
        assert int(want.sum()) == B * steps * a.spec.n_agents
        assert np.array_equal(ma, want) and np.array_equal(mb, want) and np.array_equal(ma, mb)
        b.clear_occupation()
        assert not b.occupation_map().any() and np.array_equal(a.occupation_map(), want)
    finally:
        a.close()
        b.close()


def test_occupancy_equals_env_recorder_of_one_factory():
    """B = 1, envs = [0]: the map equals EnvRecorder.occupation_map() of a Factory('eval_trio.yaml', py_seed=40)
    stepped alike. The reference recorder forgets its episodes at every reset(), so its map is taken at each episode
    end and summed over three episodes."""
    torch = _need_gpu()
    from philox import synthetic_actions
    from mfg_amd.factory import Factory
    from mfg_amd.monitor import EnvRecorder
    cfg = 'eval_trio.yaml'
    er = EnvRecorder(Factory(cfg, py_seed=BASE))
    want, t = 0, 0
    for _ in range(3):
        er.reset()
        done = False
        while not done:
            act = synthetic_actions(SEED, np.arange(1), t, er.spec.n_actions)[0]
            done = er.step([int(x) for x in act])[3]
            t += 1
            assert t < 500
        want = want + er.occupation_map()
    er.close()
    rec = _run(torch, cfg, 1, t, [0])
    try:
        got = rec.occupation_map()
        assert int(got.sum()) == t * rec.spec.n_agents and np.array_equal(got, want)
        assert [e['episode_nr'] for e in rec.records(env=0)['episodes']] == [1, 2, 3]
    finally:
        rec.close()


def test_ring_capacity_and_episode_filter():
    """eval_trio, B = 67, 60 steps, envs [66, 0, 33]: capacity 7 (a drain every 7 steps) gives the records of
    capacity 64; without draining, capacity 7 keeps the first 7 rows and drops 53 per env; episodes=[2, 4] records
    only those episode numbers."""
    torch = _need_gpu()
    cfg, B, steps, envs = RECORD_CASES[0]
    want = _oracle(cfg, B, steps, frozenset(envs))['episodes']
    big = _run(torch, cfg, B, steps, list(envs), capacity=64)
    small = _run(torch, cfg, B, steps, list(envs), capacity=7)
    lossy = _run(torch, cfg, B, steps, list(envs), capacity=7, auto_drain=False)
    some = _run(torch, cfg, B, steps, list(envs), episodes=[2, 4])
    try:
        for b in envs:
            eb, es = big.records(env=b)['episodes'], small.records(env=b)['episodes']
            assert eb == want[b] and es == eb, (b, 'capacity')
            rows_full = big.rows(b)
            assert rows_full.shape == (steps, big.recorder.row_words)
            assert np.array_equal(small.rows(b), rows_full)
            kept = lossy.rows(b)
            assert kept.shape[0] == 7 and np.array_equal(kept, rows_full[:7])
            assert lossy.dropped_by_env[b] == 53
            pick = [e for e in want[b] if e['episode_nr'] in (2, 4)]
            assert len(pick) == 2 and some.records(env=b)['episodes'] == pick, (b, 'filter')
        assert lossy.dropped == 53 * len(envs) and big.dropped == small.dropped == some.dropped == 0
    finally:
        for r in (big, small, lossy, some):
            r.close()
