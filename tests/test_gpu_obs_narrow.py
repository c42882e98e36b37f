"""The folded render's one-word cell and layer records (csrc/mfg_kernels.h build_obs, NARROW: specs with at most 16
agents) against the C oracle, against the same render with three-word records (mfg_variant.obs_wide_records) and
against the generic render (obs_generic).

Each case runs the three engines in lockstep on the Philox actions, B = 8 envs for 40 steps of 12-step episodes (three
resets, so the frozen ray origin, battery and position are rendered): every step's obs bit for bit against the oracle
and byte for byte between the engines (padding layers included), rewards, done and events as test_gpu_obs_geo does.
The oracle run of a config is computed once and shared by its cases; what it must contain for the cases to mean
anything (both door values, a battery value at cell 0, both position values, a Combined count of 2, a 1 in the last
agent's layer) is asserted on the oracle alone, without a GPU.

narrow16 / narrow17 are the agent limit of the one-word records. They cannot carry Battery or GlobalPosition layers: the
reference's Batteries and GlobalPositions groups hold pomdp_r^2 + 1 agents (10 at pomdp_r 3, spec.py Q16), so those
layers, first and last in the block, are narrow_ends.yaml's (10 agents)."""
import functools

import numpy as np
import pytest

from conftest import gpu_available
from mfg_amd.engine import EV_MISC

B, STEPS, BASE, PSEED = 8, 40, 1000, 7


@functools.lru_cache(maxsize=None)
def _oracle_run(cfg):
    """(spec, reset obs [B][A] arrays, per step: rewards [B][A], done [B], events [B], obs [B][A] arrays (after the
    auto-reset where the episode ended))."""
    import oracle as O
    from philox import synthetic_actions
    from mfg_amd.spec import compile_spec
    spec = compile_spec(cfg)
    A = spec.n_agents
    envs = [O.OracleEnv(spec, BASE + i) for i in range(B)]
    obs0 = [e.reset() for e in envs]
    steps = []
    for t in range(STEPS):
        acts = synthetic_actions(PSEED, np.arange(B), t, spec.n_actions)
        rew, done, evs, obs = [], [], [], []
        for i, env in enumerate(envs):
            r, d, ev = env.step(acts[i])
            rew.append(list(r))
            done.append(d)
            evs.append((list(ev.act[:A]), list(ev.watch[:A]), ev.door_coll, ev.door_coll_hi, ev.maint_coll))
            obs.append(env.reset() if d else env.obs_list())
        steps.append((rew, done, evs, obs))
    for e in envs:
        e.close()
    return spec, obs0, steps


def _all_obs(cfg):
    spec, obs0, steps = _oracle_run(cfg)
    yield from obs0
    for _, _, _, obs in steps:
        yield from obs


def _layer(spec, a, name):
    return spec.layer_names[a].index(name)


def _seen(cfg):
    """What the oracle's own obs hold over the run, of the values the render cases are about."""
    spec, _, steps = _oracle_run(cfg)
    A = spec.n_agents
    last = f'Agent[{spec.agent_names[A - 1]}]'
    seen = dict(closed=False, open=False, battery=False, gpx=False, gpy=False, comb2=False, last_agent=False)
    for env_obs in _all_obs(cfg):
        for a in range(A):
            o, names = env_obs[a], spec.layer_names[a]
            doors = o[names.index('Doors')]
            seen['closed'] |= bool((doors == 0.6666).any())
            seen['open'] |= bool((doors == 0.4444).any())
            if 'Battery' in names:
                assert names[0] == 'Battery' and names[-1] == 'GlobalPosition', 'a special value at each end of the block'
                seen['battery'] |= bool(o[0].flat[0] != 0.0 and not o[0].flat[1:].any())
                seen['gpx'] |= bool(o[-1].flat[0] != 0.0)
                seen['gpy'] |= bool(o[-1].flat[1] != 0.0 and not o[-1].flat[2:].any())
            seen['comb2'] |= bool((o[[n.startswith('Combined(') for n in names].index(True)] >= 2.0).any())
            if last in names:
                seen['last_agent'] |= bool((o[names.index(last)] == 1.0).any())
    assert sum(d for _, done, _, _ in steps for d in done) >= 3 * B, 'three resets per env'
    return seen


@pytest.mark.parametrize('cfg', ['narrow16.yaml', 'narrow17.yaml'])
def test_oracle_run_at_the_agent_limit_is_not_vacuous(cfg):
    """Both door values, a Combined count of 2 and a 1 in the last agent's layer. (The reference's Batteries and
    GlobalPositions groups hold pomdp_r^2 + 1 agents, so 16 agents cannot have those layers: narrow_ends has them.)"""
    seen = _seen(cfg)
    assert all(seen[k] for k in ('closed', 'open', 'comb2', 'last_agent')), seen


def test_oracle_run_with_special_values_at_the_ends_is_not_vacuous():
    """Battery first and GlobalPosition last: a nonzero battery value at cell 0 and both position values, beside both
    door values, a Combined count of 2 and the last agent's layer."""
    seen = _seen('narrow_ends.yaml')
    assert all(seen.values()), seen


def test_oracle_run_ordered_is_not_vacuous():
    """narrow_ordered: Karl's ordered Combined holds unit members and both door values; Manfred has two Doors layers."""
    cfg = 'narrow_ordered.yaml'
    spec, _, _ = _oracle_run(cfg)
    vals = set()
    for a in (0, 1):  # the two Karls
        comb = _layer(spec, a, f'Combined(Agent[{spec.agent_names[a]}])')
        for env_obs in _all_obs(cfg):
            vals |= set(np.unique(env_obs[a][comb]).tolist())
    assert 1.0 in vals and 0.6666 in vals and 0.4444 in vals, vals
    assert [n.count('Doors') for n in spec.layer_names] == [1, 1, 1, 2, 2]


def _buffers(torch, eng, K, odt):
    A, dev = eng.A, eng.device
    return dict(obs=torch.zeros((K,) + eng.obs_shape(), dtype=odt, device=dev),
                reward=torch.zeros((K, B, A), dtype=torch.float64, device=dev),
                done=torch.zeros((K, B), dtype=torch.uint8, device=dev),
                ev_act=torch.zeros((K, B, A), dtype=torch.uint8, device=dev),
                ev_watch=torch.zeros((K, B, A), dtype=torch.uint8, device=dev),
                ev_misc=torch.zeros((K, B, EV_MISC), dtype=torch.int32, device=dev))


def _lockstep(cfg, K, f32, narrow):
    if not gpu_available():
        pytest.skip('no GPU')
    import torch
    from mfg_amd.engine import Engine, events_from_rows
    spec, ref0, ref_steps = _oracle_run(cfg)
    A, nl, r = spec.n_agents, spec.n_layers, spec.c.pomdp_r
    names = ('selected', 'obs_wide_records', 'obs_generic')
    engs = [Engine(spec, B), Engine(spec, B, variant={'obs_wide_records': 1}),
            Engine(spec, B, variant={'obs_generic': 1})]
    try:
        assert [e.layout['obs_narrow'] for e in engs] == [narrow, 0, 0], 'one-word records: the selected render only'
        assert [e.layout['obs_geo_r'] for e in engs] == [r, r, 0], 'the folded render, whatever its records'
        odt = np.float32 if f32 else np.float64
        ubits = np.uint32 if f32 else np.uint64
        bufs = [_buffers(torch, e, K, torch.float32 if f32 else torch.float64) for e in engs]

        def check_obs(got_all, want_all, what):
            for i in range(B):
                for a in range(A):
                    got, want = got_all[i, a, :nl[a]], want_all[i][a].astype(odt)
                    if not (got.view(ubits) == want.view(ubits)).all():
                        dif = np.argwhere(got != want)
                        raise AssertionError(f'{what} env{i} agent{a} obs: {len(dif)} diffs, first '
                                             f'{[(tuple(x), got[tuple(x)], want[tuple(x)]) for x in dif[:6]]} '
                                             f'layers {spec.layer_names[a]}')

        obs0 = []
        for eng, buf in zip(engs, bufs):
            eng.reset(obs=buf['obs'][0], init=True, seed_base=BASE)
            obs0.append(buf['obs'][0].cpu().numpy())
        for n, o in zip(names[1:], obs0[1:]):
            assert obs0[0].tobytes() == o.tobytes(), f'reset obs: selected render vs {n}'
        check_obs(obs0[0], ref0, 'reset')
        for t0 in range(0, STEPS, K):
            out = []
            for eng, buf in zip(engs, bufs):
                eng.step(K, actions=None, philox_seed=PSEED, step_base=t0, auto_reset=True, **buf)
                out.append({k: v.cpu().numpy() for k, v in buf.items()})
            for n, other in zip(names[1:], out[1:]):
                for k in ('obs', 'reward', 'done', 'ev_act', 'ev_watch', 'ev_misc'):
                    assert out[0][k].tobytes() == other[k].tobytes(), f't{t0} {k}: selected render vs {n}'
            o = out[0]
            for k in range(K):
                t = t0 + k
                rew, done, evs, obs = ref_steps[t]
                for i in range(B):
                    assert list(o['reward'][k, i]) == rew[i], f't{t} env{i} reward'
                    assert bool(o['done'][k, i]) == done[i], f't{t} env{i} done'
                    ev = events_from_rows(o['ev_act'][k, i], o['ev_watch'][k, i], o['ev_misc'][k, i])
                    assert (list(ev['act'][:A]), list(ev['watch'][:A]), ev['door_coll'], ev['door_coll_hi'],
                            ev['maint_coll']) == evs[i], f't{t} env{i} events'
                check_obs(o['obs'][k], obs, f't{t}')
    finally:
        for e in engs:
            e.close()


@pytest.mark.gpu
@pytest.mark.parametrize('K', [1, 8])
@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
@pytest.mark.parametrize('cfg,narrow', [('narrow16.yaml', 1), ('narrow17.yaml', 0), ('narrow_ends.yaml', 1)])
def test_narrow_and_wide_records_at_the_agent_limit(cfg, narrow, f32, K):
    """16 agents: the last agent is the top bit of the one-word records' agent field; 17: the first count that keeps
    the three-word records (obs_narrow 0), still on the folded render (obs_geo_r the radius); narrow_ends: the
    battery and position values at the two ends of every agent's block."""
    _lockstep(cfg, K, f32, narrow)


@pytest.mark.gpu
@pytest.mark.parametrize('K', [1, 8])
@pytest.mark.parametrize('f32', [False, True], ids=['f64', 'f32'])
def test_flagged_layers_on_narrow_records(f32, K):
    """An ordered Combined layer with a Doors member (the member loop reads tags and agents out of the one-word cell),
    an agent with two Doors layers, Battery and GlobalPosition in every position of the block."""
    _lockstep('narrow_ordered.yaml', K, f32, 1)
