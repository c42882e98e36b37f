"""GPU: the paths that end an env abnormally, engine against oracle. Every crash config (tests/crash_cases.py; its
reasons are pinned against the reference's exceptions by the crash fixtures, and the conditions that keep these tests
from passing vacuously by tests/test_crash_paths.py) runs B = 64 envs for 100 steps of Philox actions with and without
auto-reset; every env is compared on every step with its own oracle env: rewards with ==, done, the act / watch rows,
the whole ev_misc row (crashed bit and reason, done mask, step, episode, collisions), the obs of every env that did not
crash on that step (after an auto-reset: the new episode's first obs), and at the end the MT state and floor order.
The capacity path: on the serpentine the engine reports MFG_CRASH_CAPACITY where the oracle hands out a route longer
than the stored path, never MFG_CRASH_ROUTE."""
import numpy as np
import pytest

from conftest import gpu_available
import crash_cases as CC
from mfg_amd.engine import EV_MISC

pytestmark = pytest.mark.gpu

_oracle_runs = {}


def _oracle(cfg, base, n, steps, auto_reset):
    """One oracle run per case, shared by the tests that compare against it (never modified)."""
    key = (cfg, base, n, steps, auto_reset)
    if key not in _oracle_runs:
        from mfg_amd.spec import compile_spec
        spec = compile_spec(cfg)
        run, envs = CC.oracle_run(spec, base, n, steps, auto_reset=auto_reset, with_obs=True)
        run['mt'] = np.stack([e.mt_state() for e in envs])
        run['floor'] = np.stack([e.floor() for e in envs])
        for e in envs:
            e.close()
        _oracle_runs[key] = run
    return _oracle_runs[key]


def _engine_run(cfg, base, n, steps, auto_reset, K=1):
    """The engine on the same envs: K fused steps per call (the last call takes what is left). Without auto-reset an
    env that finished without a crash is reset by hand (mfg_reset with a mask), as the oracle run does; a crashed env
    is left as it is and keeps reporting crashed + done."""
    if not gpu_available():
        pytest.skip('no GPU')
    import torch
    from mfg_amd.spec import compile_spec
    from mfg_amd.engine import Engine, RecordView
    spec = compile_spec(cfg)
    eng = Engine(spec, n)
    A, dev = spec.n_agents, eng.device
    assert K == 1 or auto_reset
    obs0 = torch.zeros(eng.obs_shape(), dtype=torch.float64, device=dev)
    eng.reset(obs=obs0, init=True, seed_base=base)
    out = dict(first=obs0.cpu().numpy().copy(), reward=[], done=[], act=[], watch=[], misc=[], obs=[])
    t = 0
    while t < steps:
        k = min(K, steps - t)
        obs = torch.zeros(eng.obs_shape(k), dtype=torch.float64, device=dev) if K > 1 else obs0[None]
        rew = torch.zeros((k, n, A), dtype=torch.float64, device=dev)
        done = torch.zeros((k, n), dtype=torch.uint8, device=dev)
        ev_a = torch.zeros((k, n, A), dtype=torch.uint8, device=dev)
        ev_w = torch.zeros((k, n, A), dtype=torch.uint8, device=dev)
        ev_m = torch.zeros((k, n, EV_MISC), dtype=torch.int32, device=dev)
        # Engine.step raises unless mfg_step returns 0: a crashed env is reported in the rows, never as a failed call
        eng.step(k, actions=None, philox_seed=CC.PHILOX_SEED, step_base=t, reward=rew, done=done, obs=obs,
                 ev_act=ev_a, ev_watch=ev_w, ev_misc=ev_m, auto_reset=auto_reset)
        if not auto_reset:
            crashed = (ev_m[0, :, 6] >> 1) & 1
            mask = ((done[0] != 0) & (crashed == 0)).to(torch.uint8)
            if int(mask.sum()):
                eng.reset(obs=obs0, mask=mask)
        out['reward'].append(rew.cpu().numpy())
        out['done'].append(done.cpu().numpy())
        out['act'].append(ev_a.cpu().numpy())
        out['watch'].append(ev_w.cpu().numpy())
        out['misc'].append(ev_m.cpu().numpy().astype(np.int64) & 0xFFFFFFFF)
        out['obs'].append(obs.cpu().numpy().copy())
        t += k
    for key in ('reward', 'done', 'act', 'watch', 'misc', 'obs'):
        out[key] = np.concatenate(out[key])
    st = eng.export_state().cpu().numpy()
    views = [RecordView(st[i], eng.layout, spec) for i in range(n)]
    out['mt'] = np.stack([v.mt() for v in views])
    out['floor'] = np.stack([v.perm() for v in views])
    out['layout'] = dict(eng.layout)
    eng.close()
    return spec, out


def _first_diff(name, got, want):
    bad = np.argwhere(got != want)
    assert not len(bad), f'{name}: {len(bad)} differ, first at [step, env, ...] {bad[0].tolist()}: engine ' \
                         f'{got[tuple(bad[0])]} oracle {want[tuple(bad[0])]}'


def _compare(spec, got, ref, steps=None, envs=None):
    """Every step row of every env (or of `envs`, up to `steps[i]` steps of env i), then the obs."""
    n = got['done'].shape[1]
    envs = range(n) if envs is None else envs
    nl, A = spec.n_layers, spec.n_agents
    for i in envs:
        T = got['done'].shape[0] if steps is None else steps[i]
        for a in range(A):
            assert (got['first'][i, a, :nl[a]] == ref['first'][i][a]).all(), f'reset obs env {i} agent {a}'
        for name in ('reward', 'done', 'act', 'watch', 'misc'):
            _first_diff(f'{name} env {i}', got[name][:T, i], ref[name][:T, i])
        for t in range(T):
            if ref['obs'][t][i] is None:
                continue
            for a in range(A):
                assert (got['obs'][t, i, a, :nl[a]] == ref['obs'][t][i][a]).all(), f'obs t{t} env {i} agent {a}'


def _flags(run):
    f = run['misc'][:, :, 6]
    return (f >> 1) & 1, (f >> 8) & 0xFF


@pytest.mark.parametrize('auto_reset', [True, False])
@pytest.mark.parametrize('cfg,base,targets', CC.STEP_CASES + CC.ALWAYS_CASES)
def test_engine_vs_oracle_across_crashes(cfg, base, targets, auto_reset):
    ref = _oracle(cfg, base, CC.B, CC.STEPS, auto_reset)
    spec, got = _engine_run(cfg, base, CC.B, CC.STEPS, auto_reset)
    crashed, reason = _flags(ref)
    for r in targets:  # the run reaches what it is meant to compare (tests/test_crash_paths.py counts the envs)
        assert (reason == r).any()
    if not auto_reset:  # a crashed env that is not reset takes no step: crashed + done with the same reason, no reward
        for i in range(CC.B):
            t0 = np.flatnonzero(crashed[:, i])
            if len(t0):
                assert (crashed[t0[0]:, i] == 1).all() and (reason[t0[0]:, i] == reason[t0[0], i]).all()
                assert (ref['reward'][t0[0] + 1:, i] == 0).all() and (ref['act'][t0[0] + 1:, i] == 0).all()
    _compare(spec, got, ref)
    # post-crash resets consumed the RNG as the oracle's did
    _first_diff('final MT state', got['mt'], ref['mt'])
    _first_diff('final floor order', got['floor'], ref['floor'])


def test_fused_steps_report_the_same_rows_across_crashes():
    """K = 8 fused steps per call (crashes and their auto-resets inside a call) give the rows of eight K = 1 calls."""
    cfg, base, _ = CC.STEP_CASES[2]  # crash_nofree: reasons 3, 4 and 5, several crashes per env
    ref = _oracle(cfg, base, CC.B, CC.STEPS, True)
    spec, one = _engine_run(cfg, base, CC.B, CC.STEPS, True, K=1)
    spec, fused = _engine_run(cfg, base, CC.B, CC.STEPS, True, K=8)
    assert _flags(ref)[0].sum() > CC.B  # crashes inside the fused calls
    for name in ('first', 'reward', 'done', 'act', 'watch', 'misc', 'obs', 'mt', 'floor'):  # every crash resets here,
        _first_diff(f'K=8 vs K=1 {name}', fused[name], one[name])                            # so every obs row is defined
    _compare(spec, fused, ref)


@pytest.mark.parametrize('auto_reset', [True, False])
@pytest.mark.parametrize('cfg,base', CC.RESET_CASES)
def test_reset_crash_reports_crashed_and_done_on_every_step(cfg, base, auto_reset):
    ref = _oracle(cfg, base, CC.B, 20, auto_reset)
    spec, got = _engine_run(cfg, base, CC.B, 20, auto_reset)
    crashed, reason = _flags(got)
    assert (crashed == 1).all() and (reason == CC.RULE).all() and (got['done'] == 1).all()
    assert (got['reward'] == 0).all()
    for name in ('reward', 'done', 'act', 'watch', 'misc'):
        _first_diff(name, got[name], ref[name])
    _first_diff('final MT state', got['mt'], ref['mt'])
    _first_diff('final floor order', got['floor'], ref['floor'])


def _serpentine_oracle():
    """The serpentine on the oracle, which has no path limit: rows, obs, and per env the first step on which
    calculate_route stored a path longer than the engine's path_cap (None: never within the run)."""
    key = 'serpentine'
    if key not in _oracle_runs:
        import oracle as O
        from philox import synthetic_actions
        from mfg_amd.spec import compile_spec
        cfg, base, n, steps = CC.SERPENTINE
        spec = compile_spec(cfg)
        cap = CC.path_cap(spec)
        A = spec.n_agents
        envs = [O.OracleEnv(spec, base + i) for i in range(n)]
        run = dict(first=[e.reset() for e in envs], reward=np.zeros((steps, n, A)), done=np.zeros((steps, n), np.uint8),
                   act=np.zeros((steps, n, A), np.uint8), watch=np.zeros((steps, n, A), np.uint8),
                   misc=np.zeros((steps, n, 16), np.int64), obs=[[None] * n for _ in range(steps)], over=[None] * n)
        for t in range(steps):
            acts = synthetic_actions(CC.PHILOX_SEED, np.arange(n), t, spec.n_actions)
            for i, e in enumerate(envs):
                r, d, ev = e.step(acts[i])
                assert not ev.crashed and not d
                run['reward'][t, i], run['done'][t, i] = r, d
                run['act'][t, i], run['watch'][t, i] = list(ev.act[:A]), list(ev.watch[:A])
                run['misc'][t, i] = CC.misc_row(ev) & 0xFFFFFFFF
                run['obs'][t][i] = e.obs_list()
                if run['over'][i] is None and e.maint_route_len(0) > cap:
                    run['over'][i] = t
        for e in envs:
            e.close()
        _oracle_runs[key] = (spec, run)
    return _oracle_runs[key]


def test_route_longer_than_path_cap_is_engine_capacity():
    """Up to the step that asks for a route over path_cap the engine equals the oracle; that step reports crashed +
    done with MFG_CRASH_CAPACITY (not MFG_CRASH_ROUTE: the reference finds the route and keeps running), the env stays
    flagged, and the envs whose routes fit run the whole length equal to the oracle."""
    cfg, base, n, steps = CC.SERPENTINE
    spec, ref = _serpentine_oracle()
    over = ref['over']
    assert sum(t is not None for t in over) >= 1
    spec, got = _engine_run(cfg, base, n, steps, False)
    # the stored paths (u16 cells, kmax * path_cap per env) end where the rank table starts: path_cap as the layout has it
    lay = got['layout']
    assert (lay['o_grank'] - lay['o_mpath']) // 2 >= CC.path_cap(spec)
    crashed, reason = _flags(got)
    _compare(spec, got, ref, steps=[steps if t is None else t for t in over])
    for i, t in enumerate(over):
        if t is None:
            assert not crashed[:, i].any(), f'env {i} crashed though every route fits'
        else:
            assert (crashed[t:, i] == 1).all() and (got['done'][t:, i] == 1).all(), f'env {i} step {t}'
            assert (reason[t:, i] == CC.CAPACITY).all(), f'env {i} step {t}: reason {reason[t:, i]}'


def test_factory_step_names_the_crash_reason():
    """Factory.step (mfg_amd/factory.py) names the reason: 'engine capacity' on the serpentine, where the reference
    keeps running, and 'the reference crashes' only for reasons 1 to 6."""
    if not gpu_available():
        pytest.skip('no GPU')
    from mfg_amd.factory import Factory
    cfg, base, n, steps = CC.SERPENTINE
    spec, ref = _serpentine_oracle()
    i = next(i for i, t in enumerate(ref['over']) if t == 0)  # the first route already exceeds the cap
    from philox import synthetic_actions
    act = synthetic_actions(CC.PHILOX_SEED, np.arange(n), 0, spec.n_actions)[i]  # the step the oracle run took
    env = Factory(cfg, py_seed=base + i)
    env.reset()
    with pytest.raises(RuntimeError, match='engine capacity') as ex:
        env.step([int(x) for x in act])
    env.close()
    assert 'reason 7' in str(ex.value) and 'the reference crashes' not in str(ex.value)
    from mfg_amd.factory import crash_message
    from mfg_amd import abi
    for r in range(1, 7):
        assert 'the reference crashes' in crash_message(r) and abi.CRASH_NAMES[r] in crash_message(r)
