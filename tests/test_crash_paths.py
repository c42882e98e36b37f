"""CPU: the conditions that keep the crash-path GPU tests (tests/test_gpu_crash_paths.py) from passing vacuously,
checked on the C oracle alone: in the seed range each case uses, every reason it targets occurs in at least 3 envs and
at least 3 envs run the whole length without a crash; the reset-crash configs crash on every step; the serpentine hands
out a route longer than the engine's stored path. The oracle's reasons themselves are pinned against the reference's
exceptions by the crash fixtures (tests/test_oracle.py)."""
import numpy as np
import pytest

import crash_cases as CC


def _reasons(run):
    """Per env: the set of crash reasons its steps reported."""
    flags = run['misc'][:, :, 6]
    crashed, reason = (flags >> 1) & 1, (flags >> 8) & 0xFF
    assert ((reason != 0) == (crashed != 0)).all()  # a reason exactly where the crashed bit is set
    assert (run['done'][crashed != 0] == 1).all()  # a crashed step reports done
    return [set(int(x) for x in reason[:, i][crashed[:, i] != 0]) for i in range(flags.shape[1])]


@pytest.mark.parametrize('cfg,base,targets', CC.STEP_CASES)
def test_every_targeted_reason_occurs_and_some_envs_run_clean(cfg, base, targets):
    from mfg_amd.spec import compile_spec
    spec = compile_spec(cfg)
    run, envs = CC.oracle_run(spec, base, CC.B, CC.STEPS)
    per_env = _reasons(run)
    counts = {r: sum(1 for s in per_env if r in s) for r in sorted(set().union(*per_env))}
    clean = sum(1 for s in per_env if not s)
    print(f'{cfg} base {base}: envs per reason {counts}, clean envs {clean}')
    for r in targets:
        assert counts.get(r, 0) >= 3, (cfg, r, counts)
    assert clean >= 3, (cfg, clean)
    assert CC.CAPACITY not in counts and CC.ACTION not in counts  # the oracle has no capacity, the actions are in range


@pytest.mark.parametrize('cfg,base,targets', CC.ALWAYS_CASES)
def test_always_crashing_config_crashes_in_every_env(cfg, base, targets):
    from mfg_amd.spec import compile_spec
    spec = compile_spec(cfg)
    run, envs = CC.oracle_run(spec, base, CC.B, CC.STEPS)
    per_env = _reasons(run)
    assert all(s == set(targets) for s in per_env), per_env[:4]
    crashed = (run['misc'][:, :, 6] >> 1) & 1
    assert (crashed.sum(0) >= 3).all() and (crashed.sum(0) < CC.STEPS).all()  # several episodes, not every step


@pytest.mark.parametrize('cfg,base', CC.RESET_CASES)
def test_reset_crash_reports_crashed_and_done_on_every_step(cfg, base):
    from mfg_amd.spec import compile_spec
    spec = compile_spec(cfg)
    for auto_reset in (True, False):
        run, envs = CC.oracle_run(spec, base, CC.B, 20, auto_reset=auto_reset)
        flags = run['misc'][:, :, 6]
        assert (((flags >> 1) & 1) == 1).all() and (((flags >> 8) & 0xFF) == CC.RULE).all()
        assert (run['done'] == 1).all() and (run['reward'] == 0).all()
        assert (run['misc'][:, :, 8] == np.arange(1, 21)[:, None]).all() == (not auto_reset)  # curr_step goes on


def test_serpentine_route_exceeds_the_engine_path_cap():
    """Within 60 steps the oracle hands out a route longer than path_cap (the engine's stored path) in every env of
    the range, and its longest has several hundred nodes."""
    from mfg_amd.spec import compile_spec
    import oracle as O
    from philox import synthetic_actions
    cfg, base, n, steps = CC.SERPENTINE
    spec = compile_spec(cfg)
    cap = CC.path_cap(spec)
    assert cap == 4 * (41 + 41) == 328 and spec.c.n_floor > 2 * cap
    envs = [O.OracleEnv(spec, base + i) for i in range(n)]
    for e in envs:
        e.reset()
    first_over, longest = {}, 0
    for t in range(steps):
        acts = synthetic_actions(CC.PHILOX_SEED, np.arange(n), t, spec.n_actions)
        for i, e in enumerate(envs):
            _, d, ev = e.step(acts[i], with_obs=False)
            assert not ev.crashed and not d
            # the stored path is route[1:]: the engine keeps it while len(route) - 1 <= path_cap
            k = e.maint_route_len(0)
            assert 0 <= e.maint_path_len(0) <= k
            longest = max(longest, k)
            if k > cap:
                first_over.setdefault(i, t)
    print(f'serpentine41: path_cap {cap}, longest stored path {longest}, first step over the cap per env {first_over}')
    assert len(first_over) >= 1 and longest > cap


def test_reason_table():
    assert CC.expected_reason('NetworkXNoPath: No path between (1, 1) and (2, 9).', '_bidirectional_pred_succ') == 2
    assert CC.expected_reason('NodeNotFound: x', 'bidirectional_shortest_path') == 2
    assert CC.expected_reason('IndexError: list index out of range', 'random_free_position') == 3
    assert CC.expected_reason('IndexError: pop from empty list', 'get_move_action') == 4
    assert CC.expected_reason('IndexError: list index out of range', '_predict_move') == 5
    assert CC.expected_reason("AttributeError: 'list' object has no attribute 'do_wait_action'") == 1
    assert CC.expected_reason("KeyError: 'Noop'", 'tick_step') == 1
    assert CC.expected_reason('IndexError: pop from empty list', 'on_reset') == 1
