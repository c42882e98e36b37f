"""The crash-path cases shared by the oracle (CPU) and engine (GPU) tests: which reference exception belongs to which
MFG_CRASH_* reason (include/mfg.h), the configs that reach each reason, and the helpers that run oracle envs."""
import numpy as np

# MFG_CRASH_* (include/mfg.h)
RULE, ROUTE, NO_FREE, NEXT_EMPTY, PATH_EMPTY, MOVE, CAPACITY, ACTION = 1, 2, 3, 4, 5, 6, 7, 8

# reference fixtures of the crash configs: (tag, config); tools/gen_golden.py --config <config> --level <its level>
FIXTURES = [('crash_route', 'crash_route.yaml'), ('crash_line', 'crash_line.yaml'),
            ('crash_nofree', 'crash_nofree.yaml'), ('crash_reset_agents', 'crash_reset_agents.yaml'),
            ('crash_reset_positions', 'crash_reset_positions.yaml'), ('crash_rule_items', 'crash_rule_items.yaml'),
            ('crash_rule_battery', 'crash_rule_battery.yaml')]


def expected_reason(message, site=None):
    """The reason that belongs to a recorded reference exception: message is the fixture's '<Type>: <text>', site the
    name of the function that raised (fixtures from before the site was recorded carry none).
    'list index out of range' is raised at two places of Maintainer.get_move_action's step: random_free_position on a
    level without a free cell, and _predict_move reading self._path[0] after both route targets were the maintainer's
    own cell; the site tells them apart."""
    kind = message.split(':', 1)[0]
    if kind in ('NetworkXNoPath', 'NodeNotFound'):
        return ROUTE
    if kind == 'IndexError' and 'list index out of range' in message and site == 'random_free_position':
        return NO_FREE
    if kind == 'IndexError' and 'pop from empty list' in message and site == 'get_move_action':
        return NEXT_EMPTY
    if kind == 'IndexError' and 'list index out of range' in message and site == '_predict_move':
        return PATH_EMPTY
    return RULE


# Batched cases (tests/test_gpu_crash_paths.py; their conditions are checked on the oracle alone by
# tests/test_crash_paths.py): config, seed base, the reasons the config targets. B = 64 envs seeded base + i, Philox
# seed 7, 100 steps with auto-reset. Counted on the oracle with these bases:
#   crash_route        base 1000: reason 2 in 34 envs, reason 4 in 11, 26 envs never crash
#   crash_line         base 1000: reason 4 in 53 envs, reason 5 in 42, 11 envs never crash
#   crash_nofree       base 2000: reason 3 in 54 envs, reason 4 in 32, reason 5 in 61, 3 envs never crash
#   crash_rule_battery base 1000: reason 1 in 39 envs, 25 envs never crash
B, PHILOX_SEED, STEPS = 64, 7, 100
STEP_CASES = [('crash_route.yaml', 1000, (ROUTE,)),
              ('crash_line.yaml', 1000, (NEXT_EMPTY, PATH_EMPTY)),
              ('crash_nofree.yaml', 2000, (NO_FREE, NEXT_EMPTY, PATH_EMPTY)),
              ('crash_rule_battery.yaml', 1000, (RULE,))]
# Configs where every env crashes by construction, so no env runs clean: the two whose reset() raises (every step of
# every env reports crashed + done), and crash_rule_items (the RespawnItems counter runs out once and is never reset:
# step 3 of the first episode and the first step of every later one crash, in every env).
RESET_CASES = [('crash_reset_agents.yaml', 1000), ('crash_reset_positions.yaml', 1000)]
ALWAYS_CASES = [('crash_rule_items.yaml', 1000, (RULE,))]

# Capacity: the serpentine's routes against the engine's stored path
SERPENTINE = ('serpentine41.yaml', 1000, 8, 60)  # config, seed base, envs, steps


def path_cap(spec):
    """The engine's stored-path limit from its inputs (csrc/mfg_engine.hip): min(4 (H + W), n_floor, 1000)."""
    return min(4 * (spec.H + spec.W), int(spec.c.n_floor), 1000)


def misc_row(ev):
    """An oracle step's events as the engine's ev_misc row (MFG_EVM_*, include/mfg.h)."""
    m = np.zeros(16, np.int64)
    m[0], m[1] = ev.door_coll & 0xFFFFFFFF, ev.door_coll >> 32
    m[2], m[3], m[4], m[5] = ev.respawn_items_value, ev.dirt_spawn_value, ev.dirt_spawn_valid, ev.dest_reached
    m[6] = (1 if ev.door_autoclose else 0) | (2 if ev.crashed else 0) | (ev.crash_reason << 8)
    m[7], m[8], m[9] = ev.done_mask & 0xFFFFFFFF, ev.step, ev.episode
    m[10], m[11] = ev.maint_coll & 0xFFFFFFFF, ev.maint_base
    m[12], m[13] = ev.door_coll_hi & 0xFFFFFFFF, ev.door_coll_hi >> 32
    m[14] = ev.maint_coll >> 32
    return m


def oracle_run(spec, base, n_envs, steps, auto_reset=True, seed=PHILOX_SEED, with_obs=False):
    """n_envs oracle envs seeded base + i stepped with the engine's Philox actions. Returns per step and env: reward
    [T, B, A], done [T, B], act / watch [T, B, A], misc [T, B, 16] (as u32 words) and, with_obs, the obs lists after
    the step (after the reset where the env was done: every done env with auto_reset, else only those that finished
    without a crash; None where the env has crashed and was not reset); and the envs (open: the caller reads their
    final state)."""
    import oracle as O
    from philox import synthetic_actions
    A = spec.n_agents
    envs = [O.OracleEnv(spec, base + i) for i in range(n_envs)]
    first = [e.reset() for e in envs]
    rew = np.zeros((steps, n_envs, A), np.float64)
    done = np.zeros((steps, n_envs), np.uint8)
    act = np.zeros((steps, n_envs, A), np.uint8)
    watch = np.zeros((steps, n_envs, A), np.uint8)
    misc = np.zeros((steps, n_envs, 16), np.int64)
    obs = [[None] * n_envs for _ in range(steps)]
    for t in range(steps):
        acts = synthetic_actions(seed, np.arange(n_envs), t, spec.n_actions)
        for i, e in enumerate(envs):
            r, d, ev = e.step(acts[i], with_obs=with_obs)
            rew[t, i], done[t, i] = r, d
            act[t, i], watch[t, i] = list(ev.act[:A]), list(ev.watch[:A])
            misc[t, i] = misc_row(ev) & 0xFFFFFFFF
            crashed = bool(ev.crashed)
            if d and (auto_reset or not crashed):  # without auto-reset the caller resets the envs that finished
                o = e.reset()                      # without a crash; a crashed env stays as it is
                crashed = bool(e.header()[2])  # the reset itself crashed: no obs
                obs[t][i] = o if with_obs and not crashed else None
            elif with_obs and not crashed:
                obs[t][i] = e.obs_list()
    return dict(first=first, reward=rew, done=done, act=act, watch=watch, misc=misc, obs=obs), envs
