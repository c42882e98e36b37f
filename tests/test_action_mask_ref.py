"""The replay checker of the action mask (tests/action_mask_ref.py) on the C oracle: CPU only.

Three conditions on the checker and on its inputs, fixed by the definition of the mask (include/mfg.h mfg_action_mask),
not measured from the engine:
  * the answer for agent 0 does not depend on what the other agents play (it acts first);
  * Noop is always valid;
  * coverage: over the probed states of the dense config Move, DoorUse, Clean and ItemAction each show a valid and an
    invalid probe; Charge, MachineAction and DestAction show none valid (Q18, Q17, and the battery that starts at 1.0
    and only rises on a fresh episode). If one of these ever is valid, the definition has to be revisited.
"""
import numpy as np
import pytest

import action_mask_ref as M
from mfg_amd import abi

SEEDS = (0, 1)
PREFIX_LENGTHS = (0, 1, 2, 3, 5, 8, 12, 16, 20)


def _states(cfg):
    """(seed, prefix) of the probed states: per seed one random action sequence cut at PREFIX_LENGTHS; states whose
    prefix ended the episode or crashed are left out (the step after them is not a step of that episode)."""
    spec = M.spec_of(cfg)
    out = []
    for seed in SEEDS:
        rng = np.random.default_rng(1000 + seed)
        full = M.random_prefix(spec, rng, max(PREFIX_LENGTHS))
        for n in PREFIX_LENGTHS:
            env, done, crashed = M.replay(spec, seed, full[:n])
            env.close()
            if not done and not crashed:
                out.append((seed, full[:n]))
    return spec, out


@pytest.fixture(scope='module')
def dense_probes():
    """Every (state, agent, slot) probe of the dense config: (op, valid) pairs."""
    spec, states = _states('dense')
    ops = M.slot_ops(spec)
    res = []
    for seed, prefix in states:
        for a in range(spec.n_agents):
            for s in range(spec.n_actions[a]):
                res.append((ops[a][s], M.probe(spec, seed, prefix, a, s) == 0x81))
    assert len(states) >= 12
    return res


def test_noop_is_always_valid(dense_probes):
    noop = [v for op, v in dense_probes if op == abi.ACT_NOOP]
    assert noop and all(noop)


def test_coverage_of_the_dense_config(dense_probes):
    seen = {}
    for op, v in dense_probes:
        seen.setdefault(op, set()).add(v)
    print({M.OP_NAMES[op]: sorted(v) for op, v in seen.items()})
    for op in (abi.ACT_MOVE, abi.ACT_DOORUSE, abi.ACT_CLEAN, abi.ACT_ITEM):
        assert seen[op] == {False, True}, f'{M.OP_NAMES[op]}: outcomes {seen[op]}'
    for op in (abi.ACT_CHARGE, abi.ACT_MACHINE, abi.ACT_DEST):
        assert seen[op] == {False}, f'{M.OP_NAMES[op]} was valid in a probe: revisit the mask\'s definition'


@pytest.mark.parametrize('cfg', ['dense', 'rooms4.yaml', 'logic_stress.yaml'])
def test_agent0_does_not_depend_on_the_others(cfg):
    spec, states = _states(cfg)
    rng = np.random.default_rng(7)
    for seed, prefix in states[::3]:
        for s in range(spec.n_actions[0]):
            want = M.probe(spec, seed, prefix, 0, s)
            for _ in range(3):
                others = [int(rng.integers(0, k)) for k in spec.n_actions]
                assert M.probe(spec, seed, prefix, 0, s, others) == want, (cfg, seed, len(prefix), s, others)
