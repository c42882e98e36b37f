"""The action mask by replay on the C oracle (test helper; CPU).

The oracle has no clone, so a probe is a replay: a fresh OracleEnv(spec, seed), reset, the recorded action prefix, then
one step in which agent a plays slot s and every other agent plays its Noop slot; bit s of the agent's word is
`ev.act[a] == 0x80 | 1 | ...` (acted and valid). Every agent of the config needs a Noop slot.
"""
from pathlib import Path

import numpy as np

import oracle as O
from mfg_amd import abi
from mfg_amd.spec import compile_spec

DENSE = Path(__file__).resolve().parent / 'action_mask_dense.yaml'
OP_NAMES = {abi.ACT_NOOP: 'Noop', abi.ACT_MOVE: 'Move', abi.ACT_CHARGE: 'Charge', abi.ACT_CLEAN: 'Clean',
            abi.ACT_DEST: 'DestAction', abi.ACT_DOORUSE: 'DoorUse', abi.ACT_ITEM: 'ItemAction',
            abi.ACT_MACHINE: 'MachineAction'}

_specs = {}


def spec_of(cfg):
    if cfg not in _specs:
        _specs[cfg] = compile_spec(str(DENSE) if cfg == 'dense' else cfg)
    return _specs[cfg]


def slot_ops(spec):
    """Per agent the opcode of every action slot."""
    return [[int(spec.c.actions[a][s].op) for s in range(spec.n_actions[a])] for a in range(spec.n_agents)]


def noop_slots(spec):
    ops = slot_ops(spec)
    assert all(abi.ACT_NOOP in o for o in ops), 'the checker needs a Noop slot for every agent'
    return [o.index(abi.ACT_NOOP) for o in ops]


def replay(spec, seed, prefix):
    """A fresh env at the state after reset + prefix, with what the last prefix step reported: (env, done, crashed)."""
    env = O.OracleEnv(spec, seed)
    env.reset()
    done = crashed = False
    for acts in prefix:
        _, done, ev = env.step(acts, with_obs=False)
        crashed = bool(ev.crashed)
    return env, done, crashed


def probe(spec, seed, prefix, a, s, others=None):
    """ev.act[a] & 0x81 of the step (agent a: slot s, the others: `others` or their Noop slots) after the prefix."""
    acts = list(noop_slots(spec) if others is None else others)
    acts[a] = s
    env, _, _ = replay(spec, seed, prefix)
    _, _, ev = env.step(acts, with_obs=False)
    out = int(ev.act[a]) & 0x81
    env.close()
    return out


def mask_of_state(spec, seed, prefix):
    """The words [A] (uint32) of the state after reset + prefix."""
    words = np.zeros(spec.n_agents, np.uint32)
    for a in range(spec.n_agents):
        for s in range(spec.n_actions[a]):
            if probe(spec, seed, prefix, a, s) == 0x81:
                words[a] |= np.uint32(1 << s)
    return words


def random_prefix(spec, rng, n):
    return [[int(rng.integers(0, k)) for k in spec.n_actions] for _ in range(n)]
