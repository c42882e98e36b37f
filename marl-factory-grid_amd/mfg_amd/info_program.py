"""The info program: `InfoColumns`' ordered op list lowered to the flat tables the device runs (include/mfg_info.h).

`InfoColumns.__init__` derives a config's key set and its accumulation ops in the reference's order
(environment/factory.py:222-259). `compile_info_program(spec)` turns that list into

* `ops`     one `MfgInfoOp` record {key, kind, agent, i0, i1, r} per op, stably sorted by key (the ops of one
            key keep their order, so every key's f64 sum is accumulated as the reference does),
* `key_off` the CSR offsets [n_keys + 1] of each key's op list,
* `action_table` f64 [A][32][5]: valid, fail, aux0, aux1 reward and the battery cost of every action slot
            (NaN: the per-action cost dict has no entry for the slot's class, as `InfoColumns` has it),
* the scalars `noop_cost` (the 'Noop' battery cost) and `dest_max`.

The same tables feed `mfg_info_create` (the device monitor, `engine.InfoMonitor`) and `mfg_info_eval_host` (the
same evaluation function on host memory, `eval_host`). A spec with host-side custom rules is refused: their
results are merged into the Result list on the host (mfg_amd/host_rules.py) and never reach the event rows.
"""
import ctypes as C

import numpy as np

from . import abi
from .info_columns import InfoColumns
from .spec import UnsupportedSpec

KINDS = ['action', 'act_coll', 'door_autoclose', 'battery_cost', 'dirt_spawn', 'dest_reach', 'respawn_items',
         'watch_bit', 'door_coll', 'maint_coll', 'done_bit', 'maint_done']  # MFG_INFO_* (include/mfg_info.h)
KIND = {k: i for i, k in enumerate(KINDS)}
MAX_KEYS = 4096  # MFG_INFO_MAX_KEYS
ATAB_N = 5       # MFG_INFO_ATAB_N
HDR_N = 8        # MFG_INFO_HDR_N
HDR_ENV, HDR_EP_INDEX, HDR_LENGTH, HDR_CRASHED, HDR_MAINT_BASE = range(5)


class MfgInfoOp(C.Structure):
    """include/mfg_info.h mfg_info_op (28 bytes, 4-byte aligned)."""
    _pack_ = 4
    _fields_ = [('key', C.c_int32), ('kind', C.c_int32), ('agent', C.c_int32), ('i0', C.c_int32), ('i1', C.c_int32),
                ('r', C.c_double)]


OP_DTYPE = np.dtype({'names': ['key', 'kind', 'agent', 'i0', 'i1', 'r'],
                     'formats': ['<i4', '<i4', '<i4', '<i4', '<i4', '<f8'],
                     'offsets': [0, 4, 8, 12, 16, 20], 'itemsize': 28})


class InfoProgram:
    """The compiled tables of one spec (numpy, host memory) and the column names."""

    def __init__(self, columns, ops, key_off, action_table, n_actions, noop_cost, dest_max):
        self.columns = list(columns)  # the keys, then 'step_reward' and 'step'
        self.n_keys = len(self.columns) - 2
        self.ops = np.ascontiguousarray(ops, OP_DTYPE)
        self.key_off = np.ascontiguousarray(key_off, np.int32)
        self.action_table = np.ascontiguousarray(action_table, np.float64)
        self.n_actions = np.ascontiguousarray(n_actions, np.int32)
        self.n_agents = int(self.n_actions.size)
        self.noop_cost = float(noop_cost)
        self.dest_max = int(dest_max)

    @property
    def n_ops(self):
        return int(self.ops.size)

    def c_args(self):
        """The leading arguments shared by mfg_info_create and mfg_info_eval_host."""
        return (self.ops.ctypes.data_as(C.c_void_p), self.n_ops, self.key_off.ctypes.data_as(C.c_void_p), self.n_keys,
                self.action_table.ctypes.data_as(C.c_void_p), self.n_agents,
                self.n_actions.ctypes.data_as(C.c_void_p), C.c_double(self.noop_cost), self.dest_max)

    def column_name(self, k, maint_base):
        """Column k's info key; a maintainer slot column is named from the episode's first maintainer u_int."""
        name = self.columns[k]
        if name.startswith('Maintainer[slot '):
            slot = int(name[len('Maintainer[slot '):name.index(']')])
            return f'Maintainer[{int(maint_base) + slot}]_Collisions'
        return name


def compile_info_program(spec, cols=None):
    """EnvSpec -> InfoProgram. cols: an `InfoColumns` of the spec to lower (else one is built)."""
    if getattr(spec, 'host_rules', None):
        raise UnsupportedSpec('the batched monitor cannot see host-side custom rules '
                              f'({[r[1] for r in spec.host_rules]}): their results never reach the event rows')
    cols = cols if cols is not None else InfoColumns(spec)
    A = spec.n_agents
    if cols.n_keys > MAX_KEYS:
        raise UnsupportedSpec(f'{cols.n_keys} info keys > {MAX_KEYS}')
    recs = []
    for key, kind, p in cols._ops:
        agent, i0, r = 0, 0, 0.0
        if kind == 'action':
            agent = p[0]
            for s in p[1]:
                i0 |= 1 << s
            if i0 >= 1 << 31:
                i0 -= 1 << 32  # the u32 bitmask in the record's int32 field
        elif kind == 'act_coll':
            agent = p[0]
        elif kind == 'battery_cost':
            agent, ri = p
            _, ri_, rf = spec.rules[ri]
            if ri_[2]:
                i0 = 1  # the cost comes from the action table (Noop: the scalar)
            else:
                r = rf[0]
        elif kind == 'dest_reach':
            agent, r = p
        elif kind == 'watch_bit':
            agent, i0, r = p
        elif kind in ('door_coll', 'maint_coll', 'done_bit'):
            i0, r = p
        elif kind == 'maint_done':
            agent, i0, r = p
        recs.append((int(key), KIND[kind], int(agent), int(i0), 0, float(r)))
    order = sorted(range(len(recs)), key=lambda i: recs[i][0])  # stable: ops of one key keep their order
    ops = np.zeros(len(recs), OP_DTYPE)
    for j, i in enumerate(order):
        ops[j] = recs[i]
    key_off = np.zeros(cols.n_keys + 1, np.int32)
    for rec in recs:
        key_off[rec[0] + 1] += 1
    key_off = np.cumsum(key_off, dtype=np.int64).astype(np.int32)
    table = np.zeros((A, abi.MAX_ACTIONS, ATAB_N), np.float64)
    cost = spec.battery_cost_dict or {}
    nan = float('nan')
    for a in range(A):
        for s, ac in enumerate(spec.agent_actions[a]):
            table[a, s] = (ac['valid'], ac['fail'], ac['aux0'], ac['aux1'], cost.get(ac['cls'], nan))
    n_actions = [len(spec.agent_actions[a]) for a in range(A)]
    return InfoProgram(cols.columns, ops, key_off, table, n_actions, cost.get('Noop', nan), cols._dest_max)


def eval_host(prog, actions, ev_act, ev_watch, ev_misc, reward):
    """One env-step on host memory through mfg_info_eval_host (the kernel's evaluation function compiled for the
    host; no GPU): -> (values f64 [Kc], present u8 [Kc])."""
    from .engine import load_lib, _check
    L = load_lib()
    A = prog.n_agents
    act = np.ascontiguousarray(actions, np.int32)
    ea = np.ascontiguousarray(ev_act, np.uint8)
    ew = np.ascontiguousarray(ev_watch, np.uint8)
    em = np.ascontiguousarray(ev_misc, np.int32)
    rw = np.ascontiguousarray(reward, np.float64)
    if not (act.size == ea.size == ew.size == rw.size == A) or em.size != abi.EV_MISC_N:
        raise ValueError('row sizes do not match the program')
    vals = np.zeros(prog.n_keys + 2, np.float64)
    pres = np.zeros(prog.n_keys + 2, np.uint8)
    _check(L.mfg_info_eval_host(*prog.c_args(), act.ctypes.data, ea.ctypes.data, ew.ctypes.data, em.ctypes.data,
                                rw.ctypes.data, vals.ctypes.data, pres.ctypes.data), 'mfg_info_eval_host')
    return vals, pres


def to_dict(prog, vals, pres, maint_base=0):
    """The info dict (the reference's key names) of one row of columns."""
    out = {}
    for k in np.nonzero(np.asarray(pres))[0]:
        name = prog.column_name(int(k), maint_base)
        out[name] = int(vals[k]) if name == 'step' else float(vals[k])
    return out
