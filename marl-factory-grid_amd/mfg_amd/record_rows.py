"""Host reference of the state recorder's rows (include/mfg_record.h, csrc/mfg_record.hip).

One row is the compaction of one env's record after a step that `views.summarize_state` needs: env id, episode
number, step, done / crashed flags, per agent the cell, the action index and the two event bytes, the battery levels
(f64 bit for bit), the door words and the item table. The word-by-word layout is documented in the C header; here

* `row_layout(spec, layout)` gives the word offsets from a compiled spec and the engine's layout dict,
* `pack_row(view, ...)` builds, in numpy, the row the kernel must write from an `engine.RecordView`,
* `row_snapshot(spec, layout, row)` turns a row back into a `views.Snapshot` (the only decoder: the batched
  recorder's step dicts are `views.summarize_state` of it).
"""
import numpy as np

from . import views as _views

FLAG_DONE, FLAG_CRASHED = 1, 2
EVM_FLAGS = 6  # MFG_EVM_FLAGS (include/mfg.h): bit1 crashed


def row_layout(spec, layout):
    """Word offsets of a row: {'A', 'nd', 'item_cap', 'has_bat', 'o_cell', 'o_act', 'o_bat' (-1 without batteries),
    'o_door', 'o_items', 'words'}. The item slots are those of the env record (o_pods - o_items)."""
    A, nd = int(spec.n_agents), int(spec.c.n_doors)
    has_bat = bool(spec.c.has_batteries)
    item_cap = (int(layout['o_pods']) - int(layout['o_items'])) // 4
    o_door = 4 + 2 * A + (2 * A if has_bat else 0)
    o_items = o_door + nd
    return dict(A=A, nd=nd, item_cap=item_cap, has_bat=has_bat, o_cell=4, o_act=4 + A,
                o_bat=4 + 2 * A if has_bat else -1, o_door=o_door, o_items=o_items, words=o_items + 2 + item_cap)


def pack_row(record_view, env, actions, ev_act, ev_watch, ev_misc, done):
    """The row (uint32 [words]) of env `env` after a step: `record_view` is the env's record as that step left it,
    actions / ev_act / ev_watch its [A] rows, ev_misc its [MFG_EV_MISC_N] row, done its flag."""
    v = record_view
    R = row_layout(v.spec, v.L)
    A, nd, cap = R['A'], R['nd'], R['item_cap']
    row = np.zeros(R['words'], np.uint32)
    crashed = (int(ev_misc[EVM_FLAGS]) >> 1) & 1
    row[0] = np.uint32(int(env) & 0xFFFFFFFF)
    row[1] = np.uint32((v.hdr('episode') + 1) & 0xFFFFFFFF)  # 1-based: the slot is 0 in the first episode
    row[2] = np.uint32(v.hdr('step') & 0xFFFFFFFF)
    row[3] = (FLAG_DONE if int(done) else 0) | (FLAG_CRASHED if crashed else 0)
    row[R['o_cell']:R['o_cell'] + A] = v.agent_pos().view(np.uint32)
    act = np.asarray(actions).astype(np.int64) & 0xFF
    row[R['o_act']:R['o_act'] + A] = (act | (np.asarray(ev_act).astype(np.int64) << 8)
                                      | (np.asarray(ev_watch).astype(np.int64) << 16)).astype(np.uint32)
    if R['has_bat']:
        row[R['o_bat']:R['o_bat'] + 2 * A] = np.frombuffer(v.b, np.uint32, 2 * A, v.L['o_battery'])
    row[R['o_door']:R['o_door'] + nd] = v.i32(v.L['o_door'], nd).view(np.uint32)
    row[R['o_items']] = np.uint32(v.hdr('n_items') & 0xFFFFFFFF)
    row[R['o_items'] + 1] = np.uint32(v.hdr('item_base') & 0xFFFFFFFF)
    row[R['o_items'] + 2:R['o_items'] + 2 + cap] = v.i32(v.L['o_items'], cap).view(np.uint32)
    return row


def row_fields(row):
    """(env, episode, step, done, crashed) of a row."""
    row = np.asarray(row, np.uint32)
    s = row[:3].view(np.int32)
    return int(s[0]), int(s[1]), int(s[2]), bool(int(row[3]) & FLAG_DONE), bool(int(row[3]) & FLAG_CRASHED)


def row_cells(spec, layout, row):
    """int32 [A] agent cells of a row."""
    R = row_layout(spec, layout)
    return np.asarray(row, np.uint32)[R['o_cell']:R['o_cell'] + R['A']].view(np.int32)


def row_snapshot(spec, layout, row):
    """`views.Snapshot` of a row; the agent states come through `views.agent_states` from the row's action indices
    and event bytes. Groups the summary drops (pods, drop-offs, destinations, dirt, machines, maintainers) stay
    empty."""
    R = row_layout(spec, layout)
    row = np.ascontiguousarray(row, np.uint32)
    A, nd, cap = R['A'], R['nd'], R['item_cap']
    cells = row[R['o_cell']:R['o_cell'] + A].view(np.int32)
    aw = row[R['o_act']:R['o_act'] + A]
    states = _views.agent_states(spec, aw & 0xFF, (aw >> 8) & 0xFF, (aw >> 16) & 0xFF)
    battery = []
    if R['has_bat']:
        battery = [float(x) for x in row[R['o_bat']:R['o_bat'] + 2 * A].view(np.float64)]
    dw = row[R['o_door']:R['o_door'] + nd]
    n_items = min(max(int(row[R['o_items']:R['o_items'] + 1].view(np.int32)[0]), 0), cap)
    base = int(row[R['o_items'] + 1:R['o_items'] + 2].view(np.int32)[0])
    items = []
    for k in range(n_items):
        w = int(row[R['o_items'] + 2 + k])
        if not w & _views.EW_ALIVE:
            continue
        items.append((base + k, -1 if (w & 0xFFFF) == _views.EW_NOPOS else w & 0xFFFF))
    return _views.Snapshot(step=int(row[2:3].view(np.int32)[0]),
                           agents=[(int(cells[a]), states[a][0], states[a][1]) for a in range(A)],
                           battery=battery, doors=[(int(w) & 1, (int(w) >> 8) & 0xFF) for w in dw], items=items)
