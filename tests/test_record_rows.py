"""CPU: the state recorder's host row reference (mfg_amd/record_rows.py) on hand-built env records with a hand-chosen
layout: a packed row decodes to the same `summarize_state` as the record itself, at 3 and 70 agents, 0 / 2 / 65
doors, with and without batteries, with carried (no position) items and dead item slots; the row words sit where
include/mfg_record.h documents them; and the argument errors of `BatchedEnvRecorder`, raised before any device work."""
from types import SimpleNamespace

import numpy as np
import pytest

from mfg_amd import views
from mfg_amd.engine import HDR, HDR_N, RecordView
from mfg_amd.record_rows import pack_row, row_cells, row_fields, row_layout, row_snapshot

EW_ALIVE, EW_NOPOS = 0x10000, 0xFFFF
H, W = 9, 11


def _spec(A, nd, has_bat, groups):
    rng = np.random.default_rng(A * 1000 + nd)
    cells = rng.permutation(H * W)
    return SimpleNamespace(
        n_agents=A, H=H, W=W, agent_names=[f'a{i}' for i in range(A)],
        action_classes=[['Noop', 'Move', 'ItemAction', 'DoorUse'] for _ in range(A)],
        wall_cells=[int(c) for c in cells[:7]], door_cells=[int(c) for c in cells[7:7 + nd]],
        group_names=groups, c=SimpleNamespace(n_doors=nd, has_batteries=int(has_bat), pod_charge_rate=0.4))


def _layout(A, nd, item_cap):
    L, o = {}, 0
    L['o_hdr'] = o; o += 4 * HDR_N
    o += 16  # rule counters
    for k in ('o_agent_pos', 'o_agent_arr', 'o_agent_par'):
        L[k] = o; o += 4 * A
    L['o_door'] = o; o += 4 * nd
    L['o_items'] = o; o += 4 * item_cap
    for k in ('o_pods', 'o_drops', 'o_dests', 'o_machines', 'o_maints', 'o_dirt_pos', 'o_dirt_id'):
        L[k] = o
    o = (o + 7) & ~7
    L['o_battery'] = o; o += 8 * A
    L['o_dirt_amt'] = o
    L['size'] = (o + 15) & ~15
    return L


def _record(spec, L, seed, items):
    """A record with random agent cells, batteries and door words, and the given item words."""
    rng = np.random.default_rng(seed)
    A, nd = spec.n_agents, spec.c.n_doors
    rec = np.zeros(L['size'], np.uint8)
    hdr = rec[L['o_hdr']:L['o_hdr'] + 4 * HDR_N].view(np.int32)
    hdr[HDR['step']], hdr[HDR['episode']] = 17, 4
    hdr[HDR['n_items']], hdr[HDR['item_base']] = len(items), 23
    rec[L['o_agent_pos']:L['o_agent_pos'] + 4 * A].view(np.int32)[:] = rng.integers(0, H * W, A)
    rec[L['o_battery']:L['o_battery'] + 8 * A].view(np.float64)[:] = rng.random(A)
    rec[L['o_door']:L['o_door'] + 4 * nd].view(np.int32)[:] = (rng.integers(0, 2, nd) | (rng.integers(0, 11, nd) << 8)
                                                             | 0x10000)
    rec[L['o_items']:L['o_items'] + 4 * len(items)].view(np.int32)[:] = items
    return rec


def _events(spec, seed):
    rng = np.random.default_rng(seed + 99)
    A = spec.n_agents
    actions = rng.integers(0, 4, A).astype(np.int32)
    ev_act = rng.choice(np.array([0, 0x80, 0x81, 0x83, 0x85], np.uint8), A)
    ev_watch = rng.choice(np.array([0, 0, 1, 2, 8], np.uint8), A)
    ev_act[0], ev_watch[0] = 0x81, 0   # acted, valid
    ev_act[1], ev_watch[1] = 0x80, 1   # WatchCollisions overrides the action
    ev_act[2], ev_watch[2] = 0, 0      # did not act: Noop / valid
    return actions, ev_act, ev_watch


CASES = {
    # A, doors, batteries, item words (slot 1 carried: no position; slot 2 dead), item capacity, groups
    'a3_bat_items': (3, 0, True, [EW_ALIVE | 40, EW_ALIVE | EW_NOPOS, 12, EW_ALIVE | 98], 5, ['Items', 'Batteries']),
    'a3_doors2': (3, 2, False, [], 0, ['Doors']),
    'a70_doors65': (70, 65, False, [EW_ALIVE | 3], 2, ['Doors', 'Items']),
    'a70_bat': (70, 0, True, [], 0, ['Batteries', 'Doors']),
}


@pytest.mark.parametrize('case', list(CASES))
def test_row_round_trip_equals_record_summary(case):
    A, nd, has_bat, items, cap, groups = CASES[case]
    spec, L = _spec(A, nd, has_bat, groups), _layout(A, nd, cap)
    rec = _record(spec, L, 5, items)
    view = RecordView(rec, L, spec)
    actions, ev_act, ev_watch = _events(spec, 5)
    misc = np.zeros(16, np.int32)
    row = pack_row(view, 4711, actions, ev_act, ev_watch, misc, 1)
    R = row_layout(spec, L)
    assert row.dtype == np.uint32 and row.shape == (R['words'],)
    assert R['words'] == 4 + 2 * A + (2 * A if has_bat else 0) + nd + 2 + cap
    want = views.summarize_state(spec, views.snapshot_from_record(view, views.agent_states(spec, actions, ev_act,
                                                                                          ev_watch)))
    got = views.summarize_state(spec, row_snapshot(spec, L, row))
    assert list(got) == list(want)
    for k in want:
        assert got[k] == want[k], (case, k)
    # the content is not trivially empty: what each case is about is there
    assert len(got['agents']) == A and got['agents'][1]['action'] == 'Collisions' and got['agents'][2]['action'] == 'Noop'
    assert got['agents'][0]['valid'] is True and got['step'] == 17
    assert len(got.get('doors', [])) == (nd if 'Doors' in groups else 0)
    if has_bat:
        assert [b['chargeLevel'] for b in got['batteries']] == [float(x) for x in view.battery()]
    if case == 'a3_bat_items':
        assert [(i['name'], i['x'], i['y']) for i in got['items']] == [
            ('Item[23]', 40 // W, 40 % W), ('Item[24]', -9999, -9999), ('Item[26]', 98 // W, 98 % W)]


def test_row_words_are_where_the_header_documents_them():
    A, nd, has_bat, items, cap, groups = CASES['a3_bat_items']
    spec, L = _spec(A, 2, has_bat, groups + ['Doors']), _layout(A, 2, cap)
    view = RecordView(_record(spec, L, 9, items), L, spec)
    actions, ev_act, ev_watch = _events(spec, 9)
    misc = np.zeros(16, np.int32)
    misc[6] = 2 | (8 << 8)  # MFG_EVM_FLAGS: crashed, reason 8
    row = pack_row(view, 2, actions, ev_act, ev_watch, misc, 0)
    assert row_fields(row) == (2, 5, 17, False, True)  # episode: the header slot (4) + 1
    assert list(row[:4]) == [2, 5, 17, 2]
    assert list(row[4:4 + A].view(np.int32)) == list(view.agent_pos()) == list(row_cells(spec, L, row))
    for a in range(A):
        assert int(row[4 + A + a]) == int(actions[a]) | int(ev_act[a]) << 8 | int(ev_watch[a]) << 16
    assert row[4 + 2 * A:4 + 4 * A].tobytes() == view.battery().tobytes()
    assert list(row[4 + 4 * A:4 + 4 * A + 2].view(np.int32)) == list(view.i32(L['o_door'], 2))
    o = 4 + 4 * A + 2
    assert list(row[o:o + 2]) == [len(items), 23] and list(row[o + 2:o + 2 + cap]) == items + [0]
    assert row_fields(pack_row(view, 2, actions, ev_act, ev_watch, np.zeros(16, np.int32), 1))[3:] == (True, False)


def test_row_round_trip_negative_control():
    """A changed row word changes the decoded summary (the comparison above can fail)."""
    A, nd, has_bat, items, cap, groups = CASES['a3_bat_items']
    spec, L = _spec(A, nd, has_bat, groups), _layout(A, nd, cap)
    view = RecordView(_record(spec, L, 5, items), L, spec)
    actions, ev_act, ev_watch = _events(spec, 5)
    row = pack_row(view, 0, actions, ev_act, ev_watch, np.zeros(16, np.int32), 0)
    base = views.summarize_state(spec, row_snapshot(spec, L, row))
    for w in (2, 4, 4 + A, 4 + 2 * A + 1, 4 + 4 * A + 2):
        bad = row.copy()
        bad[w] ^= 1
        assert views.summarize_state(spec, row_snapshot(spec, L, bad)) != base, w


@pytest.mark.parametrize('kw,msg', [(dict(envs=[1, 2, 1]), 'twice'), (dict(envs=[0, 4]), 'out of range'),
                                    (dict(envs=[-1]), 'out of range'), (dict(envs=[0], capacity=0), 'capacity'),
                                    (dict(envs=[0], episodes=[0, 2]), '1-based')])
def test_batched_env_recorder_argument_errors(kw, msg):
    """Checked before the engine or the GPU is touched: a stand-in env with only its batch size is enough."""
    from mfg_amd.monitor import BatchedEnvRecorder
    with pytest.raises(ValueError, match=msg):
        BatchedEnvRecorder(SimpleNamespace(B=4), **kw)
