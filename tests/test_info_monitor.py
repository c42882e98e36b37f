"""CPU: the batched monitor's info program and its evaluation function, run on host memory (mfg_info_eval_host: the
kernel's own per-key function compiled for the host), against the three existing statements of the reference's info
dict (info.rebuild_info, InfoColumns on CPU tensors, the fixtures' recorded dicts), its episode fold against the
reference's recorded infos and against pandas, and the program validation of mfg_info_create."""
import ctypes as C

import numpy as np
import pytest

import info_fold as F


@pytest.mark.parametrize('tag', F.FIXTURES)
def test_host_evaluation_equals_rebuild_columns_and_fixture(tag):
    """Every non-crashed step of the fixture: the dict of the host evaluation == rebuild_info == the InfoColumns
    row == the reference's recorded info, keys and f64 values."""
    import torch
    from mfg_amd.engine import events_from_rows
    from mfg_amd.info import rebuild_info
    from mfg_amd.info_columns import InfoColumns
    from mfg_amd.info_program import to_dict
    spec, prog, steps = F.replay(tag)
    live = [s for s in steps if not s['crashed']]
    assert live and len(prog.columns) == prog.n_keys + 2
    # the packing helper is the inverse of the library's decoder
    for s in steps[:50]:
        back = events_from_rows(s['act'], s['watch'], s['misc'])
        assert {k: back[k] for k in s['ev']} == s['ev']
    # InfoColumns once, with the fixture's steps as the batch
    cols = InfoColumns(spec)
    cv, cp = cols(torch.tensor(np.array([s['actions'] for s in live])), torch.tensor(np.array([s['act'] for s in live])),
                  torch.tensor(np.array([s['watch'] for s in live])), torch.tensor(np.array([s['misc'] for s in live])),
                  torch.tensor(np.array([s['reward'] for s in live])))
    assert cols.columns == prog.columns
    hv = np.array([s['vals'] for s in live])
    hp = np.array([s['pres'] for s in live]).astype(bool)
    assert np.array_equal(cp.numpy(), hp)
    assert np.array_equal(cv.numpy(), hv)
    n_fixture = 0
    for s in live:
        got = to_dict(prog, s['vals'], s['pres'], s['ev']['maint_base'])
        want = rebuild_info(spec, s['actions'], s['ev'], [float(x) for x in s['reward']])
        assert got == want, (tag, s['t'], sorted(set(got.items()) ^ set(want.items()))[:6])
        if not s['fixture_crashed']:
            assert got == s['info'], (tag, s['t'], sorted(set(got.items()) ^ set(s['info'].items()))[:6])
            n_fixture += 1
    assert n_fixture > 0
    for s in steps:
        if s['crashed']:
            assert not s['pres'].any() and not s['vals'].any()


@pytest.mark.parametrize('tag', F.FIXTURES)
def test_episode_fold_equals_reference_fold(tag):
    """The accumulate rule over the host evaluation == the Python fold of the fixture's recorded infos: one row per
    fixture done, identical sums and counts, the right lengths."""
    _, prog, steps = F.replay(tag)
    ref = F.fold_reference(steps)
    hdr, sums, counts = F.fold_host(prog, steps)
    n_done = sum(1 for s in steps if s['fixture_done'] or s['fixture_crashed'])
    assert len(ref) == len(hdr) == n_done >= 1
    from mfg_amd.info_program import HDR_LENGTH, HDR_CRASHED
    for i, ep in enumerate(ref):
        s, c = F.row_dicts(prog, hdr, sums, counts, i)
        assert s == ep['sum'] and c == ep['count'], (tag, i)
        assert hdr[i][HDR_LENGTH] == ep['length'] and hdr[i][HDR_CRASHED] == ep['crashed']


@pytest.mark.parametrize('tag', F.FIXTURES)
def test_frame_equals_pandas_aggregate(tag):
    """episode_frame (what BatchedEnvMonitor.frame() builds from the drained rows) against the reference's
    aggregate, built with pandas exactly as EnvMonitor._read_done does. Same column set per episode (absent: NaN);
    values within 1e-12 * sum|x|: pandas sums pairwise, the monitor sequentially, and for n <= 1001 f64 terms the
    two differ by at most 2 n 2^-53 sum|x| ~ 2.3e-13 sum|x|."""
    import pandas as pd
    from mfg_amd.monitor import IGNORED_DF_COLUMNS, episode_frame
    _, prog, steps = F.replay(tag)
    ref = F.fold_reference(steps)
    df = episode_frame(prog, *F.fold_host(prog, steps))
    assert len(df) == len(ref) and list(df['episode']) == list(range(len(ref)))
    assert list(df['length']) == [ep['length'] for ep in ref] and not df['env'].any()
    extra = {'env', 'episode', 'length'}
    for i, ep in enumerate(ref):
        mon = {}  # an episode of one crashed step has no info rows
        if ep['infos']:
            d = pd.DataFrame.from_dict({j: {k: v for k, v in info.items()
                                            if k not in ['terminal_observation', 'episode']}
                                        for j, info in enumerate(ep['infos'])}, orient='index')
            columns = [c for c in d.columns if c not in IGNORED_DF_COLUMNS]
            agg = d.aggregate({c: 'mean' if c.endswith('ount') else 'sum' for c in columns})
            mon = dict(agg)
        row = df.iloc[i]
        have = {c for c in df.columns if c not in extra and not pd.isna(row[c])}
        assert have == set(mon), (tag, i, sorted(have ^ set(mon))[:6])
        for k, want in mon.items():
            bound = 1e-12 * sum(abs(info[k]) for info in ep['infos'] if k in info)
            assert abs(row[k] - want) <= bound, (tag, i, k, row[k], want, bound)


def test_frame_mean_rule_on_a_count_key():
    """No fixture key ends in 'ount': a synthetic three-step episode with a key 'x_count' present in two steps is
    averaged over those two; the other keys are summed; 'step' is dropped; a key never present is NaN."""
    import pandas as pd
    from mfg_amd.info_program import InfoProgram, OP_DTYPE, HDR_N, HDR_LENGTH, HDR_ENV, HDR_EP_INDEX
    from mfg_amd.monitor import episode_frame
    prog = InfoProgram(['x_count', 'y', 'never', 'step_reward', 'step'], np.zeros(0, OP_DTYPE), np.zeros(4, np.int32),
                       np.zeros((1, 32, 5)), [1], 0.0, 0)
    infos = [{'x_count': 3.0, 'y': 1.5, 'step_reward': 0.25, 'step': 1}, {'y': 2.0, 'step_reward': 0.5, 'step': 2},
             {'x_count': 4.0, 'y': 0.25, 'step_reward': 1.0, 'step': 3}]
    sums, counts = np.zeros((2, 5)), np.zeros((2, 5), np.uint32)
    for info in infos:
        for k, v in info.items():
            sums[0, prog.columns.index(k)] += v
            counts[0, prog.columns.index(k)] += 1
    sums[1, 1], counts[1, 1] = 7.0, 1  # a second episode without x_count
    hdr = np.zeros((2, HDR_N), np.int32)
    hdr[0, HDR_ENV], hdr[0, HDR_EP_INDEX], hdr[0, HDR_LENGTH] = 5, 2, 3
    hdr[1, HDR_LENGTH] = 1
    df = episode_frame(prog, hdr, sums, counts)
    ref = pd.DataFrame.from_dict(dict(enumerate(infos)), orient='index')
    ref = ref.aggregate({c: 'mean' if c.endswith('ount') else 'sum' for c in ref.columns if c != 'step'})
    assert set(df.columns) == {'env', 'episode', 'length', 'x_count', 'y', 'step_reward'}
    assert df.loc[0, 'x_count'] == 3.5 == ref['x_count'] and df.loc[0, 'y'] == 3.75 == ref['y']
    assert df.loc[0, 'step_reward'] == 1.75 and (df.loc[0, 'env'], df.loc[0, 'episode'], df.loc[0, 'length']) == (5, 2, 3)
    assert pd.isna(df.loc[1, 'x_count']) and df.loc[1, 'y'] == 7.0 and pd.isna(df.loc[1, 'step_reward'])


def _create(prog, n_envs=4, cap=4, **over):
    """mfg_info_create on a (possibly broken) program: -> (rc, message). A valid program would go on to the GPU:
    only broken ones are passed here."""
    from mfg_amd.engine import load_lib
    L = load_lib()
    args = list(prog.c_args())
    names = ['ops', 'n_ops', 'key_off', 'n_keys', 'action_table', 'n_agents', 'n_actions', 'noop_cost', 'dest_max']
    for k, v in over.items():
        args[names.index(k)] = v
    h = C.c_void_p()
    rc = L.mfg_info_create(*args, 0, n_envs, cap, C.byref(h))
    assert not h.value
    return rc, L.mfg_last_error(None).decode()


def test_create_rejects_broken_programs_without_touching_the_gpu():
    import copy
    _, prog, _ = F.replay('rooms4')

    def broken(mutate):
        p = copy.deepcopy(prog)
        mutate(p)
        return p

    rc, msg = _create(broken(lambda p: p.ops['key'].__setitem__(3, p.n_keys)))
    assert rc < 0 and 'op key out of range' in msg, msg
    rc, msg = _create(broken(lambda p: p.ops['key'].__setitem__(3, -1)))
    assert rc < 0 and 'op key out of range' in msg, msg
    agent_op = int(np.nonzero(prog.ops['kind'] == 1)[0][0])  # an act_coll op reads its agent's row byte
    rc, msg = _create(broken(lambda p: p.ops['agent'].__setitem__(agent_op, p.n_agents)))
    assert rc < 0 and 'op agent index out of range' in msg, msg
    rc, msg = _create(broken(lambda p: p.key_off.__setitem__(2, int(p.key_off[3]) + 1)))
    assert rc < 0 and 'key_off is not monotone' in msg, msg
    rc, msg = _create(broken(lambda p: p.key_off.__setitem__(p.n_keys, p.n_ops + 5)))
    assert rc < 0 and 'key_off' in msg, msg
    rc, msg = _create(prog, n_keys=4097)
    assert rc < 0 and 'n_keys out of range' in msg and '4096' in msg, msg
    rc, msg = _create(prog, n_agents=129)
    assert rc < 0 and 'n_agents out of range' in msg, msg
    rc, msg = _create(broken(lambda p: p.ops['kind'].__setitem__(0, 12)))
    assert rc < 0 and 'op kind out of range' in msg, msg
    rc, msg = _create(broken(lambda p: p.n_actions.__setitem__(0, 33)))
    assert rc < 0 and 'n_actions out of range' in msg, msg
    rc, msg = _create(prog, n_envs=0)
    assert rc < 0 and 'n_envs' in msg, msg
    rc, msg = _create(prog, cap=0)
    assert rc < 0 and 'ep_capacity' in msg, msg


def test_program_layout_and_order():
    """The op record is the header's 28-byte struct; ops are sorted by key and, within a key, keep InfoColumns' order;
    the action bitmask and the per-action battery cost lower as the header says."""
    from mfg_amd.info_columns import InfoColumns
    from mfg_amd.info_program import MfgInfoOp, OP_DTYPE, KIND, compile_info_program
    from mfg_amd.spec import compile_spec
    assert C.sizeof(MfgInfoOp) == OP_DTYPE.itemsize == 28
    spec = compile_spec('alltest16.yaml')
    cols = InfoColumns(spec)
    prog = compile_info_program(spec, cols)
    assert prog.n_keys == cols.n_keys > 128 and prog.columns == cols.columns
    assert list(prog.ops['key']) == sorted(prog.ops['key']) and prog.key_off[-1] == prog.n_ops == len(cols._ops)
    for k in range(prog.n_keys):
        mine = [KIND[kind] for key, kind, _ in cols._ops if key == k]
        assert list(prog.ops['kind'][prog.key_off[k]:prog.key_off[k + 1]]) == mine
    a_ops = prog.ops[prog.ops['kind'] == KIND['action']]
    for a in range(spec.n_agents):  # every slot of an agent belongs to exactly one of its action ops
        masks = [int(m) & 0xFFFFFFFF for m in a_ops['i0'][a_ops['agent'] == a]]
        assert sum(masks) == (1 << len(spec.agent_actions[a])) - 1
    assert prog.action_table.shape == (spec.n_agents, 32, 5)


def test_host_rules_are_refused(monkeypatch):
    import sys
    from pathlib import Path
    # the custom rule module imports the reference's package names: the compat shadow, as tests/test_host_rules.py
    monkeypatch.syspath_prepend(str(Path(__file__).resolve().parent.parent / 'marl-factory-grid_amd' / 'compat'))
    for m in [m for m in sys.modules if m.startswith('marl_factory_grid') or m.startswith('mfg_custom_')]:
        monkeypatch.delitem(sys.modules, m)
    from mfg_amd.info_program import compile_info_program
    from mfg_amd.spec import compile_spec, UnsupportedSpec
    spec = compile_spec('custom_rules4.yaml', custom_modules_path=str(Path(__file__).parent / 'custom_rules'))
    assert spec.host_rules
    with pytest.raises(UnsupportedSpec, match='custom rules'):
        compile_info_program(spec)
