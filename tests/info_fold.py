"""Helpers of the info-monitor tests (tests/test_info_monitor.py, tests/test_gpu_info_monitor.py): the event rows of
a decoded step (the inverse of mfg_decode_events), fixture replays through the C oracle, and the reference-side
episode fold of the fixtures' recorded info dicts. Not a test module."""
import functools

import numpy as np

import golden_compare as G

FIXTURES = ['large8', 'rooms4', 'alltest16', 'maint_rooms', 'eight_puzzle', 'puzzle_dest_crash', 'qquad_doors',
            'cap_dest81', 'pass2_mix', 'cap_maint64']
EV_FIELDS = ['door_coll', 'door_coll_hi', 'maint_coll', 'respawn_items_value', 'dirt_spawn_value', 'dirt_spawn_valid',
             'dest_reached', 'door_autoclose', 'done_mask', 'crashed', 'crash_reason', 'step', 'episode', 'maint_base']


def _i32(x):
    x = int(x) & 0xFFFFFFFF
    return x - (1 << 32) if x >= 1 << 31 else x


def ev_dict(ev, A):
    """A copy of an MfgEvents record as a dict (OracleEnv reuses its record)."""
    out = {k: int(getattr(ev, k)) for k in EV_FIELDS}
    out['act'] = [int(ev.act[a]) for a in range(A)]
    out['watch'] = [int(ev.watch[a]) for a in range(A)]
    return out


def pack_rows(ev, A):
    """Decoded events (dict) -> (ev_act u8 [A], ev_watch u8 [A], ev_misc i32 [16]): the inverse of mfg_decode_events."""
    from mfg_amd import abi
    m = np.zeros(abi.EV_MISC_N, np.int32)
    m[abi.EVM_DOOR_COLL_LO] = _i32(ev['door_coll'])
    m[abi.EVM_DOOR_COLL_HI] = _i32(ev['door_coll'] >> 32)
    m[abi.EVM_DOOR_COLL_2] = _i32(ev['door_coll_hi'])
    m[abi.EVM_DOOR_COLL_3] = _i32(ev['door_coll_hi'] >> 32)
    m[abi.EVM_MAINT_COLL] = _i32(ev['maint_coll'])
    m[abi.EVM_MAINT_COLL_HI] = _i32(ev['maint_coll'] >> 32)
    m[abi.EVM_RESPAWN_ITEMS] = ev['respawn_items_value']
    m[abi.EVM_DIRT_SPAWN] = ev['dirt_spawn_value']
    m[abi.EVM_DIRT_VALID] = ev['dirt_spawn_valid']
    m[abi.EVM_DEST_REACHED] = ev['dest_reached']
    m[abi.EVM_FLAGS] = (ev['door_autoclose'] & 1) | ((ev['crashed'] & 1) << 1) | ((ev['crash_reason'] & 0xFF) << 8)
    m[abi.EVM_DONE_MASK] = _i32(ev['done_mask'])
    m[abi.EVM_STEP] = ev['step']
    m[abi.EVM_EPISODE] = ev['episode']
    m[abi.EVM_MAINT_BASE] = ev['maint_base']
    return np.asarray(ev['act'][:A], np.uint8), np.asarray(ev['watch'][:A], np.uint8), m


@functools.lru_cache(maxsize=None)
def replay(tag, seed=0):
    """The fixture's recorded actions through the C oracle. Returns (spec, program, steps): one dict per step record
    (reset records are skipped) with actions, the packed rows, reward, done, crashed, the decoded events, the
    fixture's info dict, and the host evaluation's vals / pres (mfg_info_eval_host). Computed once per fixture."""
    import oracle as O
    from mfg_amd.spec import compile_spec
    from mfg_amd.info_program import compile_info_program, eval_host
    rec, _ = G.load(tag, seed)
    spec = compile_spec(f'{tag}.yaml')
    prog = compile_info_program(spec)
    env = O.OracleEnv(spec, rec['py_seed'])
    A = spec.n_agents
    steps = []
    for r in rec['steps']:
        if r['step'] == 0:
            env.reset()
            continue
        rew, done, ev = env.step(r['actions'], with_obs=False)
        e = ev_dict(ev, A)
        act, watch, misc = pack_rows(e, A)
        vals, pres = eval_host(prog, r['actions'], act, watch, misc, rew)
        steps.append(dict(t=r['t'], actions=list(r['actions']), act=act, watch=watch, misc=misc, reward=rew,
                          done=bool(done), crashed=bool(e['crashed']), fixture_crashed=bool(r.get('crashed')),
                          fixture_done=bool(r['done']), ev=e, info=r['info'], vals=vals, pres=pres))
    env.close()
    return spec, prog, steps


def fold_reference(steps):
    """The reference-side fold of the recorded info dicts: per episode, in step order, every key starts at 0.0 and
    adds each present step's value. -> list of dict(sum, count, length, crashed, infos). A crashed step (the
    reference raised there: no info) counts in the length and ends its episode."""
    eps, cur = [], dict(sum={}, count={}, length=0, crashed=0, infos=[])
    for s in steps:
        cur['length'] += 1
        if s['fixture_crashed']:
            cur['crashed'] = 1
        else:
            cur['infos'].append(s['info'])
            for k, v in s['info'].items():
                cur['sum'][k] = cur['sum'].get(k, 0.0) + v
                cur['count'][k] = cur['count'].get(k, 0) + 1
        if s['fixture_done'] or s['fixture_crashed']:
            eps.append(cur)
            cur = dict(sum={}, count={}, length=0, crashed=0, infos=[])
    return eps


def fold_host(prog, steps):
    """The monitor's accumulate rule (include/mfg_info.h) on the host evaluation's columns: acc += value and
    cnt += 1 where present, len += 1; a row per done or crashed step. -> (hdr i32 [n, 8], sum f64 [n, Kc], count
    u32 [n, Kc]) of env 0."""
    from mfg_amd import abi
    from mfg_amd.info_program import HDR_N, HDR_EP_INDEX, HDR_LENGTH, HDR_CRASHED, HDR_MAINT_BASE
    Kc = prog.n_keys + 2
    acc, cnt, length = np.zeros(Kc, np.float64), np.zeros(Kc, np.uint32), 0
    hdr, sums, counts = [], [], []
    for s in steps:
        p = s['pres'].astype(bool)
        acc[p] = acc[p] + s['vals'][p]
        cnt[p] += 1
        length += 1
        if s['done'] or s['crashed']:
            h = np.zeros(HDR_N, np.int32)
            h[HDR_EP_INDEX], h[HDR_LENGTH], h[HDR_CRASHED] = len(hdr), length, int(s['crashed'])
            h[HDR_MAINT_BASE] = s['misc'][abi.EVM_MAINT_BASE]
            hdr.append(h)
            sums.append(acc.copy())
            counts.append(cnt.copy())
            acc[:], cnt[:], length = 0.0, 0, 0
    return np.array(hdr, np.int32).reshape(-1, HDR_N), np.array(sums).reshape(-1, Kc), np.array(counts).reshape(-1, Kc)


def row_dicts(prog, hdr, sums, counts, i):
    """Row i as ({name: sum}, {name: count}) over the keys present at least once in the episode."""
    from mfg_amd.info_program import HDR_MAINT_BASE
    ks = np.nonzero(counts[i])[0]
    names = [prog.column_name(int(k), hdr[i][HDR_MAINT_BASE]) for k in ks]
    return ({n: float(sums[i][k]) for n, k in zip(names, ks)}, {n: int(counts[i][k]) for n, k in zip(names, ks)})
