"""GPU: the second 64-lane pass of the agent-parallel kernels (the NW = 2 instantiation of k_logic, k_reset, k_resetdone
and k_action_mask, and the long-ray render) on full-module specs, and the maintainer / machine caps, against the
reference fixtures and the C oracle (bit-exact, through the checkers of the existing GPU test modules).
  pass2_mix:   70 agents, agents 64..69 are Carriers (ItemAction, Charge, MachineAction, Clean; Batteries that drain and
               end episodes through DoneAtBatteryDischarge; 40 maintainers: slots 32..39 set the high maintainer word).
  pass2_bound: 69 agents; Karl (64) with configured Positions and a bound destination, Heinz_the_2nd (68) with a bound
               destination, ordered Combined layers with agent members >= 64, 7-point rays in the long-ray render.
  cap_maint64: 64 maintainers and 30 machines, the engine's caps.
What the runs of these configs reach is counted on the CPU in test_second_pass.py."""
import re
from pathlib import Path

import numpy as np
import pytest

from conftest import gpu_available
import test_gpu_parity as P
from test_second_pass import PASS2_FIXTURES

pytestmark = pytest.mark.gpu

CFG_DIR = Path(__file__).resolve().parent.parent / 'marl-factory-grid_amd' / 'mfg_amd' / 'configs'
BATCHED = [('pass2_mix.yaml', 90, 4), ('pass2_bound.yaml', 70, 6), ('cap_maint64.yaml', 110, 8)]
FUSED = ['pass2_mix.yaml', 'pass2_bound.yaml']


# ---- 1. the reference fixtures at B = 1 ----
@pytest.mark.parametrize('tag,cfg,seed', PASS2_FIXTURES)
def test_engine_vs_second_pass_fixture(tag, cfg, seed):
    P.test_engine_vs_reference_fixture(tag, cfg, seed)


# ---- 2. batched against the oracle, across auto-resets ----
@pytest.mark.parametrize('stagger', [None, 5])
@pytest.mark.parametrize('cfg,steps,B', BATCHED)
def test_engine_vs_oracle_second_pass_batched(cfg, steps, B, stagger):
    P.test_engine_vs_oracle_batched(cfg, steps, B, stagger=stagger)


@pytest.mark.parametrize('variant', [{'pairs_lds': 4}, {'bfs_hbm': 1}, {'render_slots': 2}], ids=lambda v: next(iter(v)))
def test_engine_vs_oracle_pass2_mix_variant(variant):
    """Identifier-collision pairs spilled to HBM, the maintainers' BFS scratch in HBM, and fewer render waves than envs:
    each changes a path that the second pass goes through."""
    P.test_engine_vs_oracle_batched('pass2_mix.yaml', 90, 4, variant)


# ---- 3. fused and narrow outputs ----
@pytest.mark.parametrize('cfg', FUSED)
def test_fused_k8_equals_k1_second_pass(cfg):
    import test_gpu_timed_path as T
    T.test_fused_k8_equals_k1(cfg, 2, 16)


@pytest.mark.parametrize('cfg', FUSED)
def test_f32_obs_equal_the_oracle_cast(cfg):
    """Two K = 8 calls with float32 obs: rewards, done, events, obs == the oracle's f64 obs cast to float32, and the
    MT state and floor order after each call."""
    import test_gpu_timed_path as T
    T._timed_path(np.float32, cfg, B=2, calls=2, idx=[0, 1])


@pytest.mark.parametrize('cfg', FUSED)
def test_packed_obs_match_dense_second_pass(cfg):
    """Packed rows == the dense f32 obs (the comparison of test_marl.test_packed_obs_matches_dense), B = 2, the reset
    and two K = 8 calls; no row is truncated."""
    if not gpu_available():
        pytest.skip('no GPU')
    import torch
    import test_marl as M
    B, K, cap = 2, 8, 1024
    spec, dense, packed, po, w, b = M._engine_pair(cfg, B, K, cap=cap)
    obs = torch.zeros(dense.obs_shape(K), dtype=torch.float32, device='cuda')
    dense.reset(obs=obs[0], init=True, seed_base=5)
    packed.reset(obs=po.view(0), init=True, seed_base=5)
    M._check_rows(obs[0], po, w, b, 0)
    for it in range(2):
        dense.step(K, philox_seed=9, step_base=1 + it * K, obs=obs, auto_reset=True)
        packed.step(K, philox_seed=9, step_base=1 + it * K, obs=po, auto_reset=True)
        for k in range(K):
            M._check_rows(obs[k], po, w, b, k)
        assert 0 < int(po.count.max()) <= cap, 'a packed row was truncated'
        po.check()
    dense.close()
    packed.close()


# ---- 4. the exported record ----
def _exported_vs_oracle(cfg, B, steps, extra):
    """Every env's exported record, decoded by views.snapshot_from_record, against views_compare.oracle_snapshot after
    the reset and after every tenth step of an auto-reset run; extra(rv, snap, ref, where) per comparison."""
    import oracle as O
    import views_compare as V
    from philox import synthetic_actions
    from mfg_amd.engine import RecordView
    from mfg_amd.views import snapshot_from_record
    base, pseed = 1000, 7
    torch, spec, eng = P._engine(cfg, B)
    eng.reset(init=True, seed_base=base)
    envs = [O.OracleEnv(spec, base + i) for i in range(B)]
    for e in envs:
        e.reset()
    done = torch.zeros((1, B), dtype=torch.uint8, device=eng.device)

    def compare(where):
        st = eng.export_state().cpu().numpy()
        for i, env in enumerate(envs):
            rv = RecordView(st[i], eng.layout, spec)
            snap, ref = snapshot_from_record(rv, None), V.oracle_snapshot(env)
            assert [c for c, _, _ in snap.agents] == [c for c, _, _ in ref.agents], f'{where} env {i}: agent cells'
            for f in ('step', 'battery', 'doors', 'items', 'pods', 'drops', 'dests', 'dirt', 'machines', 'maints'):
                assert getattr(snap, f) == getattr(ref, f), f'{where} env {i}: {f} differ'
            extra(rv, snap, ref, f'{where} env {i}')

    compare('reset')
    for t in range(steps):
        eng.step(1, actions=None, philox_seed=pseed, step_base=t, done=done, auto_reset=True)
        acts = synthetic_actions(pseed, np.arange(B), t, spec.n_actions)
        for i, env in enumerate(envs):
            _, d, _ = env.step(acts[i], with_obs=False)
            assert bool(done[0, i].item()) == d, f't{t} env {i} done'
            if d:
                env.reset()
        if t % 10 == 9:
            compare(f't{t}')
    eng.close()
    return spec


def test_exported_caps_match_oracle():
    """All 64 maintainer and all 30 machine slots of cap_maint64."""
    upper = set()

    def extra(rv, snap, ref, where):
        assert rv.hdr('n_maints') == 64 == len(snap.maints) and rv.hdr('n_machines') == 30 == len(snap.machines), where
        upper.update((where.split()[-1], k, cell) for k, (_, cell) in enumerate(snap.maints) if k >= 32)

    _exported_vs_oracle('cap_maint64.yaml', 4, 30, extra)
    assert len(upper) > 2 * 4 * 32, 'the maintainers of slots 32..63 hardly moved between the comparisons'


def test_exported_second_pass_agents_match_oracle_mix():
    """pass2_mix: the batteries of agents 64..69 (each its own f64 level below 1.0 once the episode runs) and the items,
    those picked up included (cell none: upstream an inventory never holds what its agent picked up)."""
    seen = dict(levels=set(), picked=0)

    def extra(rv, snap, ref, where):
        assert snap.battery[64:] == ref.battery[64:] and len(snap.battery) == 70, where
        seen['levels'].update(snap.battery[64:])
        seen['picked'] += sum(1 for _, cell in ref.items if cell < 0)

    _exported_vs_oracle('pass2_mix.yaml', 3, 30, extra)
    assert len(seen['levels']) > 6 and min(seen['levels']) < 1.0, 'the batteries of agents >= 64 never drained apart'
    assert seen['picked'] > 0, 'no item was ever picked up'


def test_exported_second_pass_agents_match_oracle_bound():
    """pass2_bound: SpawnDestinationsPerAgent makes one destination per entry, bound to the entry's agent: Karl (64),
    Heinz_the_2nd (68) and Swarm_the_5th (6). Slot order, cells, reached flags, and the binding itself (the record's
    EW_BOUND field against the spec's entries); Karl's lies on one of his two configured cells."""
    from mfg_amd.spec import compile_spec
    spec = compile_spec('pass2_bound.yaml')
    want_bound = [a for a, _, _ in spec.dest_entries]
    assert want_bound == [64, 68, 6]
    karl_cells = set(spec.dest_entries[0][2])

    def extra(rv, snap, ref, where):
        words = [int(x) for x in rv.group('dests')]
        assert [((w >> 20) & 0xFF) - 1 for w in words] == want_bound, f'{where}: bound agents'
        assert len(snap.dests) == 3 and snap.dests[0][1] in karl_cells, where

    _exported_vs_oracle('pass2_bound.yaml', 4, 30, extra)


# ---- 5. consumers of the second pass and of the high maintainer word ----
def test_mask_against_the_step_pass2_mix():
    """test_gpu_action_mask's fan-out (one row per agent and slot; the step's ev_act valid bits are the mask) on states
    of pass2_mix in which an agent >= 64 stands alone on a charge pod, on an item, on a dirt pile and on a machine,
    with every battery lowered to 0.5 as test_mask_against_the_step_with_low_batteries does. Charge, ItemAction and
    Clean must show valid for that agent, MachineAction never (upstream it cannot succeed)."""
    import torch
    import action_mask_ref as M
    import test_gpu_action_mask as AM
    from mfg_amd import abi
    from mfg_amd.engine import RecordView
    AM._need_gpu()
    spec, eng = AM._stepped_engine('pass2_mix.yaml', 9)
    A, L = spec.n_agents, eng.layout
    assert A == 70 and eng.B == sum(spec.n_actions)
    state = eng.export_state()
    ob = L['o_battery']
    bat = torch.full((eng.B, A), 0.5, dtype=torch.float64, device='cuda')
    state[:, ob:ob + 8 * A] = bat.view(torch.uint8).view(eng.B, 8 * A)
    host = state.cpu().numpy()
    ok = AM._header(eng, state, 'crashed') == 0
    ops = M.slot_ops(spec)
    hi = range(64, A)
    want = {}  # op -> (env, agent)
    for b in np.nonzero(ok)[0]:
        v = RecordView(host[b], L, spec)
        pos = [int(p) for p in v.agent_pos()]

        def cells(words, flag=0x10000):
            return set(int(w) & 0xFFFF for w in words if int(w) & flag)
        pods, items, drops = cells(v.group('pods')), cells(v.group('items')), cells(v.group('drops'))
        dirt = cells(v.dirt()[0], 0x20000)
        machines = cells(v.i32(L['o_machines'], v.hdr('n_machines')))
        for a in hi:
            if pos[a] in pods and pos.count(pos[a]) == 1:
                want.setdefault(abi.ACT_CHARGE, (int(b), a))
            if pos[a] in items and pos[a] not in drops:
                want.setdefault(abi.ACT_ITEM, (int(b), a))
            if pos[a] in dirt:
                want.setdefault(abi.ACT_CLEAN, (int(b), a))
            if pos[a] in machines:
                want.setdefault(abi.ACT_MACHINE, (int(b), a))
        if len(want) == 4:
            break
    assert len(want) == 4, f'the probed states miss a case for agents >= 64: found {sorted(want)}'
    for op, (b, a) in want.items():
        got, stepped = AM._fan_out(eng, spec, state[b].clone())
        assert np.array_equal(got, stepped), (op, b, got, stepped)
        assert bool((got[a] >> ops[a].index(op)) & 1) == (op != abi.ACT_MACHINE), (op, b, a, got[a])
        for x in hi:
            assert not (got[x] >> ops[x].index(abi.ACT_MACHINE)) & 1 and (got[x] >> spec.n_actions[x]) == 0
    eng.close()


@pytest.mark.parametrize('cfg,B', [('pass2_mix.yaml', 3), ('cap_maint64.yaml', 5)])
def test_step_columns_with_the_high_maintainer_word(cfg, B):
    import test_gpu_info_monitor as IM
    IM.test_step_columns_equal_torch_columns(cfg, B, None, min_maint_slot=32)


def test_recorder_device_rows_pass2_mix():
    import test_gpu_recorder as R
    R.test_device_rows_equal_pack_row('pass2_mix.yaml', 3, 30, (2, 0))


def test_recorder_records_pass2_mix():
    import test_gpu_recorder as R
    R.test_records_equal_oracle('pass2_mix.yaml', 3, 30, (2, 0))


# ---- 6. one more than the caps ----
@pytest.mark.parametrize('group,q', [('Maintainers', 65), ('Machines', 31)])
def test_engine_refuses_more_than_the_caps(tmp_path, group, q):
    """mfg_create refuses the spec, naming the group, before any kernel is launched."""
    from mfg_amd.spec import compile_spec
    from mfg_amd.engine import Engine
    P._engine('simple1.yaml', 1)[2].close()  # (skips without a GPU)
    text = (CFG_DIR / 'cap_maint64.yaml').read_text()
    new, n = re.subn(rf'^(  {group}: \{{coords_or_quantity: )\d+', rf'\g<1>{q}', text, flags=re.M)
    assert n == 1
    p = tmp_path / f'cap_{group}_{q}.yaml'
    p.write_text(new)
    spec = compile_spec(str(p))
    with pytest.raises(RuntimeError, match=group):
        Engine(spec, 2)
