"""GPU: items, charge pods, drop-off locations and destinations above 64 slots per env (up to MFG_MAX_GROUP = 128): the
two-pass step / reset kernels, the long-ray render's two-word identifier-dedupe sets and the host views, against the
reference fixtures and the C oracle (bit-exact, through the checkers of test_gpu_parity.py).
  cap_groups: 128 items, 70 charge pods, 65 drop-offs, 66 destinations, 8 agents; the identifier spaces overlap, so the
              dedupe pairs involve slots >= 64 and spill past the LDS pair capacity.
  cap_dest81: 81 blocking agents on large_qquad, each with a bound destination (slots and EW_BOUND values above 64)."""
import random

import numpy as np
import pytest

from conftest import gpu_available
import golden_compare as G
import test_gpu_parity as P

pytestmark = pytest.mark.gpu

CAP_FIXTURES = [('cap_groups', 'cap_groups.yaml'), ('cap_dest81', 'cap_dest81.yaml')]


@pytest.mark.parametrize('tag,cfg', CAP_FIXTURES)
@pytest.mark.parametrize('seed', [0, 1])
def test_engine_vs_cap_fixture(tag, cfg, seed):
    P.test_engine_vs_reference_fixture(tag, cfg, seed)


@pytest.mark.parametrize('cfg,steps,B,stagger', [('cap_groups.yaml', 130, 8, None), ('cap_dest81.yaml', 90, 4, None),
                                                 ('cap_groups.yaml', 70, 4, 5)])
def test_engine_vs_oracle_cap_batched(cfg, steps, B, stagger):
    P.test_engine_vs_oracle_batched(cfg, steps, B, stagger=stagger)


def test_engine_vs_oracle_cap_pair_spill():
    """Four LDS pairs: nearly every identifier-collision pair, those with suppressed slots >= 64 included, lives in the
    HBM spill."""
    P.test_engine_vs_oracle_batched('cap_groups.yaml', 70, 4, {'pairs_lds': 4})


def test_exported_groups_match_oracle():
    """The exported record, decoded by RecordView / views.snapshot_from_record, holds every slot of the four groups as
    the oracle env does: identifier, cell (or none: an item picked up) and the destinations' reached flag per alive
    slot, and the present bit = the entity is in the oracle's global pos_dict at its cell. Compared after the reset
    and after every tenth step of a batched auto-reset run (episode ends at 60 and 120)."""
    import oracle as O
    import views_compare as V
    from philox import synthetic_actions
    from mfg_amd.engine import RecordView
    from mfg_amd.views import EW_ALIVE, EW_PRESENT, snapshot_from_record
    B, steps, base, pseed = 8, 130, 1000, 7
    torch, spec, eng = P._engine('cap_groups.yaml', B)
    eng.reset(init=True, seed_base=base)
    envs = [O.OracleEnv(spec, base + i) for i in range(B)]
    for e in envs:
        e.reset()
    done = torch.zeros((1, B), dtype=torch.uint8, device=eng.device)
    names = {'items': ('Item', 'item_base'), 'pods': ('ChargePod', 'pod_base'),
             'drops': ('DropOffLocation', 'drop_base'), 'dests': ('Destination', 'dest_base')}
    want_n = {'items': 128, 'pods': 70, 'drops': 65, 'dests': 66}
    picked = 0

    def compare(where):
        nonlocal picked
        st = eng.export_state().cpu().numpy()
        for i, env in enumerate(envs):
            rv = RecordView(st[i], eng.layout, spec)
            snap, ref = snapshot_from_record(rv, None), V.oracle_snapshot(env)
            pd = env.posdict()
            for g, (cls, base_key) in names.items():
                assert getattr(snap, g) == getattr(ref, g), f'{where} env {i}: {g} slots differ'
                w = rv.group(g)
                assert len(w) == want_n[g], f'{where} env {i}: {g} has {len(w)} slots'
                b = rv.hdr(base_key)
                for k, x in enumerate(int(x) for x in w):
                    here = f'{cls}[{b + k}]' in pd.get(x & 0xFFFF, [])
                    assert bool(x & EW_PRESENT) == (bool(x & EW_ALIVE) and here), f'{where} env {i}: {g} slot {k} present'
            picked += sum(1 for _, cell in snap.items[64:] if cell < 0)

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
    assert picked > 0, 'no item of slots 64..127 was ever picked up: the run does not cover the second pass'


def test_facade_replays_cap_groups():
    if not gpu_available():
        pytest.skip('no GPU')
    from mfg_amd.factory import Factory
    rec, _ = G.load('cap_groups', 0)
    random.seed(rec['py_seed'])
    env = Factory('cap_groups.yaml')
    assert env.named_action_space == rec['named_action_space']
    nl = env.spec.n_layers
    errs = []
    for r in rec['steps']:
        t = r['t']
        if r['step'] == 0:
            obs = list(env.reset().values())
        else:
            _, obs, reward, done, info = env.step(list(r['actions']))
            if reward != r['reward'] or done != r['done']:
                errs.append((t, 'reward/done', reward, r['reward']))
            ok, bad = G.info_equal(info, r['info'])
            if not ok:
                errs.append((t, 'info', bad))
        if G.sha(G.obs_bytes([np.asarray(x)[:nl[a]] for a, x in enumerate(obs)])) != r['obs_sha']:
            errs.append((t, 'obs'))
        st = np.asarray(random.getstate()[1], dtype=np.uint32)
        if G.sha(st.tobytes()) != r['mt']:
            errs.append((t, 'python random state'))
        if len(errs) > 10:
            break
    env.close()
    assert not errs, errs[:10]


def test_packed_obs_matches_dense_cap_groups():
    """Packed rows == the dense f32 obs (the comparison of test_marl.test_packed_obs_matches_dense), B = 4, 20 steps."""
    import torch
    import test_marl as M
    B, K = 4, 4
    spec, dense, packed, po, w, b = M._engine_pair('cap_groups.yaml', B, K, cap=512)
    obs = torch.zeros(dense.obs_shape(K), dtype=torch.float32, device='cuda')
    dense.reset(obs=obs[0], init=True, seed_base=5)
    packed.reset(obs=po.view(0), init=True, seed_base=5)
    M._check_rows(obs[0], po, w, b, 0)
    for it in range(5):
        dense.step(K, philox_seed=9, step_base=1 + it * K, obs=obs, auto_reset=True)
        packed.step(K, philox_seed=9, step_base=1 + it * K, obs=po, auto_reset=True)
        for k in range(K):
            M._check_rows(obs[k], po, w, b, k)
    po.check()
    dense.close()
    packed.close()


@pytest.mark.parametrize('cfg', ['agents81.yaml', 'large8.yaml'])
def test_old_dispatch_still_works(cfg):
    """Specs with every group <= 64 keep their instantiations (one pass for large8, the agent passes for agents81)."""
    P.test_engine_vs_oracle_batched(cfg, 60, 8)
