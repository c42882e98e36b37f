"""Checkpoint / resume (include/mfg.h mfg_export_state / mfg_import_state) against the C oracle's uninterrupted run.

Engine X is created, reset and stepped t1 times, the last d of them with MFG_STEP_DEFER_REPLAY, so the snapshot taken
straight after (same stream, no synchronize) holds pending shuffle debt: an MT state and floor order that are not the
reference's. X is closed. Engine Y is a fresh engine that is never reset: it imports the snapshot (whole or a run of
rows, possibly with another mfg_variant of the same record layout) and goes on stepping with step_base = t1 + k and
env_base = its first row. Every step of Y is compared with the oracle env of the same global index, which was stepped
t1 + k times without any interruption: rewards with ==, done, the event fields, f64 obs bit for bit; after every call
the MT19937 state and index, floor order, PCG64 state and a debt of 0. The truth is never engine X.

What a resume has to survive lies outside the record: the host's done-list parity (X's is t1 & 1, Y's 0), the two done
lists and their counters, the done flags, the replay order buffers and the per-env HBM pools (BFS scratch, pair spill,
long-ray render slots), all of which Y has as mfg_create left them.
"""
import numpy as np
import pytest

from conftest import gpu_available
import oracle_compare as OC

pytestmark = pytest.mark.gpu

BASE, PSEED = 1000, 7


def _need_gpu():
    if not gpu_available():
        pytest.skip('no GPU')
    import torch
    return torch


def _x_calls(t1, d, stagger):
    """Engine X's calls [(step_base, K, defer)]: K = 8 where the steps up to the stagger / the deferred tail allow it,
    K = 1 for the rest; the last d steps one by one with the replay deferred."""
    assert d >= 1 and (stagger is None or 0 < stagger <= t1 - d)
    calls, cuts = [], sorted({0, t1 - d} | ({stagger} if stagger is not None else set()))
    for lo, hi in zip(cuts, cuts[1:]):
        t = lo
        while t < hi:
            K = 8 if hi - t >= 8 else 1
            calls.append((t, K, False))
            t += K
    return calls + [(t, 1, True) for t in range(t1 - d, t1)]


def _y_calls(t2, fused=None):
    """Engine Y's K per call: a plain K = 1 step first (it pays the imported debt), then `fused` once if given, then
    K = 1 and K = 3 in turn (the last one cut to fit t2)."""
    ks, pattern = [1] + ([fused] if fused else []), [1, 3]
    while sum(ks) < t2:
        ks.append(min(pattern[len(ks) % 2], t2 - sum(ks)))
    assert sum(ks) == t2
    return ks


def _same_layout(lx, ly):
    """The record layouts of two engines (Engine.layout) are equal: the size and every offset."""
    assert lx['size'] == ly['size']
    for k in lx:
        if k.startswith('o_'):
            assert lx[k] == ly[k], f'record offset {k} differs between the two engines'


def _snapshot_checks(snap, layout, ob, straddle, debt=True):
    """What keeps a case from passing vacuously: the imported rows carry debt and are not the reference's state; their
    episode counters (0 in an env's first episode) are the oracle's, and with straddle == 'later' some env is past its
    first episode at the checkpoint. debt=False: the one case whose last step before the checkpoint pays every env's
    debt inside the step; what it asserts instead is exactly that."""
    from mfg_amd.engine import RecordView
    rvs = [RecordView(snap[j], layout, ob.spec) for j in range(len(ob.envs))]
    if debt:
        assert any(rv.hdr('debt') > 0 for rv in rvs), 'no imported record carries shuffle debt: lengthen the deferred tail'
        assert any(not np.array_equal(rv.mt(), e.mt_state()) or not np.array_equal(rv.perm(), e.floor())
                   for rv, e in zip(rvs, ob.envs)), 'the snapshot already holds the reference MT state and floor order'
    else:
        assert not OC.state_errors(snap, layout, ob)
    assert all(rv.hdr('crashed') == 0 for rv in rvs)
    assert [rv.hdr('episode') for rv in rvs] == [int(e.header()[1]) for e in ob.envs]
    if straddle == 'later':
        assert any(rv.hdr('episode') > 0 for rv in rvs)


def _step_y(torch, Y, ob, buf, ks, t1, env_base):
    """Y's calls after the import, every step and the records after every call against the oracle batch."""
    t = t1
    for c, K in enumerate(ks):
        assert ob.t == t
        Y.step(K, actions=None, philox_seed=PSEED, env_base=env_base, step_base=t, auto_reset=True,
               **{k: v[:K] for k, v in buf.items()})
        OC.compare_call(f'call {c} (K = {K})', ob, OC.rows_of(buf, K), K)
        t += K
        OC.check_state(f'after call {c} (step {t})', Y.export_state().cpu().numpy(), Y.layout, ob)


def _resume_case(cfg, B, t1, d, t2, stagger=None, rows=None, x_variant=None, y_variant=None, fused=None,
                 straddle='later', base=BASE, env0=0, debt=True):
    """X: B envs, t1 steps (the last d deferred, the odd envs reset before step `stagger`), export, close. Y: an engine
    over `rows` (a range of X's rows, default all) that imports them and steps t2 more times against the oracle.
    X's row b is the global env env0 + b: seeded base + env0 + b, its Philox key env0 + b.
    straddle: 'later' = an episode ends in the compared steps and some env is past its first episode at the checkpoint,
    'first' = an episode ends in the compared steps and the checkpoint lies in every env's first one, None = neither."""
    torch = _need_gpu()
    from mfg_amd.spec import compile_spec
    from mfg_amd.engine import Engine
    spec = compile_spec(cfg)
    rows = range(B) if rows is None else rows
    r0, r1 = rows[0], rows[-1] + 1
    ob = OC.OracleBatch(spec, [env0 + r for r in rows], base, PSEED)
    X = Engine(spec, B, variant=x_variant)
    X.reset(init=True, seed_base=base + env0)
    ob.reset()
    for t, K, defer in _x_calls(t1, d, stagger):
        if t == stagger:
            X.reset(mask=(torch.arange(B, device=X.device) + env0).remainder(2).to(torch.uint8))
            ob.reset(odd_only=True)
        X.step(K, actions=None, philox_seed=PSEED, env_base=env0, step_base=t, auto_reset=True, defer_replay=defer)
        ob.run(K)
    snap = X.export_state()  # straight after the step: the join of X's second stream is part of what is tested
    mask_x = X.action_mask()[r0:r1].cpu().numpy()
    layout_x = dict(X.layout)
    X.close()
    assert ob.t == t1
    _snapshot_checks(snap[r0:r1].cpu().numpy(), layout_x, ob, straddle, debt)

    Y = Engine(spec, r1 - r0, variant=y_variant)  # never reset
    _same_layout(layout_x, Y.layout)
    Y.import_state(snap[r0:r1])
    assert np.array_equal(Y.action_mask().cpu().numpy(), mask_x), 'action mask of the imported rows'
    buf = OC.make_buffers(torch, Y, max(3, fused or 0))
    _step_y(torch, Y, ob, buf, _y_calls(t2, fused), t1, env0 + r0)
    Y.close()
    if straddle:
        assert ob.ended.sum() >= 1, 'no env finished an episode in the compared steps'
    else:
        assert ob.ended.sum() == 0
    ob.close()
    return ob


# cfg, B, t1, d, t2, stagger, Y's variant, K of Y's second call, straddle (_resume_case)
CASES = [
    ('eval_trio.yaml', 16, 15, 3, 16, 5, None, None, 'later'),
    # even t1: the same done-list parity on both sides. After 16 steps no deferred tail of any length leaves debt:
    # eval_trio's RespawnDirt (respawn_freq 15, counted over the env's lifetime) fires in step 15 of every env and pays
    # the whole debt inside that step (NO_DEBT below). After 18 steps the tail of 2 does.
    ('eval_trio.yaml', 16, 16, 1, 14, 5, None, None, 'later'),
    ('eval_trio.yaml', 16, 18, 2, 14, 5, None, None, 'later'),
    ('grid128_full_ep.yaml', 7, 15, 2, 14, 5, {'render_slots': 2}, None, 'later'),
    ('agents81.yaml', 3, 55, 3, 8, None, None, None, 'first'),
    ('cap_groups.yaml', 4, 57, 2, 6, None, None, None, 'first'),
    ('cap_maint64.yaml', 4, 47, 2, 6, None, None, None, 'later'),
    ('alltest16.yaml', 8, 495, 5, 12, None, None, None, 'later'),
    ('large8.yaml', 8, 495, 7, 16, None, None, 8, 'first'),
    ('grid128_64.yaml', 2, 9, 4, 8, None, None, None, None),
]
NO_DEBT = {('eval_trio.yaml', 16)}


@pytest.mark.parametrize('cfg,B,t1,d,t2,stagger,y_variant,fused,straddle', CASES,
                         ids=[f'{c[0][:-5]}-t{c[2]}' for c in CASES])
def test_resume_in_a_fresh_engine(cfg, B, t1, d, t2, stagger, y_variant, fused, straddle):
    from mfg_amd.spec import compile_spec
    ms = OC.max_steps(compile_spec(cfg))
    if straddle:  # the checkpoint lies inside an episode that ends (max_steps) in the compared steps
        assert t1 % ms and t1 % ms + t2 >= ms
    ob = _resume_case(cfg, B, t1, d, t2, stagger=stagger, y_variant=y_variant, fused=fused, straddle=straddle,
                      debt=(cfg, t1) not in NO_DEBT)
    if stagger is not None:
        # 12-step episodes, the odd envs restarted before step 5: at the checkpoint the even envs are in episode 2, the
        # odd ones in their restarted episode 1, and every env of both groups ends an episode in the compared steps
        assert ms == 12 and t1 > ms and t2 >= ms and ob.ended.min() >= 1
    if cfg == 'large8.yaml':
        assert ob.ended.min() >= 1  # the step-500 mass reset: every env went through Y's done list
    if cfg == 'alltest16.yaml':
        assert ob.dirt_rises >= 1, 'no RespawnDirt spawn in the compared steps'


@pytest.mark.parametrize('cfg,B,t1,d,t2,stagger,rows', [('eval_trio.yaml', 16, 15, 3, 16, 5, range(6, 11)),
                                                      ('large8.yaml', 8, 495, 7, 16, None, range(5, 8))],
                         ids=['eval_trio-rows6to10', 'large8-rows5to7'])
def test_resume_a_slice_of_the_rows(cfg, B, t1, d, t2, stagger, rows):
    """A record holds nothing about its index (mfg_amd/shard.py moves rows between engines): a smaller engine imports a
    run of rows and steps them with env_base = the first row's global index."""
    _resume_case(cfg, B, t1, d, t2, stagger=stagger, rows=rows, fused=8 if cfg == 'large8.yaml' else None,
                 straddle='later' if stagger else 'first')


@pytest.mark.parametrize('cfg,B,t1,d,t2,stagger,xv,yv', [
    ('alltest16.yaml', 8, 495, 5, 12, None, None, {'serial': 1}),
    ('eval_trio.yaml', 16, 15, 3, 16, 5, None, {'shuffle_table_path': 1}),
    ('grid128_full_ep.yaml', 7, 15, 2, 14, 5, {'serial': 1}, None)],
    ids=['alltest16-to-serial', 'eval_trio-to-table-path', 'grid128_full_ep-from-serial'])
def test_resume_across_variants(cfg, B, t1, d, t2, stagger, xv, yv):
    """A snapshot of one mfg_variant resumes in another of the same record layout."""
    _need_gpu()
    from mfg_amd.spec import compile_spec
    from mfg_amd.engine import Engine
    spec = compile_spec(cfg)
    x, y = Engine(spec, 2, variant=xv), Engine(spec, 2, variant=yv)
    _same_layout(x.layout, y.layout)
    x.close()
    y.close()
    if cfg == 'alltest16.yaml':
        # global envs 644 .. 651 seeded 644 .. 651: none ends an episode before step 495 (the oracle's rollout), so the
        # step-500 mass reset puts every env on Y's done list at once
        ob = _resume_case(cfg, B, t1, d, t2, x_variant=xv, y_variant=yv, straddle='first', base=0, env0=644)
        assert ob.ended.min() >= 1
    else:
        _resume_case(cfg, B, t1, d, t2, stagger=stagger, x_variant=xv, y_variant=yv)


def test_resume_with_pending_done_and_no_auto_reset():
    """eval_trio without auto-reset up to the step that sets done for every env (max_steps); the snapshot is imported by
    a fresh engine, whose mfg_reset(mask = done, init = 0) gives the oracle's reset obs; 13 more steps follow."""
    torch = _need_gpu()
    from mfg_amd.spec import compile_spec
    from mfg_amd.engine import Engine
    cfg, B, d = 'eval_trio.yaml', 8, 2
    spec = compile_spec(cfg)
    t1 = OC.max_steps(spec)
    ob = OC.OracleBatch(spec, list(range(B)), BASE, PSEED)
    X = Engine(spec, B)
    X.reset(init=True, seed_base=BASE)
    ob.reset()
    done = torch.zeros((1, B), dtype=torch.uint8, device=X.device)
    for t in range(t1):
        X.step(1, actions=None, philox_seed=PSEED, step_base=t, done=done, auto_reset=False, defer_replay=t >= t1 - d)
        ref_done = ob.run(1, auto_reset=False)
        assert ref_done.all() == (t == t1 - 1)
    snap = X.export_state()
    assert done[0].cpu().numpy().all()
    layout_x = dict(X.layout)
    X.close()
    _snapshot_checks(snap.cpu().numpy(), layout_x, ob, None)

    Y = Engine(spec, B)
    _same_layout(layout_x, Y.layout)
    Y.import_state(snap)
    buf = OC.make_buffers(torch, Y, 3)
    Y.reset(obs=buf['obs'][0], mask=done[0].clone())
    got, want = buf['obs'][0].cpu().numpy(), ob.reset()
    for j in range(B):
        OC.compare_obs(f'reset obs env {j}', spec, got[j], want[j])
    _step_y(torch, Y, ob, buf, _y_calls(13), t1, 0)
    Y.close()
    assert ob.ended.min() >= 1  # 13 > max_steps: every env ended its new episode too
    ob.close()
