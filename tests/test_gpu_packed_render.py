"""The packed render (MFG_OBS_PACKED: build_obs<..., PK = 1 | 2> in csrc/mfg_kernels.h, dispatched by launch_obs in
csrc/mfg_engine.hip) against the C oracle, at every placement shape (per-layer ballots with short rays, the flattened
pass, per-layer ballots over several 64-cell blocks, the long-ray render), entries only (PK 1) and with the fused
projection (PK 2), single- and multi-wave, on rows of more than 64 and more than 128 entries: the 64-entry queue is
flushed inside the row, so the stored slots start at qbase > 0, a cap can fall inside a later flush, and the projection
accumulators are carried over flushes. tests/test_packed_render_cases.py holds the cases, their oracle runs (shared,
computed once) and what those runs must contain.

A run: B envs seeded BASE + i on the Philox actions with auto-reset, every (step, env, agent) row against
float32(oracle obs) of that env and agent. Criteria per row (include/mfg.h mfg_packed_obs,
tests/test_gpu_learn_kernels.py):
  * count == the float32 nonzero count of the oracle row;
  * the stored slots hold the first min(count, cap) nonzero entries in mfg.h's order, values bit-equal to
    float32(oracle); slots from count up to cap are 0 / 0.0;
  * |emb - ref| <= (n + 2) 2^-24 S, ref the f64 product of the f32 row with the f32 weights plus the bias, n the row's
    count, S = |bias| + sum |v| |w| (sequential f32 fma), over ALL entries also where the stored row is truncated;
  * idx, val, count and emb live between guard words that keep their sentinel, and no slot inside keeps the sentinel
    the buffers were filled with (idx 0xFFFF: the row is narrower than 65535; val and emb a NaN; count -1);
  * rendering the same state twice (mfg_reset with an all-zero mask: every env rendered, none reset) gives equal bits.
Every case prints its largest err / bound; with MFG_PACKED_FIGURES set to a file name the figures are written there as
JSON (profiles/packed_render.json is one such run on an MI355X)."""
import json
import os
from pathlib import Path

import numpy as np
import pytest

from conftest import gpu_available
import test_packed_render_cases as PC
from test_packed_render_cases import BASE, CASES, PSEED

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
GUARD = 64
NAN_BITS = 0x7FC0DEAD  # a quiet NaN no render produces
FIGURES = {}


def _keep(run, fig):
    """Per test: its largest err / bound and the facts of each of its runs."""
    test = os.environ.get('PYTEST_CURRENT_TEST', run).split('::')[-1].split(' ')[0]
    rec = FIGURES.setdefault(test, dict(err_over_bound=0.0, runs={}))
    rec['err_over_bound'] = max(rec['err_over_bound'], fig['err_over_bound'])
    rec['runs'][run] = fig
    print(f'{test}: {run}: {fig}')
    dst = os.environ.get('MFG_PACKED_FIGURES')
    if dst:
        Path(dst).write_text(json.dumps(FIGURES, indent=1))


class Guarded:
    """The four output arrays of a PackedObs re-homed into sentinel-filled buffers with GUARD words on both sides."""
    FILL = {'idx': ('int16', -1), 'val': ('int32', NAN_BITS), 'count': ('int32', -1), 'emb': ('int32', NAN_BITS)}

    def __init__(self, torch, po):
        self.torch, self.po, self.raw = torch, po, {}
        for f, (bits, fill) in self.FILL.items():
            t = getattr(po, f)
            if t is None:
                continue
            raw = torch.empty(t.numel() + 2 * GUARD, dtype=t.dtype, device=t.device)
            self.raw[f] = raw
            setattr(po, f, raw[GUARD:GUARD + t.numel()].view(t.shape))
        self.refill()
        po.desc = po._make_desc()

    def refill(self):
        for f, raw in self.raw.items():
            bits, fill = self.FILL[f]
            raw.view(getattr(self.torch, bits)).fill_(fill)

    def bits(self, f):
        """The whole buffer of array f, guards included, as host integers."""
        return self.raw[f].view(getattr(self.torch, self.FILL[f][0])).cpu().numpy()

    def check_guards(self, what):
        for f in self.raw:
            b, fill = self.bits(f), np.array(self.FILL[f][1]).astype(self.FILL[f][0])
            assert (b[:GUARD] == fill).all() and (b[-GUARD:] == fill).all(), f'{what}: a guard word of {f} was written'

    def rows(self, k, what, untouched=False):
        """Row k of every array as host arrays (val and emb as their bits); every slot written (or, untouched, none)."""
        out = {}
        for f in self.raw:
            t = getattr(self.po, f)[k]
            b = t.contiguous().view(getattr(self.torch, self.FILL[f][0])).cpu().numpy()
            fill = np.array(self.FILL[f][1]).astype(self.FILL[f][0])
            if untouched:
                assert (b == fill).all(), f'{what}: {f} was written'
            else:  # (an idx of 0xFFFF cannot occur: lmax*h*w <= 65535)
                assert (b != fill).all(), f'{what}: {int((b == fill).sum())} slots of {f} were not written'
            out[f] = b.view(np.uint16) if f == 'idx' else b
        return out


def check_rows(spec, maxpts, ref, got, cap, wt64, b64, what):
    """One render's rows `got` (Guarded.rows) against the oracle's f32 rows ref [B][A][kdim]; returns the largest
    err / bound of the projection (None without emb)."""
    B, A, kdim = ref.shape
    dd = spec.obs_hw[0] * spec.obs_hw[1]
    blocks = PC.block_order(maxpts, dd)
    n_ref = PC.counts(ref)
    if 'count' in got:
        bad = np.argwhere(got['count'] != n_ref)
        assert not len(bad), f'{what}: count of (env, agent) {bad[:4].tolist()} is ' \
                             f'{[int(got["count"][tuple(x)]) for x in bad[:4]]}, ' \
                             f'oracle {[int(n_ref[tuple(x)]) for x in bad[:4]]}'
    if 'idx' in got:
        for i in range(B):
            for a in range(A):
                want = PC.expected_idx(ref[i, a], dd, blocks)
                m = min(len(want), cap)
                gi, gv = got['idx'][i, a], got['val'][i, a]
                dif = gi[:m] != want[:m]
                assert not dif.any(), \
                    f'{what} env{i} agent{a}: stored idx (count {len(want)}, cap {cap}) differ from slot ' \
                    f'{int(np.argmax(dif))}: {gi[:m][dif][:6]} vs {want[:m][dif][:6]}'
                assert (gv[:m] == ref[i, a][want[:m]].view(np.int32)).all(), f'{what} env{i} agent{a}: stored values'
                assert not gi[m:].any() and not gv[m:].any(), \
                    f'{what} env{i} agent{a}: slots past the count are not 0 / 0.0'
    if 'emb' not in got:
        return None
    emb = got['emb'].view(np.float32).astype(np.float64)
    r64 = ref.astype(np.float64)
    want = r64 @ wt64 + b64
    S = np.abs(r64) @ np.abs(wt64) + np.abs(b64)
    bound = (n_ref[..., None] + 2) * EPS * S
    err = np.abs(emb - want)
    assert np.isfinite(emb).all(), f'{what}: emb is not finite'
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    worst = np.unravel_index(np.argmax(ratio), ratio.shape)
    assert ratio.max() <= 1.0, f'{what}: emb (env, agent, j) {worst}: err {err[worst]:.3e} > bound ' \
                               f'{bound[worst]:.3e} (count {n_ref[worst[:2]]})'
    return float(ratio.max())


def _weights(torch, E, kdim, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(E, kdim, generator=g) * 0.1).cuda(), (torch.randn(E, generator=g) * 0.1).cuda()


def render_run(cfg, *, pk=2, K=1, E=96, cap=None, entries=True, count=True, emb_only_count=False,
               waves=None, stagger=None, refresh_at=None, bias='random'):
    """One case: the engine's packed rows of a whole run against the oracle run of CASES[cfg]. Returns the arrays of
    every render [(idx, val, count, emb bits)] for comparisons between runs.
    pk 1: no projection; cap None: the largest row of the run + 7 (every row fits, some slots stay unused);
    waves: mfg_variant.obs_waves; stagger: a masked reset of the odd envs before that step; refresh_at: new projection
    weights (set_projection) before that step; bias 'zero': a zero bias buffer, 'null': NULL in the descriptor;
    emb_only_count: a descriptor with every output NULL but count."""
    if not gpu_available():
        pytest.skip('no GPU')
    import torch
    from mfg_amd.engine import Engine, PackedObs
    c = CASES[cfg]
    B, steps = c['B'], c['steps']
    assert steps % K == 0
    spec, rows, done = PC.oracle_run(cfg, B, steps, stagger)
    n_all = PC.assert_not_vacuous(cfg, rows, done)
    if cap is None:
        cap = int(n_all.max()) + 7
    kdim = rows.shape[-1]
    eng = Engine(spec, B, variant={'obs_waves': waves} if waves else None)
    try:
        lay = eng.layout
        assert lay['obs_maxpts'] == c['maxpts'], f'{cfg}: render instantiated for MAXPTS {lay["obs_maxpts"]}'
        assert lay['obs_waves'] == (waves or c['waves']), f'{cfg}: {lay["obs_waves"]} render waves per env'
        assert kdim == lay['lmax'] * spec.obs_hw[0] * spec.obs_hw[1]
        w = b = None
        if pk == 2:
            w, b = _weights(torch, E, kdim, 1)
            if bias != 'random':
                b = None  # (PackedObs: a zero bias buffer)
        po = PackedObs(eng, K=K, cap=cap, weight=w, bias=b, entries=entries and not emb_only_count,
                       count=count or emb_only_count)
        g = Guarded(torch, po)
        if bias == 'null':  # no buffer: PackedObs.view and _make_desc then leave the descriptor's bias NULL
            po.bias = None
            po.desc = po._make_desc()
            assert po.desc.bias is None and po.desc.emb
        if emb_only_count:
            assert not (po.desc.idx or po.desc.val or po.desc.emb or po.desc.wt) and po.desc.count
        what = f'{cfg} pk{pk} K{K} E{E} cap{cap}' + (f' waves{waves}' if waves else '') + \
            ('' if bias == 'random' else f' bias {bias}') + ('' if entries else ' no entries') + \
            ('' if count else ' no count')

        def ref_w():
            if w is None:
                return None, None
            return po.wt.double().cpu().numpy(), (np.zeros(E) if po.bias is None else po.bias.double().cpu().numpy())

        wt64, b64 = ref_w()
        out, worst = [], 0.0

        def take(k, ref, tag):
            nonlocal worst
            got = g.rows(k, f'{what} {tag}')
            r = check_rows(spec, c['maxpts'], ref, got, cap, wt64, b64, f'{what} {tag}')
            worst = max(worst, r or 0.0)
            out.append(got)

        first = po if K == 1 else po.view(0)  # (a reset renders one row)
        g.refill()
        eng.reset(obs=first, init=True, seed_base=BASE)
        take(0, rows[0], 'reset')
        ri = 1  # next row of the oracle run
        truncated = int(n_all.max()) > cap
        for t0 in range(0, steps, K):
            if stagger is not None and t0 == stagger:
                mask = torch.tensor([i % 2 for i in range(B)], dtype=torch.uint8, device=eng.device)
                g.refill()
                eng.reset(obs=first, mask=mask)
                take(0, rows[ri], f'masked reset before t{t0}')
                ri += 1
            if refresh_at is not None and t0 == refresh_at:
                w2, b2 = _weights(torch, E, kdim, 2)
                if bias == 'null':
                    po.wt.copy_(w2.t())
                else:
                    po.set_projection(w2, b2 if bias == 'random' else None)
                wt64, b64 = ref_w()
            g.refill()
            eng.step(K, actions=None, philox_seed=PSEED, step_base=t0, obs=po, auto_reset=True)
            for k in range(K):
                take(k, rows[ri], f't{t0 + k}')
                ri += 1
            if entries and count and not emb_only_count:
                over = bool(PC.counts(rows[ri - K:ri]).max() > cap)
                if over:
                    with pytest.raises(RuntimeError, match='nonzero entries > cap'):
                        po.check()
                else:
                    po.check()
        assert ri == len(rows)
        if c['done']:
            assert done.any(), 'no episode end' + (' with the reset overlap on' if lay['reset_overlap'] else '')
        # the same state rendered twice: identical bits, and still the oracle's last rows
        none = torch.zeros(B, dtype=torch.uint8, device=eng.device)
        twice = []
        for _ in range(2):
            g.refill()
            eng.reset(obs=first, mask=none)
            twice.append(g.rows(0, f'{what} re-render'))
        for f in twice[0]:
            assert twice[0][f].tobytes() == twice[1][f].tobytes(), f'{what}: {f} differs between two renders'
        check_rows(spec, c['maxpts'], rows[-1], twice[0], cap, wt64, b64, f'{what} re-render')
        g.check_guards(what)
        if pk == 2:
            _keep(what, dict(shape=PC.SHAPE_OF[c['maxpts']], obs_maxpts=lay['obs_maxpts'], obs_waves=lay['obs_waves'],
                                    reset_overlap=lay['reset_overlap'], largest_row=int(n_all.max()),
                                    truncated=truncated, episode_ends=int(done.sum()), err_over_bound=worst))
        return out
    finally:
        eng.close()


def _same(a, b, fields, what):
    assert len(a) == len(b)
    for t, (x, y) in enumerate(zip(a, b)):
        for f in fields:
            assert x[f].tobytes() == y[f].tobytes(), f'{what}: {f} of render {t} differs'


# ---- 1. shapes x modes -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('pk', [1, 2], ids=['entries', 'proj'])
@pytest.mark.parametrize('cfg', list(CASES))
def test_shape_and_mode(cfg, pk):
    """Every placement shape (and every MAXPTS the cases reach) entries-only and with the fused projection, the cap
    above the largest row."""
    render_run(cfg, pk=pk)


@pytest.mark.parametrize('pk', [1, 2], ids=['entries', 'proj'])
@pytest.mark.parametrize('cfg', ['packed_r3.yaml', 'packed_r4.yaml', 'packed_full.yaml', 'packed_lr81.yaml'])
def test_shape_and_mode_two_fused_steps(cfg, pk):
    """K = 2 on one config per shape: the second fused step's rows stand B*A rows further in every array."""
    render_run(cfg, pk=pk, K=2)


# ---- 2. render waves ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cfg,multi', [('packed_r4.yaml', 2), ('packed_r5.yaml', 4), ('packed_full.yaml', 4),
                                       ('packed_full.yaml', 8)])
def test_single_and_multi_wave_render_agree(cfg, multi):
    """The flattened and the multi-block shape forced to one render wave per env (k_obs) and to several (k_obs_mw, the
    waves split the agents): both meet the criteria and their idx, val and count are bit-equal."""
    one = render_run(cfg, waves=1)
    many = render_run(cfg, waves=multi)
    _same(one, many, ('idx', 'val', 'count'), f'{cfg}: 1 wave vs {multi}')


def test_obs_waves_that_cannot_be_honoured():
    """More than one wave needs rays of at least 10 points and is not a thing of the long-ray render; other values than
    1, 2, 4, 8 are refused."""
    if not gpu_available():
        pytest.skip('no GPU')
    from mfg_amd.engine import Engine
    from mfg_amd.spec import compile_spec
    for cfg, w, msg in (('packed_r3.yaml', 2, 'obs_waves > 1 needs'), ('packed_lr81.yaml', 2, 'obs_waves > 1 needs'),
                        ('packed_r4.yaml', 3, 'must be 0, 1, 2, 4 or 8'),
                        ('packed_r4.yaml', 16, 'must be 0, 1, 2, 4 or 8')):
        with pytest.raises(RuntimeError, match=msg):
            Engine(compile_spec(cfg), 2, variant={'obs_waves': w})


# ---- 3. cap against the flush ------------------------------------------------------------------------------------
@pytest.mark.parametrize('cfg,cap', [('packed_r3.yaml', c) for c in (1, 63, 64, 65, 100, 128)] +
                         [('packed_lr81.yaml', c) for c in (64, 100)])
def test_cap_against_the_flush(cfg, cap):
    """Rows up to 181 (170) entries stored into cap slots: truncated rows keep exactly their first cap entries, shorter
    rows are zero-filled up to cap, the next agent's row and the guards are intact, count is the true count, emb covers
    all entries and PackedObs.check() raises exactly at the steps where a count exceeds cap (render_run)."""
    render_run(cfg, cap=cap)


# ---- 4. projection width -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('E', [1, 63, 64, 65, 128])
@pytest.mark.parametrize('cfg', ['packed_r3.yaml', 'packed_r4.yaml'])
def test_projection_width(cfg, E):
    """One and two accumulator registers per lane, full and partial; the weights are replaced (set_projection) before
    step 10 and the next render uses the new ones."""
    render_run(cfg, E=E, refresh_at=10)


@pytest.mark.parametrize('cfg', ['packed_r3.yaml', 'packed_r4.yaml'])
def test_null_bias_is_a_zero_bias(cfg):
    """bias = NULL in the descriptor against a zero bias buffer: the criteria with a zero bias, and equal bits."""
    null = render_run(cfg, E=65, bias='null', refresh_at=10)
    _same(null, render_run(cfg, E=65, bias='zero', refresh_at=10), ('idx', 'val', 'count', 'emb'), f'{cfg}: NULL vs zero bias')
    c = CASES[cfg]
    spec, rows, _ = PC.oracle_run(cfg, c['B'], c['steps'])
    assert PC.counts(rows).min() == 0, 'an empty row: its emb is the bias alone'
    assert all((g['emb'][PC.counts(r) == 0] == 0).all() for g, r in zip(null, rows)), 'emb of an empty row is +0.0'


# ---- 5. optional outputs -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('cfg', ['packed_r3.yaml', 'packed_r4.yaml', 'packed_full.yaml', 'packed_lr81.yaml'])
def test_optional_outputs(cfg):
    """entries=False (emb and count), count=False (entries and emb) and a descriptor with count alone: the arrays that
    are present meet the criteria and are bit-equal to those of the full descriptor."""
    full = render_run(cfg, E=65)
    _same(full, render_run(cfg, E=65, entries=False), ('count', 'emb'), f'{cfg}: entries=False')
    _same(full, render_run(cfg, E=65, count=False), ('idx', 'val', 'emb'), f'{cfg}: count=False')
    _same(full, render_run(cfg, pk=1, emb_only_count=True), ('count',), f'{cfg}: count alone')
    _same(full, render_run(cfg, pk=1), ('idx', 'val', 'count'), f'{cfg}: entries-only render')


# ---- 6. masked reset ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cfg', ['packed_r3.yaml', 'packed_full.yaml'])
def test_masked_reset_then_packed_rows(cfg):
    """Before step 5 the odd envs are reset with a mask and packed obs; every env's row matches its oracle env then and
    at every later step (the episodes of odd and even envs now end at different steps)."""
    render_run(cfg, stagger=PC.STAGGER_AT)


# ---- 7. refusals -------------------------------------------------------------------------------------------------
def test_descriptor_refusals_launch_nothing():
    """check_packed's refusals: an error with its message, no output written, and the engine renders a valid descriptor
    correctly afterwards."""
    if not gpu_available():
        pytest.skip('no GPU')
    import torch
    from mfg_amd.engine import Engine, PackedObs
    cfg = 'packed_r3.yaml'
    c = CASES[cfg]
    spec, rows, _ = PC.oracle_run(cfg, c['B'], c['steps'])
    eng = Engine(spec, c['B'])
    try:
        kdim, cap = rows.shape[-1], 200
        w, b = _weights(torch, 64, kdim, 1)
        po = PackedObs(eng, K=1, cap=cap, weight=w, bias=b)
        g = Guarded(torch, po)
        eng.reset(obs=None, init=True, seed_base=BASE)
        none = torch.zeros(c['B'], dtype=torch.uint8, device=eng.device)
        good = {f: getattr(po.desc, f) for f in ('cap', 'emb_dim', 'idx', 'val', 'count', 'wt', 'bias', 'emb')}
        for change, msg in ((dict(val=None), 'idx and val must both be set or both NULL'),
                            (dict(idx=None), 'idx and val must both be set or both NULL'),
                            (dict(cap=0), 'cap must be > 0'), (dict(cap=-3), 'cap must be > 0'),
                            (dict(wt=None), 'emb needs wt'), (dict(emb_dim=0), 'emb needs wt'),
                            (dict(emb_dim=129), 'emb needs wt')):
            for f, v in {**good, **change}.items():
                setattr(po.desc, f, v)
            g.refill()
            with pytest.raises(RuntimeError, match=msg):
                eng.reset(obs=po, mask=none)
            with pytest.raises(RuntimeError, match=msg):
                eng.step(1, philox_seed=PSEED, step_base=0, obs=po)
            torch.cuda.synchronize()
            g.rows(0, f'refused {change}', untouched=True)
        for f, v in good.items():
            setattr(po.desc, f, v)
        eng.reset(obs=po, mask=none)
        check_rows(spec, c['maxpts'], rows[0], g.rows(0, 'after the refusals'), cap, po.wt.double().cpu().numpy(),
                   po.bias.double().cpu().numpy(), 'after the refusals')
        g.check_guards('refusals')
    finally:
        eng.close()


def test_row_too_wide_for_u16_is_refused():
    """grid128_full: the row is 114,688 wide, so packed obs are refused; the engine renders dense obs afterwards."""
    if not gpu_available():
        pytest.skip('no GPU')
    import torch
    import oracle as O
    from mfg_amd.engine import Engine, PackedObs
    from mfg_amd.spec import compile_spec
    spec = compile_spec('grid128_full.yaml')
    eng = Engine(spec, 1)
    try:
        assert eng.layout['obs_agent_stride'] == 114688
        po = PackedObs(eng, K=1, cap=8)
        g = Guarded(torch, po)
        with pytest.raises(RuntimeError, match='does not fit the u16 idx'):
            eng.reset(obs=po, init=True, seed_base=BASE)
        torch.cuda.synchronize()
        g.rows(0, 'refused', untouched=True)
        obs = torch.zeros(eng.obs_shape(), dtype=torch.float64, device=eng.device)
        eng.reset(obs=obs, init=True, seed_base=BASE)
        env = O.OracleEnv(spec, BASE)
        ref, o = env.reset(), obs.cpu().numpy()
        env.close()
        for a in range(spec.n_agents):
            assert (o[0, a, :spec.n_layers[a]] == ref[a]).all()
    finally:
        eng.close()
