"""The learner-side kernels of include/mfg_learn.h, each called through learn_lib.lib() at the shapes where its code
takes another path: the edge shapes, strides and NULL arguments of the five A2C-era kernels (csrc/mfg_learn.hip), the
grid-stride and finishing loops of the loss heads (mfg_ppo.hip, mfg_seac.hip) with their limits, the second GRU pass of
mfg_policy_act and a second block of mfg_eval_fold (mfg_act.hip), and the heads' contract on infinite logits.

Criteria (the project's own):
  * a kernel that computes: its largest error against the f64 reference (tests/learn_ref.py, or the tensor code in f64)
    is at most 4 times the error of the same formulas in f32 torch on the device against that reference, plus 1e-7
    (tests/test_gpu_mappo.py, tests/test_gpu_eval.py);
  * a kernel that only moves values: bit equality;
  * the projections: |out - ref| <= (cap + 2) 2^-24 S, S = |bias| + sum |v| |w| of the row (tests/test_gpu_seac.py);
  * every output sits between guard words and has pad columns, all of which keep their sentinel;
  * a second call gives identical bits.
Every comparing test prints its kernel error, the f32 torch error and their ratio; with MFG_LEARN_FIGURES set to a file
name they are written there as JSON (profiles/learn_kernels.json is one such run on an MI355X).
"""
import json
import os
from pathlib import Path

import pytest
import torch

import learn_ref as R
import mfg_amd.evaluate as EV
import test_gpu_eval as TE
import test_gpu_mappo as TM
import test_gpu_seac as TS
from mfg_amd import learn_lib

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -24
FILL = -7.0
GUARD = 32
FIGURES = {}
INF, NAN = float('inf'), float('nan')


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _keep(key, fig):
    FIGURES[key] = fig
    dst = os.environ.get('MFG_LEARN_FIGURES')
    if dst:
        Path(dst).write_text(json.dumps(FIGURES, indent=1))


def _record(key, e_ker, e_f32):
    """Print and keep one comparison: the kernel's and the f32 tensor code's largest errors against f64, per output."""
    ratio = [a / b if b else (float('inf') if a else 0.0) for a, b in zip(e_ker, e_f32)]
    print(f'{key}: kernel err = {e_ker}, f32 torch err = {e_f32}, ratio = {ratio}')
    _keep(key, dict(kernel_err=e_ker, torch_f32_err=e_f32, ratio=ratio))


def _four_times(key, e_ker, e_f32):
    _record(key, e_ker, e_f32)
    for k, f in zip(e_ker, e_f32):
        assert k <= 4 * f + 1e-7, (key, e_ker, e_f32)


def _errs(got, ref):
    return [float((a.double().cpu() - b.double().cpu()).abs().max()) for a, b in zip(got, ref)]


class Out:
    """An output of `rows` rows of `width` values held with `pad` more columns per row and GUARD words on either side,
    all at a sentinel the kernels do not produce."""

    def __init__(self, rows, width, pad=0, fill=FILL, dtype=torch.float32):
        self.fill, self.width, self.row = fill, width, width + pad
        self.buf = torch.full((rows * self.row + 2 * GUARD,), fill, dtype=dtype, device='cuda')
        self.mat = self.buf[GUARD:GUARD + rows * self.row].view(rows, self.row)

    def ptr(self):
        return self.mat.data_ptr()

    def data(self):
        return self.mat[:, :self.width].clone()

    def intact(self):
        f = self.fill
        return (bool((self.buf[:GUARD] == f).all()) and bool((self.buf[-GUARD:] == f).all())
                and bool((self.mat[:, self.width:] == f).all()))

    def untouched(self):
        return bool((self.buf == self.fill).all())


def _window(v, t=3, step=1, junk=1e30):
    """v [n, w] as step `step` of an [n, t, w] buffer whose other steps hold junk: (the view, its row stride)."""
    n, w = v.shape
    buf = torch.full((n, t, w), junk, dtype=v.dtype, device='cuda')
    buf[:, step] = v.cuda()
    return buf[:, step], t * w


def _padded(v, pad, junk=1e30):
    """v [n, w] with `pad` junk columns per row: (the view, its row stride)."""
    n, w = v.shape
    buf = torch.full((n, w + pad), junk, dtype=v.dtype, device='cuda')
    buf[:, :w] = v.cuda()
    return buf[:, :w], w + pad


# ---------------------------------------------------------------------------------------------------------------------
# 1, 2: the GRU step
# ---------------------------------------------------------------------------------------------------------------------
GRU_SHAPES = [(1, 1), (3, 5), (7, 37), (300, 16), (5, 128), (2, 129)]


def _gru_fwd_call(x, n, hd, bh, rpg=None, null_h=False):
    """mfg_gru_fwd_step (rpg None) or mfg_gru_fwd_step_grouped on windowed / padded views: (rc, the six Outs)."""
    gi, gi_row = _window(x['gi'])
    keep, keep_row = _window(x['keep'][:, None])
    h, h_row = _padded(x['h'], 1)
    gh0, bhd = x['gh0'].cuda().contiguous(), bh.cuda().contiguous()
    outs = [Out(max(n, 1), max(hd, 1), 2)] + [Out(max(n, 1), max(hd, 1), 3) for _ in range(5)]
    L = learn_lib.lib()
    head = (gi.data_ptr(), gi_row, gh0.data_ptr(), bhd.data_ptr())
    tail = (None if null_h else h.data_ptr(), h_row, keep.data_ptr(), keep_row, outs[0].ptr(), outs[0].row,
            *[o.ptr() for o in outs[1:]], outs[1].row, n, hd, _stream())
    rc = L.mfg_gru_fwd_step(*head, *tail) if rpg is None else L.mfg_gru_fwd_step_grouped(*head, rpg, *tail)
    torch.cuda.synchronize()
    return rc, outs


def _gru_fwd_check(key, x, n, hd, bh, rpg, null_h):
    rc, outs = _gru_fwd_call(x, n, hd, bh, rpg, null_h)
    assert rc == 0 and all(o.intact() for o in outs), key
    got = [o.data() for o in outs]
    args = lambda dt, dev: (x['gi'].to(dev, dt), x['gh0'].to(dev, dt), bh.to(dev, dt),  # noqa: E731
                            None if null_h else x['h'].to(dev, dt), x['keep'].to(dev, dt))
    ref = R.gru_fwd(*args(torch.float64, 'cpu'))
    f32 = R.gru_fwd(*args(torch.float32, 'cuda'))
    _four_times(key, _errs(got, ref), _errs(f32, ref))
    if null_h:
        assert bool((got[1] == 0).all())
    rc, again = _gru_fwd_call(x, n, hd, bh, rpg, null_h)
    assert rc == 0 and all(torch.equal(a, o.data()) for a, o in zip(got, again)), key
    return got


@pytest.mark.parametrize('n,hd', GRU_SHAPES)
def test_gru_fwd_step(n, hd):
    """All six outputs against the header's formulas in f64, on windowed inputs and padded outputs; h NULL; the grouped
    call bit-equal with one group and against f64 with a bias per row."""
    x = R.gru_inputs(n, hd)
    if n > 1:
        assert set(x['keep'].tolist()) == {0.0, 1.0}
    sat = R.gru_fwd(x['gi'], x['gh0'], x['bh'], x['h'], x['keep'])  # f32: the saturated rows reach the gates' ends
    if n * hd >= 15:
        assert bool((sat[2] == 0).any() or (sat[2] == 1).any()) and bool((sat[3] == 0).any() or (sat[3] == 1).any())
        assert bool((1 - sat[4] * sat[4] == 0).any())
    got = _gru_fwd_check(f'gru_fwd.n{n}.hd{hd}', x, n, hd, x['bh'], None, False)
    _gru_fwd_check(f'gru_fwd.n{n}.hd{hd}.h_null', x, n, hd, x['bh'], None, True)
    rc, one = _gru_fwd_call(x, n, hd, x['bh'], rpg=n)
    assert rc == 0 and all(o.intact() and torch.equal(o.data(), a) for o, a in zip(one, got))
    _gru_fwd_check(f'gru_fwd_grouped.n{n}.hd{hd}.bias_per_row', x, n, hd, x['bh_rows'], 1, False)
    _gru_fwd_check(f'gru_fwd_grouped.n{n}.hd{hd}.bias_per_row.h_null', x, n, hd, x['bh_rows'], 1, True)


def test_gru_fwd_step_refuses_bad_sizes():
    x = R.gru_inputs(6, 5)
    for n, hd, rpg in ((0, 5, None), (6, 0, None), (0, 5, 1), (6, 0, 1), (6, 5, 4), (6, 5, 0)):
        rc, outs = _gru_fwd_call(x, n, hd, x['bh_rows'], rpg)
        assert rc == -1 and all(o.untouched() for o in outs), (n, hd, rpg)


def _gru_bwd_call(x, saved, n, hd, with_dout, with_dhp):
    dout, do_row = _window(x['dout'])
    keep_nx, keep_row = _window(x['keep_next'][:, None])
    dhp = x['dhp_next'].cuda().contiguous()
    sv = [_padded(s, 3) for s in saved]  # r, z, n, ghn, hp
    dgi, dgh, dhz = Out(n, 3 * hd, 1), Out(n, 3 * hd, 2), Out(n, hd, 0)
    rc = learn_lib.lib().mfg_gru_bwd_step(dout.data_ptr() if with_dout else None, do_row,
                                          dhp.data_ptr() if with_dhp else None,
                                          keep_nx.data_ptr() if with_dhp else None, keep_row,
                                          *[s[0].data_ptr() for s in sv], sv[0][1], dgi.ptr(), dgi.row, dgh.ptr(),
                                          dgh.row, dhz.ptr(), n, hd, _stream())
    torch.cuda.synchronize()
    return rc, (dgi, dgh, dhz)


@pytest.mark.parametrize('n,hd', GRU_SHAPES)
def test_gru_bwd_step(n, hd):
    """dgi, dgh against autograd in f64 of the forward formulas, dhz = dh z, with the saved activations of the f64
    forward rounded to f32; dout and dhp_next present or NULL in all four combinations."""
    x = R.gru_inputs(n, hd)
    d = {k: v.double() for k, v in x.items()}
    gh = d['gh0'] * d['keep'][:, None] + d['bh']
    _, hp, r, z, nn, ghn = R.gru_fwd(d['gi'], d['gh0'], d['bh'], d['h'], d['keep'])
    saved = [v.float() for v in (r, z, nn, ghn, hp)]
    for with_dout in (True, False):
        for with_dhp in (True, False):
            key = f'gru_bwd.n{n}.hd{hd}.dout{int(with_dout)}.dhp{int(with_dhp)}'
            rc, outs = _gru_bwd_call(x, saved, n, hd, with_dout, with_dhp)
            assert rc == 0 and all(o.intact() for o in outs), key
            got = [o.data() for o in outs]
            if not with_dout and not with_dhp:
                assert all(bool((g == 0).all()) for g in got), key
                continue

            def dh_of(dt, dev):
                dh = torch.zeros((n, hd), dtype=dt, device=dev)
                if with_dhp:
                    dh = x['dhp_next'].to(dev, dt) * x['keep_next'].to(dev, dt)[:, None]
                if with_dout:
                    dh = x['dout'].to(dev, dt) + dh
                return dh
            ref = R.gru_bwd(d['gi'], gh, hp, dh_of(torch.float64, 'cpu'))
            f32 = R.gru_bwd_formulas(dh_of(torch.float32, 'cuda'), *[s.cuda() for s in saved])
            _four_times(key, _errs(got, ref), _errs(f32, ref))
            rc, again = _gru_bwd_call(x, saved, n, hd, with_dout, with_dhp)
            assert rc == 0 and all(torch.equal(a, o.data()) for a, o in zip(got, again)), key


# ---------------------------------------------------------------------------------------------------------------------
# 3: packed rows to dense
# ---------------------------------------------------------------------------------------------------------------------
def _scatter_rows(m, cap, k, g):
    """Packed rows with distinct indices per row: about a quarter of the values are zero (at nonzero indices, between
    nonzero entries) and about a sixth of the entries carry an index >= k with a nonzero value (ignored)."""
    idx = torch.rand((m, k), generator=g).argsort(-1)[:, :cap]
    val = torch.randn((m, cap), generator=g)
    val = torch.where(val == 0, torch.ones_like(val), val)
    if m > 1:
        val[torch.rand((m, cap), generator=g) < 0.25] = 0.0
        over = torch.rand((m, cap), generator=g) < 0.16
        idx = torch.where(over, torch.randint(k, 65536, (m, cap), generator=g), idx)
    return idx, val


@pytest.mark.parametrize('m,cap,k', [(1, 1, 1), (5, 16, 4096), (9, 130, 300), (32773, 3, 7)])
def test_packed_densify_is_scatter(m, cap, k):
    """Bit-exact against a scatter of the entries with a nonzero value and an index < k. k = 4096: the dynamic LDS is
    exactly 64 KiB; cap = 130: three entry chunks; m = 32,773: 8,192 blocks and a second stride pass of 5 rows."""
    g = torch.Generator().manual_seed(m + cap + k)
    idx, val = _scatter_rows(m, cap, k, g)
    live = (val != 0) & (idx < k)
    if m > 1:
        assert bool((idx >= k).any()) and bool(((val == 0) & (idx < k) & (idx > 0)).any())
    ref = torch.zeros((m, k))
    rows = torch.arange(m)[:, None].expand(m, cap)
    ref[rows[live], idx[live]] = val[live]
    iu, vc = idx.to(torch.uint16).cuda(), val.cuda()
    L = learn_lib.lib()
    outs = []
    for _ in range(2):
        out = Out(m, k, 3)
        assert L.mfg_packed_densify(iu.data_ptr(), vc.data_ptr(), m, cap, k, out.ptr(), out.row, _stream()) == 0
        torch.cuda.synchronize()
        assert out.intact()
        assert torch.equal(out.data().cpu(), ref)
        outs.append(out.data())
    assert torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32))


def test_packed_densify_refuses_bad_sizes():
    L = learn_lib.lib()
    iu = torch.zeros((2, 4), dtype=torch.uint16, device='cuda')
    vc = torch.ones((2, 4), device='cuda')
    out = Out(2, 4097, 3)
    assert L.mfg_packed_densify(iu.data_ptr(), vc.data_ptr(), 2, 4, 4097, out.ptr(), out.row, _stream()) == -1
    assert L.mfg_packed_densify(iu.data_ptr(), vc.data_ptr(), 2, 4, 16, out.ptr(), 15, _stream()) == -1
    torch.cuda.synchronize()
    assert out.untouched()


# ---------------------------------------------------------------------------------------------------------------------
# 4: the packed-row projection
# ---------------------------------------------------------------------------------------------------------------------
def _compacted_rows(cap, k, g):
    """Front-compacted rows as the engine writes them (include/mfg.h: a row's nonzero entries first, zeros after), two
    of every entry count in {0, 1, 63, 64, 65, 127, 128} that fits cap; about a sixth of the entries carry an index
    >= k (a nonzero value, ignored)."""
    counts = [c for c in (0, 1, 63, 64, 65, 127, 128) if c <= cap] * 2
    m = len(counts)
    cnt = torch.tensor(counts)
    idx = torch.rand((m, k), generator=g).argsort(-1)[:, :cap]
    over = torch.rand((m, cap), generator=g) < 0.16
    idx = torch.where(over, torch.randint(k, 65536, (m, cap), generator=g), idx)
    val = torch.randn((m, cap), generator=g)
    val = torch.where(val.abs() < 0.05, torch.ones_like(val), val)
    live = torch.arange(cap)[None] < cnt[:, None]
    return idx * live, val * live, cnt


@pytest.mark.parametrize('cap', [64, 70, 128])
@pytest.mark.parametrize('e_dim', [1, 64, 65, 130])
def test_packed_project(cap, e_dim):
    """Against a dense f64 matmul with the projections' derived bound; entry counts at the kernel's early-exit
    decisions (a chunk of exactly 64 nonzero entries goes on to the next, anything less stops); a row without entries
    is the bias exactly; bit-equal to mfg_packed_project_grouped with one network (the same products added in the same
    order) where that call takes the size (e_dim <= 128)."""
    k = 300
    g = torch.Generator().manual_seed(cap * 1000 + e_dim)
    idx, val, cnt = _compacted_rows(cap, k, g)
    m = idx.shape[0]
    assert bool(((idx >= k) & (val != 0)).any())
    wt, bias = torch.randn((k, e_dim), generator=g), torch.randn(e_dim, generator=g)
    live = (val != 0) & (idx < k)
    d = torch.zeros((m, k), dtype=torch.float64)
    rows = torch.arange(m)[:, None].expand(m, cap)
    d[rows[live], idx[live]] = val[live].double()
    ref = d @ wt.double() + bias.double()
    mag = d.abs() @ wt.double().abs() + bias.double().abs()
    iu, vc, cw, cb = idx.to(torch.uint16).cuda(), val.cuda(), wt.cuda(), bias.cuda()
    L = learn_lib.lib()
    got = []
    for _ in range(2):
        out = Out(m, e_dim, 3)
        assert L.mfg_packed_project(iu.data_ptr(), vc.data_ptr(), m, cap, cw.data_ptr(), cb.data_ptr(), e_dim, k,
                                    out.ptr(), out.row, _stream()) == 0
        torch.cuda.synchronize()
        assert out.intact()
        got.append(out.data().cpu())
    assert torch.equal(got[0], got[1])
    err = (got[0].double() - ref).abs()
    bound = (cap + 2) * EPS * mag
    worst = float((err / bound).max())
    print(f'packed_project.cap{cap}.E{e_dim}: max err = {float(err.max())}, largest err / bound = {worst}')
    _keep(f'packed_project.cap{cap}.E{e_dim}', dict(max_err=float(err.max()), err_over_bound=worst))
    assert bool((err <= bound + 1e-30).all()), (cap, e_dim, float(err.max()))
    assert torch.equal(got[0][cnt == 0], bias[None].expand(int((cnt == 0).sum()), e_dim))
    if e_dim <= 128:
        grp = Out(m, e_dim, 3)
        assert L.mfg_packed_project_grouped(iu.data_ptr(), vc.data_ptr(), m, cap, 1, cw.data_ptr(), cb.data_ptr(),
                                            e_dim, k, 0, grp.ptr(), grp.row, _stream()) == 0
        torch.cuda.synchronize()
        assert grp.intact() and torch.equal(grp.data().cpu(), got[0])


# ---------------------------------------------------------------------------------------------------------------------
# 5: categorical sampling
# ---------------------------------------------------------------------------------------------------------------------
def _sample(logits, n_act, u):
    n = logits.shape[0]
    lg, ud = logits.cuda().contiguous(), u.cuda().contiguous()
    out = Out(n, 1, 0, fill=-77, dtype=torch.int32)
    rc = learn_lib.lib().mfg_sample_categorical(lg.data_ptr(), logits.shape[1], n_act, ud.data_ptr(), n, out.ptr(),
                                                _stream())
    torch.cuda.synchronize()
    assert rc == 0 and out.intact()
    return out.data().flatten().cpu().long()


@pytest.mark.parametrize('n_act', [1, 2, 7, 32])
@pytest.mark.parametrize('n', [20000, 1])
def test_sample_categorical_per_row(n, n_act):
    """Every row's pick against the inversion of the f64 CDF at the same u. A row is left out only where u lies within
    1e-5 of a CDF step (f32 rounding may pick either neighbour there), and at most 1% of the rows may be."""
    logits, u = R.sampler_inputs(n, n_act)
    pick, near = R.cdf_pick(logits[:, :n_act], u)
    share = float(near.double().mean())
    got = _sample(logits, n_act, u)
    wrong = int((got[~near] != pick[~near]).sum())
    print(f'sample_categorical.n{n}.act{n_act}: left out {100 * share:.3f}% of the rows, {wrong} of the rest differ')
    _keep(f'sample_categorical.n{n}.act{n_act}', dict(left_out_share=share, differ=wrong))
    assert share <= 0.01
    assert wrong == 0
    assert int(got.min()) >= 0 and int(got.max()) < n_act  # the +1000 pad columns are never picked
    assert torch.equal(got, _sample(logits, n_act, u))


def test_sample_categorical_edges_of_the_range():
    """An action of probability 0 in f32 (120 below the rest, or -inf) at either end is never picked, at u = 0 for the
    first and at u = 1 - 2^-24 for the last; rows without a distribution (all -inf, any +inf, any NaN) give -1."""
    g = torch.Generator().manual_seed(11)
    n, n_act = 4096, 7
    for low in (-120.0, -INF):
        lg = torch.randn((n, n_act), generator=g) * 3
        lg[n // 2:] += 80.0
        first, last = lg.clone(), lg.clone()
        first[:, 0] = lg[:, 1:].max(-1).values + low
        last[:, -1] = lg[:, :-1].max(-1).values + low
        assert bool((_sample(first, n_act, torch.zeros(n)) >= 1).all())
        assert bool((_sample(last, n_act, torch.full((n,), R.U_LAST)) <= n_act - 2).all())
    # -inf in the middle: per row against the f64 CDF, and never picked
    lg = torch.randn((n, n_act), generator=g) * 3
    lg[:, 3] = -INF
    u = torch.rand(n, generator=g)
    u[0], u[1], u[2] = 0.0, R.U_LAST, 2.0 ** -30
    pick, near = R.cdf_pick(lg, u)
    got = _sample(lg, n_act, u)
    assert bool((got != 3).all()) and torch.equal(got[~near], pick[~near]) and float(near.double().mean()) <= 0.01
    bad = torch.randn((4, n_act), generator=g)
    bad[0, :] = -INF
    bad[1, 2] = INF
    bad[2, 5] = NAN
    assert _sample(bad, n_act, torch.full((4,), 0.5))[:3].tolist() == [-1, -1, -1]
    assert _sample(bad, n_act, torch.full((4,), 0.5))[3] >= 0


# ---------------------------------------------------------------------------------------------------------------------
# 6: the loops of mfg_mc_returns and mfg_ppo_head
# ---------------------------------------------------------------------------------------------------------------------
LOOP_SHAPES = [(262401, 2), (70000, 1)]  # 1024 blocks, four finish passes, a second stride pass of 257 rows; 274 blocks


@pytest.mark.parametrize('n,t', LOOP_SHAPES)
def test_mc_returns_loops(n, t):
    TM.test_mc_returns_kernel(n, t, 'mixed')


@pytest.mark.parametrize('n,t', LOOP_SHAPES)
def test_ppo_head_loops(n, t):
    x = TM.head_inputs(n, t, 3)
    e_ker, e_f32, ref, ker = TM.head_errors(x)
    _record(f'ppo_head.n{n}.t{t}.act3', e_ker, e_f32)
    assert e_ker[0] <= 4 * e_f32[0], (e_ker[0], e_f32[0])
    assert e_ker[1] <= 4 * e_f32[1] + 1e-7, (e_ker[1], e_f32[1])
    assert e_ker[2] <= 4 * e_f32[2] + 1e-7, (e_ker[2], e_f32[2])
    rc, *again = TM.kernel_head(x)
    assert rc == 0 and all(torch.equal(a, b) for a, b in zip(ker, again))


# ---------------------------------------------------------------------------------------------------------------------
# 7: the heads on infinite logits
# ---------------------------------------------------------------------------------------------------------------------
def _spare_column(row, a):
    """A column of the row that is neither the action nor the row's maximum."""
    return next(c for c in range(row.numel()) if c != a and c != int(row.argmax()))


@pytest.mark.parametrize('bad', [-INF, INF, NAN])
@pytest.mark.parametrize('where', ['spare', 'action', 'old'])
def test_ppo_head_non_finite_logit(bad, where):
    """One element with a non-finite logit: its gradients are exactly 0, the loss is NaN, every other gradient is
    finite, the guards are intact (kernel_head asserts them)."""
    x = TM.head_inputs(3, 5, 10)
    e = 7
    a = int(x['act'][e])
    col = a if where == 'action' else _spare_column(x['logits'][e], a)
    if where == 'old':
        x = dict(x, old=x['old'].clone())
        x['old'][e, col] = bad
        rc, loss, dl, dc = TM.kernel_head(x)
    else:
        logits = x['logits'].clone()
        logits[e, col] = bad
        rc, loss, dl, dc = TM.kernel_head(x, logits=logits)
    assert rc == 0 and bool(torch.isnan(loss))
    assert bool((dl[e] == 0).all()) and float(dc[e]) == 0
    assert bool(torch.isfinite(dl).all()) and bool(torch.isfinite(dc).all())


@pytest.mark.parametrize('bad', [-INF, INF, NAN])
@pytest.mark.parametrize('where', ['spare', 'action'])
@pytest.mark.parametrize('cross', [1, 0])
def test_seac_head_non_finite_logit(cross, where, bad):
    """Row 2 (agent 0, env 2), step 1. cross: network 2's logit spoils loss 2 only (an off-policy element, no entropy
    term); the row's own network's logit spoils every loss through the importance weight. own: loss 0 only."""
    A, B, t = 3, 4, 5
    x = TS.head_inputs(A, B, t, 10, cross, 'none')
    row, s = 2, 1
    a = int(x['act'][s, 2, 0])
    for net in ((2, 0) if cross else (0,)):
        col = a if where == 'action' else _spare_column(x['logits'][net, row, s], a)
        logits = x['logits'].clone()
        logits[net, row, s, col] = bad
        rc, loss, dl, dc = TS.kernel_head(x, 0.0, logits=logits)
        assert rc == 0
        want = [True] * A if (cross and net == 0) else [j == net for j in range(A)]
        assert torch.isnan(loss).tolist() == want, (net, loss)
        hit = slice(None) if (cross and net == 0) else net
        assert bool((dl[hit, row, s] == 0).all()) and bool((dc[hit, row, s] == 0).all())
        assert bool(torch.isfinite(dl).all()) and bool(torch.isfinite(dc).all())
        rc, loss, dl, dc = TS.kernel_head(x, 0.95, logits=logits)  # with a GAE scan through the element
        assert rc == 0 and torch.isnan(loss).tolist() == want
        assert bool((dl[hit, row, s] == 0).all()) and bool(torch.isfinite(dl).all()) and bool(torch.isfinite(dc).all())


# ---------------------------------------------------------------------------------------------------------------------
# 8: the limits of mfg_seac_head
# ---------------------------------------------------------------------------------------------------------------------
SEAC_LIMITS = [((2, 150, 255, 3), 1), ((2, 150, 255, 3), 0),  # one pair per block; 300 pairs: a second stride pass
               ((2, 5, 128, 3), 1), ((2, 5, 128, 3), 0),      # one pair per block and 127 idle threads
               ((3, 4, 84, 4), 1), ((3, 4, 84, 4), 0),        # three pairs per block and one idle thread
               ((2, 400, 5, 4), 1)]                           # 800 rows at 42 pairs per block


@pytest.mark.parametrize('shape,cross', SEAC_LIMITS)
@pytest.mark.parametrize('gae', [0.0, 0.95])
def test_seac_head_limits(shape, cross, gae):
    """test_gpu_seac.py's criteria at the sizes where the block holds one pair, idle threads exist, or the stride and
    finish loops take a second pass."""
    A, B, t, n_act = shape
    x = TS.head_inputs(A, B, t, n_act, cross, 'mixed')
    assert 0 < float(x['done'].sum()) < x['done'].numel()
    ref = TS.torch_head(x, torch.float64, 'cpu', gae)
    f32 = TS.torch_head(x, torch.float32, 'cuda', gae)
    rc, *ker = TS.kernel_head(x, gae)
    assert rc == 0
    e_ker, e_f32 = _errs(ker, ref), _errs(f32, ref)
    key = f'seac_head.A{A}_B{B}_t{t}_n{n_act}_cross{cross}_gae{gae}'
    _record(key, e_ker, e_f32)
    assert e_ker[0] <= 4 * e_f32[0] + TS._ulp(float(ref[0].abs().max())), (e_ker[0], e_f32[0])
    assert e_ker[1] <= 4 * e_f32[1] + 1e-7, (e_ker[1], e_f32[1])
    assert e_ker[2] <= 4 * e_f32[2] + 1e-7, (e_ker[2], e_f32[2])
    assert bool((ker[1][..., t, :] == 0).all()) and bool((ker[2][..., t] == 0).all())
    rc, *again = TS.kernel_head(x, gae)
    assert rc == 0 and all(torch.equal(a, b) for a, b in zip(ker, again))


@pytest.mark.parametrize('cross', [1, 0])
def test_seac_head_refuses_t_256(cross):
    x = TS.head_inputs(2, 2, 256, 3, cross, 'none')
    rc, loss, dl, dc = TS.kernel_head(x, 0.95)
    assert rc == -1
    assert bool((loss == -3.0).all()) and bool((dl == -3.0).all()) and bool((dc == -3.0).all())


# ---------------------------------------------------------------------------------------------------------------------
# 9: the second GRU pass of mfg_policy_act
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('sizes', [(40, 7, 100, 11), (128, 32, 65, 32), (128, 32, 128, 32)])
@pytest.mark.parametrize('g', [1, 3])
def test_policy_act_second_gru_pass(g, sizes):
    """H > 64: the GRU loop runs twice, with a block barrier inside. Logits and h' against f64 by the 4x rule at 32, 33
    and 64 rows per network, both layouts; guards intact; the rows of one env alone (another launch shape) give the
    same bits."""
    E, AE, H, n_max = sizes
    gen = torch.Generator().manual_seed(7 * g + H)
    n_act = TE.n_acts(n_max, g)
    w = TE.make_weights(g, E, AE, H, n_max, gen)
    shapes = [(32, 1), (11, 3), (64, 1)] if g == 1 else [(32, 3), (33, 3), (64, 3)]
    for B, A in shapes:
        emb, h, pa, pd, u = TE.make_inputs(B, A, E, H, n_act, gen)
        ref = TE.formulas(w, emb, h, pa, pd, torch.float64)
        f32 = TE.formulas(w, emb, h, pa, pd, torch.float32)
        for layout in ('engine', 'agent'):
            rc, lg, hn, act, ok = TE.run_kernel(w, emb, h, pa, pd, u, n_act, layout)
            assert rc == 0 and ok
            key = f'policy_act.g{g}.E{E}.AE{AE}.H{H}.n{n_max}.B{B}.A{A}.{layout}'
            _four_times(key, _errs((lg, hn), ref), _errs(f32, ref))
            assert int(act.min()) >= 0
            rc, lg2, hn2, act2, ok = TE.run_kernel(w, emb, h, pa, pd, u, n_act, layout)
            assert rc == 0 and ok and torch.equal(lg2, lg) and torch.equal(hn2, hn) and torch.equal(act2, act)
            b = 5
            rc, lg3, hn3, act3, ok = TE.run_kernel(w, emb[b:b + 1], h[b:b + 1], pa[b:b + 1], pd[b:b + 1], u[b:b + 1],
                                                   n_act, layout)
            assert rc == 0 and ok
            assert torch.equal(lg3[0], lg[b]) and torch.equal(hn3[0], hn[b]) and torch.equal(act3[0], act[b])


# ---------------------------------------------------------------------------------------------------------------------
# 10: the grouped projection at its largest cap, the fold over two blocks
# ---------------------------------------------------------------------------------------------------------------------
def test_grouped_projection_at_cap_2048():
    """cap = 2048: the compacted entries of a block's four rows fill exactly 64 KiB of LDS. Both modes against the dense
    f64 matmul with the derived bound; cap = 2049 is refused and nothing is written."""
    G, m, E, k, cap = 2, 8, 128, 4096, 2048
    g = torch.Generator().manual_seed(2048)
    idx, val = TS._packed_rows(m, cap, k, g)
    assert int((val[1] != 0).sum()) >= cap - 1  # row 1 is full
    wt, bias = torch.randn((G, k, E), generator=g), torch.randn((G, E), generator=g)
    d = torch.zeros((m, k), dtype=torch.float64).scatter_add_(1, idx, val.double())
    ref_all = torch.einsum('rk,gke->gre', d, wt.double()) + bias.double()[:, None]
    mag_all = torch.einsum('rk,gke->gre', d.abs(), wt.double().abs()) + bias.double().abs()[:, None]
    ci, cv, cw, cb = idx.to(torch.uint16).cuda(), val.cuda(), wt.cuda(), bias.cuda()
    L = learn_lib.lib()
    r = torch.arange(m)
    mb = m // G
    for all_ in (0, 1):
        rows = G * m if all_ else m
        runs = []
        for _ in range(2):
            out = Out(rows, E, 3)
            assert L.mfg_packed_project_grouped(ci.data_ptr(), cv.data_ptr(), m, cap, G, cw.data_ptr(), cb.data_ptr(),
                                                E, k, all_, out.ptr(), out.row, _stream()) == 0
            torch.cuda.synchronize()
            assert out.intact()
            runs.append(out.data().cpu())
        assert torch.equal(runs[0], runs[1])
        got = runs[0].double()
        if all_:
            got, ref, mag = got.view(G, G, mb, E)[:, r % G, r // G], ref_all, mag_all
        else:
            got, ref, mag = got.view(G, mb, E)[r % G, r // G], ref_all[r % G, r], mag_all[r % G, r]
        err = (got - ref).abs()
        bound = (cap + 2) * EPS * mag
        worst = float((err / bound).max())
        print(f'project_grouped.cap2048.all{all_}: max err = {float(err.max())}, largest err / bound = {worst}')
        _keep(f'project_grouped.cap2048.all{all_}', dict(max_err=float(err.max()), err_over_bound=worst))
        assert bool((err <= bound + 1e-30).all()), (all_, float(err.max()))
    out = Out(m, E, 3)
    big_i = torch.zeros((m, 2049), dtype=torch.uint16, device='cuda')
    big_v = torch.ones((m, 2049), device='cuda')
    assert L.mfg_packed_project_grouped(big_i.data_ptr(), big_v.data_ptr(), m, 2049, G, cw.data_ptr(), cb.data_ptr(), E,
                                        k, 0, out.ptr(), out.row, _stream()) == -1
    torch.cuda.synchronize()
    assert out.untouched()


def test_eval_fold_over_two_blocks():
    """B = 300 envs (two blocks of 256), A = 3, six steps against evaluate.eval_fold after every step; env 0 ends three
    episodes with n_episodes = 2 and writes no third row."""
    B, A, n_ep, steps = 300, 3, 2, 6
    gen = torch.Generator().manual_seed(300)
    rewards = torch.randn((steps, B, A), generator=gen, dtype=torch.float64) * 0.3
    dones = (torch.rand((steps, B), generator=gen) < 0.3).to(torch.uint8)
    dones[:, 0] = torch.tensor([1, 1, 0, 1, 0, 1])
    dones[:, B - 1] = torch.tensor([0, 1, 1, 1, 0, 0])
    dev = 'cuda'

    def state(device):
        return [torch.zeros((B, A), device=device), torch.zeros(B, dtype=torch.int32, device=device),
                torch.zeros(B, dtype=torch.int32, device=device)]
    eps, ln, cnt = state(dev)
    rows, lengths = Out(B * n_ep, A + 1, 0, fill=333.0), Out(B, n_ep, 0, fill=-5, dtype=torch.int32)
    rows.mat.zero_()
    lengths.mat.zero_()
    fin = torch.zeros((), dtype=torch.int32, device=dev)
    st = state('cpu') + [torch.zeros((B, n_ep, A + 1)), torch.zeros((B, n_ep), dtype=torch.int32),
                         torch.zeros((), dtype=torch.int32)]
    rw, dn = rewards.to(dev), dones.to(dev)
    L = learn_lib.lib()
    for t in range(steps):
        assert L.mfg_eval_fold(rw[t].data_ptr(), dn[t].data_ptr(), B, A, n_ep, eps.data_ptr(), ln.data_ptr(),
                               cnt.data_ptr(), rows.ptr(), lengths.ptr(), fin.data_ptr(), _stream()) == 0
        torch.cuda.synchronize()
        EV.eval_fold(rewards[t], dones[t], n_ep, *st)
        got = (eps, ln, cnt, rows.mat.view(B, n_ep, A + 1), lengths.mat, fin)
        assert all(torch.equal(a.cpu(), b) for a, b in zip(got, st)), t
        assert rows.intact() and lengths.intact()
    assert int(cnt[0]) == n_ep and int(cnt.max()) == n_ep and int(fin) == int((dones.sum(0) >= n_ep).sum())
    assert int(fin) > 0 and int((cnt < n_ep).sum()) > 0
