"""The call-level contract of include/mfg.h around the kernels: profiled stepping (mfg_profile / mfg_profile_read),
stepping on a non-default stream (the `stream` argument of every entry point) and mfg_hbm_copy.

The stepping tests run the comparison loop of tests/oracle_compare.py: every env and step against its own C-oracle env
(rewards with ==, done, event fields, f64 obs bit for bit) and after every call the records' RNG state and floor order.
"""
import ctypes
import time

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


def _ks(steps, stagger=None):
    """K per call, 1, 3, 1, 3 ... with a call boundary at the stagger step."""
    ks, t = [], 0
    for hi in ([stagger] if stagger else []) + [steps]:
        while t < hi:
            ks.append(min((1, 3)[len(ks) % 2], hi - t))
            t += ks[-1]
    return ks


def _compared_run(torch, eng, ob, steps, stagger=None, call=lambda fn: fn(), mask_at=None):
    """reset(init) and `steps` steps of `eng` against the oracle batch `ob`, the odd envs reset before step `stagger`.
    Every engine call goes through `call` (a function that runs it and returns its result); everything else here
    (buffers aside) is host work or a copy to the host on the current stream. mask_at: a step before which
    mfg_action_mask runs into a poisoned buffer, checked against a second run after a device synchronize."""
    spec, B = ob.spec, eng.B
    buf = OC.make_buffers(torch, eng, 3)
    odd = torch.as_tensor(ob.odd_mask(), device=eng.device)
    mask_out = torch.full((B, eng.A), -1, dtype=torch.int32, device=eng.device)
    torch.cuda.synchronize()
    call(lambda: eng.reset(obs=buf['obs'][0], init=True, seed_base=BASE))
    got, want = buf['obs'][0].cpu().numpy(), ob.reset()
    for j in range(B):
        OC.compare_obs(f'reset obs env {j}', spec, got[j], want[j])
    t = 0
    for c, K in enumerate(_ks(steps, stagger)):
        if t == stagger:
            call(lambda: eng.reset(obs=buf['obs'][0], mask=odd))
            got, want = buf['obs'][0].cpu().numpy(), ob.reset(odd_only=True)
            for j in range(B):
                OC.compare_obs(f'staggered reset obs env {j}', spec, got[j], want[j])
        if t == mask_at:
            call(lambda: eng.action_mask(mask_out))
            got = mask_out.cpu().numpy()
            assert (got != -1).all(), 'mfg_action_mask had not written its rows when its stream was done'
            torch.cuda.synchronize()
            assert np.array_equal(got, eng.action_mask().cpu().numpy())
        call(lambda: eng.step(K, actions=None, philox_seed=PSEED, env_base=0, step_base=t, auto_reset=True,
                              **{k: v[:K] for k, v in buf.items()}))
        OC.compare_call(f'call {c} (K = {K})', ob, OC.rows_of(buf, K), K)
        t += K
        OC.check_state(f'after call {c} (step {t})', call(eng.export_state).cpu().numpy(), eng.layout, ob)
    assert t == steps and (mask_at is None or mask_at < steps)


def _engine(cfg, B, variant=None):
    from mfg_amd.spec import compile_spec
    from mfg_amd.engine import Engine
    spec = compile_spec(cfg)
    return spec, Engine(spec, B, variant=variant)


# ---------------------------------------------------------------------------------------------------------------------
# profiled stepping
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cfg,B,steps,stagger', [('grid128_full_ep.yaml', 7, 30, 5), ('alltest16.yaml', 8, 24, None)])
def test_profiled_run_equals_the_oracle(cfg, B, steps, stagger):
    """Events around every launch, on both streams where the engine uses its second one (grid128_full_ep: the done-list
    render; alltest16: the per-step replay too), change no result."""
    torch = _need_gpu()
    spec, eng = _engine(cfg, B)
    assert eng.layout['reset_overlap'] == 1
    eng.profile(True)
    ob = OC.OracleBatch(spec, list(range(B)), BASE, PSEED)
    _compared_run(torch, eng, ob, steps, stagger)
    prof = eng.profile_read()
    assert prof['k_logic'][1] == steps and prof['k_obs_done'][1] == steps
    if stagger:
        assert ob.ended.min() >= 1  # 12-step episodes: every env went through the done list and its render
    eng.close()
    ob.close()


@pytest.mark.parametrize('cfg,variant,B,N,K,replays,sel', [
    ('large8.yaml', None, 8, 3, 4, 'N', None),
    ('alltest16.yaml', None, 8, 3, 4, 'NK', 0),
    ('alltest16.yaml', {'serial': 1}, 8, 3, 4, 'N', 'NK'),
    ('grid128_full_ep.yaml', {'render_slots': 2}, 7, 2, 3, None, None),
    ('eval_trio.yaml', None, 16, 2, 3, None, None)],
    ids=['large8', 'alltest16', 'alltest16-serial', 'grid128_full_ep', 'eval_trio'])
def test_profile_launch_counts(cfg, variant, B, N, K, replays, sel):
    """mfg_profile_read's launch counts are the launch structure include/mfg.h documents: per step one k_logic, one
    k_resetdone (auto-reset) and one k_obs (obs), one k_obs_done where the resets run beside the render; one k_replay
    per call (per step where the engine replays every step), k_replay_sel per step where RespawnDirt's debt is paid
    ahead of k_logic instead; one k_reset per mfg_reset and one k_action_mask per mfg_action_mask."""
    torch = _need_gpu()
    spec, eng = _engine(cfg, B, variant)
    buf = OC.make_buffers(torch, eng, K)
    want = {'N': N, 'NK': N * K, 0: 0}

    def step(k, **kw):
        eng.step(k, actions=None, philox_seed=PSEED, step_base=step.t, auto_reset=True,
                 **{n: v[:k] for n, v in buf.items()}, **kw)
        step.t += k
    step.t = 0

    eng.profile(True)
    eng.reset(init=True, seed_base=BASE)
    eng.reset(mask=torch.arange(B, device=eng.device).remainder(2).to(torch.uint8))
    eng.action_mask()
    eng.action_mask()
    for _ in range(N):
        step(K)
    prof = eng.profile_read()
    counts = {k: v[1] for k, v in prof.items()}
    assert counts['k_logic'] == counts['k_resetdone'] == counts['k_obs'] == N * K
    assert counts['k_obs_done'] == (N * K if eng.layout['reset_overlap'] else 0)
    assert counts['k_reset'] == 2 and counts['k_action_mask'] == 2
    if replays is not None:
        assert counts['k_replay'] == want[replays]
    else:
        assert counts['k_replay'] in (N, N * K)
    if sel is not None:
        assert counts['k_replay_sel'] == want[sel]
    for k, (ms, n) in prof.items():
        assert (ms > 0) == (n > 0), f'{k}: {n} launches in {ms} ms'
    # the read cleared the accumulators
    assert all(v == (0.0, 0) for v in eng.profile_read().values())
    # a deferred replay is no k_replay launch; the next plain step's is one
    step(1, defer_replay=True)
    prof = eng.profile_read()
    assert prof['k_replay'][1] == 0 and prof['k_logic'][1] == 1
    step(1)
    assert eng.profile_read()['k_replay'][1] == 1
    # off: further steps add nothing
    eng.profile(False)
    step(K)
    eng.action_mask()
    torch.cuda.synchronize()
    assert all(v == (0.0, 0) for v in eng.profile_read().values())
    eng.close()


# ---------------------------------------------------------------------------------------------------------------------
# stepping on a side stream
# ---------------------------------------------------------------------------------------------------------------------
FILLER_BYTES = 1 << 30
FILLER_CHAIN = 32


@pytest.mark.parametrize('cfg,B', [('eval_trio.yaml', 16), ('grid128_full_ep.yaml', 7)])
def test_stepping_on_a_side_stream(cfg, B):
    """Every engine call (reset, a masked reset before step 5, 30 steps, export_state after every call, action_mask) is
    made on a non-blocking side stream while the default stream is kept busy with work the side stream does not wait
    for: before each call a chain of FILLER_CHAIN device-to-device copies of a FILLER_BYTES buffer and an event behind
    it. The event is still pending when the call has been enqueued (asserted), then the side stream alone is
    synchronised and the results compared with the oracle: a launch, memset, copy or event the engine put on the
    default stream would still be queued behind the filler, and the comparison would see stale rows.

    Filler length: it has to outlast the host's enqueue of one engine call, not the kernels. Measured on the MI355X:
    the slowest enqueue of one call of this test took 0.48 ms on the host (grid128_full_ep; median 0.11 ms; eval_trio
    0.18 / 0.02 ms); one copy of the 1 GiB buffer takes 0.42 ms, so a chain of 16 copies (6.7 - 6.9 ms measured) has
    the 10x margin and the chain of 32 used here about 28x."""
    torch = _need_gpu()
    spec, eng = _engine(cfg, B)
    ob = OC.OracleBatch(spec, list(range(B)), BASE, PSEED)
    default = torch.cuda.current_stream(eng.device)
    side = torch.cuda.Stream(eng.device)
    fill = torch.zeros((2, FILLER_BYTES), dtype=torch.uint8, device=eng.device)
    enqueue, chains = [], []

    def call(fn):
        with torch.cuda.stream(default):
            ev0, ev = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            for _ in range(FILLER_CHAIN):
                fill[1].copy_(fill[0])
            ev.record()
        t0 = time.perf_counter()
        out = fn()  # on the side stream
        enqueue.append(time.perf_counter() - t0)
        assert not ev.query(), 'the filler on the default stream ended before the call was enqueued: lengthen it'
        side.synchronize()
        chains.append((ev0, ev))
        return out

    torch.cuda.synchronize()
    side.wait_stream(default)
    with torch.cuda.stream(side):
        _compared_run(torch, eng, ob, 30, stagger=5, call=call, mask_at=4)
    torch.cuda.synchronize()
    print(f'{cfg}: slowest enqueue of one engine call {1e3 * max(enqueue):.3f} ms, median '
          f'{1e3 * float(np.median(enqueue)):.3f} ms; filler chain {chains[-1][0].elapsed_time(chains[-1][1]):.2f} ms')
    assert ob.ended.min() >= 1  # every env went through an auto-reset (on the engine's second stream where it has one)
    eng.close()
    ob.close()


# ---------------------------------------------------------------------------------------------------------------------
# mfg_hbm_copy
# ---------------------------------------------------------------------------------------------------------------------
GUARD = 4096


def _guarded(torch, n, fill):
    """(whole buffer, its n payload bytes) with GUARD bytes of `fill` on both sides."""
    raw = torch.full((GUARD + n + GUARD,), fill, dtype=torch.uint8, device='cuda')
    return raw, raw[GUARD:GUARD + n]


@pytest.mark.parametrize('n', [16, 4080, 4096, 4112, (1 << 20) + 16])
def test_hbm_copy_copies_exactly_its_bytes(n):
    """16 B (one lane), 255 lanes, one full block, one lane into a second block, 1 MiB + 16 B: dst equals src and the
    guard regions around dst (and src) are untouched."""
    torch = _need_gpu()
    from mfg_amd.engine import hbm_copy
    gen = torch.Generator(device='cuda').manual_seed(n)
    sraw, src = _guarded(torch, n, 0xA5)
    src.copy_(torch.randint(0, 256, (n,), dtype=torch.uint8, device='cuda', generator=gen))
    keep = sraw.clone()
    draw, dst = _guarded(torch, n, 0x5A)
    hbm_copy(dst, src)
    torch.cuda.synchronize()
    assert torch.equal(dst, src)
    assert (draw[:GUARD] == 0x5A).all() and (draw[GUARD + n:] == 0x5A).all(), 'write outside dst'
    assert torch.equal(sraw, keep)


@pytest.mark.parametrize('what', ['zero', '8', '24', 'dst+8', 'src+8', 'dst-null', 'src-null'])
def test_hbm_copy_refuses_bad_arguments(what):
    """A size that is no positive multiple of 16 B, a pointer that is not 16-B aligned or NULL: the call returns
    non-zero and writes nothing."""
    torch = _need_gpu()
    from mfg_amd.engine import load_lib
    L = load_lib()
    n = 64
    _, src = _guarded(torch, n, 0xA5)
    draw, dst = _guarded(torch, n, 0x5A)
    d, s, nbytes = dst.data_ptr(), src.data_ptr(), 32
    if what == 'zero':
        nbytes = 0
    elif what in ('8', '24'):
        nbytes = int(what)
    elif what == 'dst+8':
        d += 8
    elif what == 'src+8':
        s += 8
    elif what == 'dst-null':
        d = None
    elif what == 'src-null':
        s = None
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.mfg_hbm_copy(ctypes.c_void_p(d), ctypes.c_void_p(s), nbytes, stream)
    torch.cuda.synchronize()
    assert rc != 0
    assert (draw == 0x5A).all(), 'a refused mfg_hbm_copy wrote to dst'
    assert L.mfg_last_error(None)  # the message of the failed argument check
