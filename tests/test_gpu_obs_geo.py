"""The dense render compiled for a window radius (pomdp_r 1, 2, 3: window geometry folded at compile time,
csrc/mfg_kernels.h ObsGeo) against the C oracle and against the generic render of the same spec.

Every case runs two engines in lockstep, one as mfg_create selects it and one with mfg_variant.obs_generic, on the
batched oracle loop of test_gpu_parity.py: each env against its own OracleEnv every step, f64 rewards ==, done, events
and obs bit for bit; and the two engines' obs buffers must be byte-identical (padding layers included)."""
import numpy as np
import pytest

from conftest import gpu_available
from mfg_amd.engine import EV_MISC

pytestmark = pytest.mark.gpu


def _engines(cfg, B):
    if not gpu_available():
        pytest.skip('no GPU')
    import torch
    from mfg_amd.spec import compile_spec
    from mfg_amd.engine import Engine
    spec = compile_spec(cfg)
    return torch, spec, Engine(spec, B), Engine(spec, B, variant={'obs_generic': 1})


def _buffers(torch, eng, K, odt):
    B, A, dev = eng.B, eng.A, eng.device
    return dict(obs=torch.zeros((K,) + eng.obs_shape(), dtype=odt, device=dev),
                reward=torch.zeros((K, B, A), dtype=torch.float64, device=dev),
                done=torch.zeros((K, B), dtype=torch.uint8, device=dev),
                ev_act=torch.zeros((K, B, A), dtype=torch.uint8, device=dev),
                ev_watch=torch.zeros((K, B, A), dtype=torch.uint8, device=dev),
                ev_misc=torch.zeros((K, B, EV_MISC), dtype=torch.int32, device=dev))


def _lockstep(cfg, steps, B, K=1, f32=False, geo_r=None):
    """steps env-steps in calls of K on both engines; returns how many episodes ended. geo_r: the radius the engine
    created without a variant must report (0: the generic render)."""
    import oracle as O
    from philox import synthetic_actions
    from mfg_amd.engine import events_from_rows
    assert steps % K == 0
    base, pseed = 1000, 7
    torch, spec, geo, gen = _engines(cfg, B)
    want_r = spec.c.pomdp_r if geo_r is None else geo_r
    assert geo.layout['obs_geo_r'] == want_r, 'render chosen by mfg_create'
    assert gen.layout['obs_geo_r'] == 0, 'mfg_variant.obs_generic forces the generic render'
    A, nl = spec.n_agents, spec.n_layers
    odt = np.float32 if f32 else np.float64
    ubits = np.uint32 if f32 else np.uint64
    bufs = [_buffers(torch, e, K, torch.float32 if f32 else torch.float64) for e in (geo, gen)]
    envs = [O.OracleEnv(spec, base + i) for i in range(B)]
    ref = [e.reset() for e in envs]
    obs0 = []
    for eng, buf in zip((geo, gen), bufs):
        eng.reset(obs=buf['obs'][0], init=True, seed_base=base)
        obs0.append(buf['obs'][0].cpu().numpy())
    assert obs0[0].tobytes() == obs0[1].tobytes(), 'reset obs: specialised vs generic render'
    for i in range(B):
        for a in range(A):
            assert (obs0[0][i, a, :nl[a]].view(ubits) == ref[i][a].astype(odt).view(ubits)).all(), \
                f'reset obs env {i} agent {a}'
    ndone = 0
    for t0 in range(0, steps, K):
        out = []
        for eng, buf in zip((geo, gen), bufs):
            eng.step(K, actions=None, philox_seed=pseed, step_base=t0, auto_reset=True, **buf)
            out.append({k: v.cpu().numpy() for k, v in buf.items()})
        assert out[0]['obs'].tobytes() == out[1]['obs'].tobytes(), f't{t0} obs: specialised vs generic render'
        for k in ('reward', 'done', 'ev_act', 'ev_watch', 'ev_misc'):
            assert out[0][k].tobytes() == out[1][k].tobytes(), f't{t0} {k}: the two engines'
        o = out[0]
        for k in range(K):
            t = t0 + k
            acts = synthetic_actions(pseed, np.arange(B), t, spec.n_actions)
            for i, env in enumerate(envs):
                r_ref, d_ref, ev_ref = env.step(acts[i])
                assert list(o['reward'][k, i]) == list(r_ref), f't{t} env{i} reward'
                assert bool(o['done'][k, i]) == d_ref, f't{t} env{i} done'
                ev = events_from_rows(o['ev_act'][k, i], o['ev_watch'][k, i], o['ev_misc'][k, i])
                assert list(ev['act'][:A]) == list(ev_ref.act[:A]), f't{t} env{i} act events'
                assert list(ev['watch'][:A]) == list(ev_ref.watch[:A]), f't{t} env{i} watch events'
                assert (ev['door_coll'], ev['door_coll_hi']) == (ev_ref.door_coll, ev_ref.door_coll_hi), \
                    f't{t} env{i} door collisions'
                assert ev['maint_coll'] == ev_ref.maint_coll, f't{t} env{i} maintainer collisions'
                if d_ref:
                    ndone += 1
                    ro = env.reset()
                else:
                    ro = env.obs_list()
                for a in range(A):
                    got, want = o['obs'][k, i, a, :nl[a]], ro[a].astype(odt)
                    if not (got.view(ubits) == want.view(ubits)).all():
                        dif = np.argwhere(got != want)
                        raise AssertionError(f't{t} env{i} agent{a} obs: {len(dif)} diffs, first '
                                             f'{[(tuple(x), got[tuple(x)], want[tuple(x)]) for x in dif[:6]]} '
                                             f'layers {spec.layer_names[a]} done={d_ref}')
    geo.close()
    gen.close()
    return ndone


def test_r3_c3_k8_across_the_episode_boundary():
    """The headline spec in the benched mode (K = 8, Philox actions, auto-reset, f64 obs) across the step-500 reset:
    the frozen ray origin (Q12) and the frozen battery and position (Q11) are active afterwards."""
    assert _lockstep('large8.yaml', 520, 32, K=8) >= 32


def test_r3_c3_f32():
    _lockstep('large8.yaml', 40, 32, K=8, f32=True)


@pytest.mark.parametrize('cfg', ['clean_and_bring.yaml', 'default_large.yaml'])
def test_r3_dirt_and_machines(cfg):
    """The DIRT instantiation (clean_and_bring) and the machines / maintainers one (default_large)."""
    _lockstep(cfg, 60, 16)


@pytest.mark.parametrize('cfg', ['wide40.yaml', 'maint_rooms.yaml'])
def test_r2(cfg):
    """wide40: 40 agents, agent masks wider than 32 bits."""
    _lockstep(cfg, 60, 8)


@pytest.mark.parametrize('cfg', ['rooms4_r1.yaml', 'large8_r1.yaml'])
def test_r1(cfg):
    _lockstep(cfg, 60, 16)


@pytest.mark.parametrize('tag', ['rooms4_r1', 'large8_r1'])
@pytest.mark.parametrize('seed', [0, 1])
def test_r1_vs_reference_fixture(tag, seed):
    """pomdp_r 1 against the reference's own recorded run (tests/golden), not only the oracle."""
    import test_gpu_parity as P
    P.test_engine_vs_reference_fixture(tag, tag + '.yaml', seed)


@pytest.mark.parametrize('r', [1, 2, 3])
def test_window_over_the_level_edge(r):
    """Agents start in the four corners and along the four borders (Positions): the first-visit table and the
    placement clamp against the grid on every side, where a folded fw or dd would show."""
    _lockstep(f'edge_r{r}.yaml', 8, 8)


def test_identifier_dedupe_inside_the_window():
    """65 doors (walls and doors with equal identifiers): the dedupe's wall suppression inside a 7 x 7 window."""
    _lockstep('qquad_doors.yaml', 40, 8)


@pytest.mark.parametrize('cfg', ['alltest16.yaml', 'large_full.yaml'])
def test_other_radii_keep_the_generic_render(cfg):
    """pomdp_r 4 and full observability have no compiled geometry: mfg_create reports the generic render and the
    results are the oracle's."""
    _lockstep(cfg, 24, 8, geo_r=0)


def test_c3_takes_the_specialised_render():
    torch, spec, geo, gen = _engines('large8.yaml', 4)
    assert geo.layout['obs_geo_r'] == 3 and gen.layout['obs_geo_r'] == 0
    geo.close()
    gen.close()
