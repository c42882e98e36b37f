"""The cases of tests/test_gpu_packed_render.py, their oracle runs and the expected-row helpers, with the checks that need
no GPU: every case's oracle run, with the seeds and step counts the GPU test uses, really has the rows the case is about
(more than 64 entries: a queue flush inside the row; more than 128: two; empty rows), and the order helper gives the
entry order include/mfg.h states for mfg_packed_obs.

A packed row is the dense f32 row [lmax][h][w] of one agent (the oracle's f64 obs cast to float32). Its stored entries
stand in (64-cell block, layer, cell) order, which is ascending flat index when h*w <= 64, when the observation rays have
9..12 points (the render instantiated for MAXPTS 10 or 12) and in the long-ray render (obs_maxpts 0)."""
import functools

import numpy as np
import pytest

BASE, PSEED = 1000, 7

# cfg -> the render shape mfg_create selects (mfg_layout obs_maxpts, obs_waves), B, steps, whether a row over 128 entries
# and an empty row must occur, whether an episode end must be crossed (the packed_* configs have 8- and 12-step episodes;
# the older ones 500-step episodes, too long for a quick test). Every run must have a row over 64 entries but those of
# grid128_r10 and large_full (over64 False: their rows stay below 46 entries; they are here for their MAXPTS alone).
CASES = {
    # per-layer ballots, short rays
    'packed_r1.yaml': dict(maxpts=4, waves=1, B=8, steps=30, over128=False, empty=True, done=True),
    'packed_r2.yaml': dict(maxpts=6, waves=1, B=8, steps=30, over128=False, empty=True, done=True),
    'packed_r3.yaml': dict(maxpts=8, waves=1, B=4, steps=30, over128=True, empty=True, done=True),
    # the flattened pass
    'packed_r4.yaml': dict(maxpts=10, waves=1, B=4, steps=30, over128=True, empty=True, done=True),
    'packed_r5.yaml': dict(maxpts=12, waves=2, B=4, steps=30, over128=True, empty=True, done=True),
    # per-layer ballots over several 64-cell blocks
    'packed_full.yaml': dict(maxpts=14, waves=4, B=4, steps=30, over128=True, empty=True, done=True),
    'grid128_r10.yaml': dict(maxpts=24, waves=4, B=2, steps=10, over128=False, empty=False, done=False,
                             over64=False),
    'large_full.yaml': dict(maxpts=32, waves=1, B=2, steps=10, over128=False, empty=False, done=False,
                            over64=False),
    'grid128_r20.yaml': dict(maxpts=48, waves=1, B=2, steps=10, over128=False, empty=False, done=False),
    # long-ray
    'packed_lr81.yaml': dict(maxpts=0, waves=1, B=3, steps=10, over128=True, empty=False, done=True),
}
SHAPE_OF = {4: 'per-layer short', 6: 'per-layer short', 8: 'per-layer short', 10: 'flattened', 12: 'flattened',
            14: 'per-layer multi-block', 24: 'per-layer multi-block', 32: 'per-layer multi-block',
            48: 'per-layer multi-block', 0: 'long-ray'}
STAGGER_AT = 5  # the masked-reset case resets the odd envs before this step


def block_order(maxpts, dd):
    """Whether a render instantiated for `maxpts` (0: long-ray) stores a window of dd cells in (64-cell block, layer,
    cell) order that is not plain ascending flat index (include/mfg.h, mfg_packed_obs)."""
    return not (dd <= 64 or maxpts in (10, 12) or maxpts == 0)


def expected_idx(row, dd, blocks):
    """The flat indices of the nonzero entries of a dense f32 row [layers * dd] in the order the packed row stores them:
    ascending, or with `blocks` by 64-cell block of the window first, then layer, then cell."""
    nz = np.flatnonzero(row)
    if blocks:
        nz = nz[np.argsort((nz % dd) // 64, kind='stable')]
    return nz


@functools.lru_cache(maxsize=None)
def oracle_run(cfg, B, steps, stagger=None):
    """(spec, rows f32 [1 + steps][B][A][lmax * dd], done bool [steps][B]) of B oracle envs seeded BASE + i on the Philox
    actions with auto-reset: rows[0] the reset obs, rows[1 + t] the obs after step t (the new episode's first obs where
    the episode ended). stagger: the odd envs are reset before that step, as a masked mfg_reset does; rows gets the obs
    of that render inserted before step `stagger`'s (so it has 2 + steps entries)."""
    import oracle as O
    from philox import synthetic_actions
    from mfg_amd.spec import compile_spec
    spec = compile_spec(cfg)
    A, dd = spec.n_agents, spec.obs_hw[0] * spec.obs_hw[1]
    kdim = max(spec.n_layers) * dd

    def pack(env_obs):
        out = np.zeros((B, A, kdim), np.float32)
        for i in range(B):
            for a in range(A):
                flat = env_obs[i][a].astype(np.float32).ravel()
                out[i, a, :flat.size] = flat
        return out

    envs = [O.OracleEnv(spec, BASE + i) for i in range(B)]
    rows = [pack([e.reset() for e in envs])]
    done = np.zeros((steps, B), bool)
    for t in range(steps):
        if t == stagger:
            rows.append(pack([e.reset() if i % 2 else e.obs_list() for i, e in enumerate(envs)]))
        acts = synthetic_actions(PSEED, np.arange(B), t, spec.n_actions)
        obs = []
        for i, env in enumerate(envs):
            _, d, _ = env.step(acts[i])
            done[t, i] = d
            obs.append(env.reset() if d else env.obs_list())
        rows.append(pack(obs))
    for e in envs:
        e.close()
    rows = np.stack(rows)
    rows.setflags(write=False)
    return spec, rows, done


def counts(rows):
    return (rows != 0).sum(-1)


def assert_not_vacuous(cfg, rows, done, over128=None, empty=None, need_done=None):
    """The run holds what its case is about; the case's own expectations unless given."""
    c = CASES[cfg]
    n = counts(rows)
    if c.get('over64', True):
        assert n.max() > 64, f'{cfg}: no row with more than 64 entries (largest {n.max()}): no queue flush inside a row'
    else:
        assert n.max() <= 64, f'{cfg}: rows over 64 entries after all: say so in CASES'
    if c['over128'] if over128 is None else over128:
        assert n.max() > 128, f'{cfg}: no row with more than 128 entries (largest {n.max()})'
    if c['empty'] if empty is None else empty:
        assert (n == 0).any(), f'{cfg}: no empty row'
    if c['done'] if need_done is None else need_done:
        assert done.any(), f'{cfg}: no episode end in {len(done)} steps'
    return n


@pytest.mark.parametrize('cfg', list(CASES))
def test_oracle_run_is_not_vacuous(cfg):
    """Rows over 64 (and, where the case says so, over 128 and of 0) entries and an episode end, in the very run the GPU
    cases compare against; the row fits the u16 index."""
    c = CASES[cfg]
    spec, rows, done = oracle_run(cfg, c['B'], c['steps'])
    n = assert_not_vacuous(cfg, rows, done)
    assert rows.shape[-1] < 65536
    print(f'{cfg}: {SHAPE_OF[c["maxpts"]]}, MAXPTS {c["maxpts"]}, row width {rows.shape[-1]}, largest row {n.max()}, '
          f'rows > 64: {(n > 64).sum()}, > 128: {(n > 128).sum()}, empty: {(n == 0).sum()}, ends: {done.sum()}')


@pytest.mark.parametrize('cfg', ['packed_r3.yaml', 'packed_full.yaml'])
def test_oracle_run_with_masked_reset_is_not_vacuous(cfg):
    """The masked-reset case: the odd envs restart before step STAGGER_AT, so their episodes end at other steps."""
    c = CASES[cfg]
    spec, rows, done = oracle_run(cfg, c['B'], c['steps'], STAGGER_AT)
    assert_not_vacuous(cfg, rows, done)
    assert len(rows) == c['steps'] + 2
    ends = [set(np.flatnonzero(done[:, i])) for i in range(c['B'])]
    assert ends[0] and ends[1] and ends[0] != ends[1], 'odd and even envs end at different steps'


def test_cap_cases_truncate_and_do_not():
    """The cap cases: each cap below the largest row truncates some row and leaves another whole, so both sides of
    PackedObs.check() and of the slot fill are met; 64 and 128 are rows' flush boundaries."""
    for cfg, caps in (('packed_r3.yaml', (1, 63, 64, 65, 100, 128)), ('packed_lr81.yaml', (64, 100))):
        c = CASES[cfg]
        _, rows, _ = oracle_run(cfg, c['B'], c['steps'])
        n = counts(rows)
        for cap in caps:
            assert (n > cap).any() and (n < cap).any(), f'{cfg} cap {cap}'
        assert ((n > 64) & (n < 128)).any(), 'a cap of 100 or 128 that falls inside the second flush'


def test_expected_idx_orders():
    """The order helper against include/mfg.h's wording, on hand-made rows: 2 layers of a 70-cell window (two 64-cell
    blocks: cells 0..63 and 64..69)."""
    dd = 70
    row = np.zeros(2 * dd, np.float32)
    for l, cell in ((0, 3), (0, 65), (1, 0), (1, 63), (1, 64), (0, 69)):
        row[l * dd + cell] = 1.0 + l
    asc = [3, 65, 69, 70, 133, 134]
    assert expected_idx(row, dd, False).tolist() == asc
    # block 0: (layer 0, cell 3), (layer 1, cells 0, 63); block 1: (layer 0, cells 65, 69), (layer 1, cell 64)
    assert expected_idx(row, dd, True).tolist() == [3, 70, 133, 65, 69, 134]
    # one block: the two orders agree
    one = np.zeros(3 * 49, np.float32)
    one[[5, 48, 49, 100, 146]] = 0.5
    assert expected_idx(one, 49, True).tolist() == expected_idx(one, 49, False).tolist() == [5, 48, 49, 100, 146]
    assert expected_idx(np.zeros(10, np.float32), 5, True).size == 0
    # which renders store in block order (h*w <= 64, rays of 9..12 points and the long-ray render do not)
    assert [block_order(m, d) for m, d in ((8, 49), (10, 81), (12, 121), (14, 195), (48, 1681), (0, 361), (14, 60))] == \
        [False, False, False, True, True, False, False]
