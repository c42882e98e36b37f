"""mfg_replay against CPython itself: random.shuffle from the env's own MT19937 state on the env's own floor
permutation, `debt` times. The levels put the shuffle's first rank hi = nf - 1 below, at and above the replay's tail
bound (MFG_RP_TAIL: chunks at icur <= TAIL take per-lane widths), the MT indices put chunks before, across and
past the state's end; what the cases contain is shown on the census model by test_replay_tail_cases.py."""
import numpy as np
import pytest

from conftest import gpu_available
from replay_tail_cases import B, LEVELS, cpython, env_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('level', range(len(LEVELS)), ids=[f"{c.split('.')[0]}{'-full_temper' if v else ''}"
                                                           for c, v, _ in LEVELS])
def test_replay_vs_cpython(level):
    if not gpu_available():
        pytest.skip('no GPU')
    import torch
    from mfg_amd.engine import HDR, Engine
    from mfg_amd.spec import compile_spec
    cfg, variant, nf = LEVELS[level]
    spec = compile_spec(cfg)
    assert spec.c.n_floor == nf
    eng = Engine(spec, B, variant=variant)
    eng.reset(init=True, seed_base=0)
    L = eng.layout
    st = eng.export_state().cpu().numpy().copy()
    o_hdr, o_mt, o_perm = L['o_hdr'], L['o_mt'], L['o_perm']
    hdr = st[:, o_hdr:o_hdr + 4 * 40].view(np.int32)
    mtw = st[:, o_mt:o_mt + 4 * 624].view(np.uint32)
    cases = [env_case(level, e) for e in range(B)]
    for e, (mt, mti, debt) in enumerate(cases):
        mtw[e] = mt
        hdr[e, HDR['mt_idx']] = mti
        hdr[e, HDR['debt']] = debt
    assert (st[:, o_mt:o_mt + 4 * 624].view(np.uint32)[B - 1] == np.asarray(cases[B - 1][0], np.uint32)).all()
    src = torch.from_numpy(st).to(eng.device)
    stream = torch.cuda.current_stream(eng.device).cuda_stream

    def run():
        eng.import_state(src)
        rc = eng.L.mfg_replay(eng.h, stream)
        assert rc == 0, eng.L.mfg_last_error(eng.h)
        torch.cuda.synchronize()
        return eng.export_state().cpu().numpy()

    out = run()
    again = run()
    eng.close()
    assert out.tobytes() == again.tobytes(), 'a second run from the same input differs'
    ohdr = out[:, o_hdr:o_hdr + 4 * 40].view(np.int32)
    omt = out[:, o_mt:o_mt + 4 * 624].view(np.uint32)
    operm = out[:, o_perm:o_perm + 2 * nf].view(np.uint16)
    iperm = st[:, o_perm:o_perm + 2 * nf].view(np.uint16)
    for e, (mt, mti, debt) in enumerate(cases):
        r = cpython(mt, mti)
        want = [int(x) for x in iperm[e]]
        for _ in range(debt):
            r.shuffle(want)
        what = f'{cfg} env {e} (mt_idx {mti}, debt {debt})'
        assert [int(x) for x in operm[e]] == want, f'{what}: permutation'
        state = r.getstate()[1]
        assert int(ohdr[e, HDR['mt_idx']]) == state[624], f'{what}: mt_idx'
        assert (omt[e] == np.asarray(state[:624], np.uint32)).all(), f'{what}: MT words'
        assert int(ohdr[e, HDR['debt']]) == 0, f'{what}: debt'
    # nothing else in the record moves
    keep = np.ones(st.shape[1], bool)
    keep[o_mt:o_mt + 4 * 624] = False
    keep[o_perm:o_perm + 2 * nf] = False
    for k in ('mt_idx', 'debt'):
        keep[o_hdr + 4 * HDR[k]:o_hdr + 4 * HDR[k] + 4] = False
    assert (out[:, keep] == st[:, keep]).all(), f'{cfg}: record bytes outside MT, permutation, mt_idx and debt changed'
