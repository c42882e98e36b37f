"""Time the two fused loss heads alone (not bench.py: a side measurement): mfg_mc_returns + mfg_ppo_head at batch sizes
1,024 and 16,384 (T = 5, 12 actions) and mfg_seac_head at tools/bench_seac.py's head shape (8 agents x 8,192 envs,
T = 5, 12 actions; cross and own). Device events around windows of back-to-back calls; prints one JSON line with the
median / min / max per-call microseconds of the windows and a checksum of the outputs (loss, dlogits, dcritic).

    python tools/bench_heads.py LABEL

The library is the one mfg_amd.engine loads, so MFG_HIP_LIB=path/to/another/libmfg_hip.so times another build: to
compare two builds, alternate them in fresh processes and compare the lines."""
import hashlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / 'marl-factory-grid_amd'))
import torch  # noqa: E402
from mfg_amd import learn_lib  # noqa: E402

label = sys.argv[1] if len(sys.argv) > 1 else 'run'
L = learn_lib.lib()
st = torch.cuda.current_stream().cuda_stream
dev = 'cuda'
CALLS, WINDOWS = 200, 9


def timed(fn):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    per = []
    for _ in range(WINDOWS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        torch.cuda.synchronize()
        per.append(a.elapsed_time(b) * 1000.0 / CALLS)
    per.sort()
    return dict(median_us=per[len(per) // 2], min_us=per[0], max_us=per[-1])


def digest(*ts):
    h = hashlib.sha256()
    for t in ts:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()[:16]


out = dict(label=label)
g = torch.Generator().manual_seed(0)
for n in (1024, 16384):
    t, n_act = 5, 12
    m = n * t
    lg = (torch.randn((m, n_act), generator=g) * 1.5).to(dev)
    old = (lg.cpu() + torch.randn((m, n_act), generator=g) * 0.3).to(dev)
    cr = torch.randn(m, generator=g).to(dev)
    act = torch.randint(0, n_act, (m,), generator=g).to(torch.int32).to(dev)
    rew = (torch.randn((n, t), generator=g) * 0.5).to(dev)
    dn = (torch.rand((n, t), generator=g) < 0.15).float().to(dev)
    ret = torch.empty((n, t), device=dev)
    stats = torch.zeros(2, dtype=torch.float64, device=dev)
    ws = torch.empty(2048, dtype=torch.float64, device=dev)
    loss, dl, dc = torch.zeros((), device=dev), torch.empty((m, n_act), device=dev), torch.empty(m, device=dev)

    def ppo():
        assert L.mfg_mc_returns(rew.data_ptr(), t, dn.data_ptr(), t, n, t, 0.99, ret.data_ptr(), t, stats.data_ptr(),
                                ws.data_ptr(), st) == 0
        assert L.mfg_ppo_head(lg.data_ptr(), n_act, old.data_ptr(), n_act, cr.data_ptr(), act.data_ptr(),
                              ret.data_ptr(), stats.data_ptr(), m, n_act, 0.2, 0.5, 0.01, loss.data_ptr(),
                              dl.data_ptr(), n_act, dc.data_ptr(), ws.data_ptr(), st) == 0
    r = timed(ppo)
    r['digest'] = digest(loss, dl, dc)
    out[f'ppo_head_bs{n}'] = r

A, B, T, n_act = 8, 8192, 5, 12
for cross in (1, 0):
    nets = A if cross else 1
    lg = (torch.randn((nets, A * B, T + 1, n_act), generator=g) * 1.5).to(dev)
    cr = (torch.randn((nets, A * B, T + 1), generator=g) * 0.5).to(dev)
    act = torch.randint(0, n_act, (T, B, A), generator=g).to(torch.int32).to(dev)
    rew = (torch.randn((T, B, A), generator=g) * 0.5).to(dev)
    dn = (torch.rand((T, B), generator=g) < 0.2).float().to(dev)
    na = torch.full((A,), n_act, dtype=torch.int32, device=dev)
    loss, dl, dc = torch.zeros(A, device=dev), torch.empty_like(lg), torch.empty_like(cr)
    ws = torch.empty(A * 512, dtype=torch.float64, device=dev)

    def seac():
        assert L.mfg_seac_head(lg.data_ptr(), cr.data_ptr(), A, B, T, n_act, act.data_ptr(), B * A, A, 1,
                               rew.data_ptr(), B * A, A, 1, dn.data_ptr(), B, 1, 0, na.data_ptr(), 0.99, 0.95, 0.5,
                               0.01, cross, loss.data_ptr(), dl.data_ptr(), dc.data_ptr(), ws.data_ptr(), st) == 0
    r = timed(seac)
    r['digest'] = digest(loss, dl, dc)
    out[f'seac_head_cross{cross}'] = r
    del lg, dl
print(json.dumps(out))
