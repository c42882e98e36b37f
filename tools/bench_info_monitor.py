"""Time the device info monitor against the torch info columns on one GPU (not bench.py: a side measurement).

    timeout 600 python tools/bench_info_monitor.py [--config large8.yaml] [--batch 65536] [--out profiles/info_monitor.json]

The engine is stepped `--settle` times with uniform random actions so the event rows are those of a running batch.
Then ONE timed region: `--warmup` + `--calls` rounds, each round timing three calls on the last step's buffers with
device events, alternating so all three see the same clock state:

  fold      mfg_info_step, K = 1, vals / pres NULL (the per-episode fold alone)
  columns   mfg_info_step, K = 1, writing vals f64 / pres u8 [B, Kc] as well
  torch     BatchedFactory.info_columns (mfg_amd.info_columns.InfoColumns: one group of torch ops per op)

Reported: median, 10th / 90th percentile per call, the ratio to the engine step (`--step-ms`, BENCH_r06.json:
1.854 ms at B = 65,536), and the achieved GB/s of the fold against the bytes it has to move per env-step
(2A event bytes + 64 B ev_misc + 4A actions + 8A rewards + 1 done, plus the accumulators read and written once per
call: 2 * 12 Kc + 16).
"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / 'marl-factory-grid_amd'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='large8.yaml')
    ap.add_argument('--batch', type=int, default=65536)
    ap.add_argument('--settle', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--step-ms', type=float, default=1.854)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'info_monitor.json'))
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_info_monitor needs a GPU: no timing is taken without one')
    from mfg_amd.factory import BatchedFactory
    from mfg_amd.monitor import BatchedEnvMonitor
    B = args.batch
    bf = BatchedFactory(args.config, B, seed_base=0)
    mon = BatchedEnvMonitor(bf)
    m, A, Kc = mon.monitor, bf.spec.n_agents, mon.monitor.Kc
    mon.reset()
    n_act = torch.tensor(bf.spec.n_actions, dtype=torch.float64, device=bf.device)
    gen = torch.Generator(device=bf.device)
    gen.manual_seed(1)
    acts = None
    for _ in range(args.settle):
        acts = (torch.rand((B, A), dtype=torch.float64, device=bf.device, generator=gen) * n_act).to(torch.int32)
        mon.step(acts)
    vals = torch.zeros((1, B, Kc), dtype=torch.float64, device=bf.device)
    pres = torch.zeros((1, B, Kc), dtype=torch.uint8, device=bf.device)
    rows = (bf.ev_act, bf.ev_watch, bf.ev_misc, bf.reward, bf.done)
    calls = {'fold': lambda: m.step(1, *rows, actions=acts),
             'columns': lambda: m.step(1, *rows, actions=acts, vals=vals, pres=pres),
             'torch': lambda: bf.info_columns(acts)}
    n = args.warmup + args.calls
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
          for k in calls}
    for i in range(n):  # the timed region
        for k, f in calls.items():
            a, b = ev[k][i]
            a.record()
            f()
            b.record()
    torch.cuda.synchronize()
    row_bytes = 2 * A + 64 + 4 * A + 8 * A + 1
    acc_bytes = 2 * 12 * Kc + 16
    out = {'config': args.config, 'batch': B, 'n_agents': A, 'n_columns': Kc, 'n_ops': mon.program.n_ops,
           'keys_per_lane': m.keys_per_lane, 'waves_per_block': m.waves_per_block, 'lds_bytes_per_block': m.lds_bytes,
           'warmup_calls': args.warmup, 'timed_calls': args.calls, 'engine_step_ms': args.step_ms,
           'device': torch.cuda.get_device_name(bf.device),
           'fold_bytes_per_env_step': {'rows': row_bytes, 'accumulators': acc_bytes}}
    for k in calls:
        t = np.array([a.elapsed_time(b) for a, b in ev[k][args.warmup:]])
        out[k] = {'median_ms': float(np.median(t)), 'p10_ms': float(np.percentile(t, 10)),
                  'p90_ms': float(np.percentile(t, 90)), 'min_ms': float(t.min()), 'max_ms': float(t.max()),
                  'ratio_to_engine_step': float(np.median(t) / args.step_ms)}
    sec = out['fold']['median_ms'] * 1e-3
    out['fold']['achieved_GBs_rows'] = B * row_bytes / sec / 1e9
    out['fold']['achieved_GBs_rows_and_accumulators'] = B * (row_bytes + acc_bytes) / sec / 1e9
    out['torch_over_columns'] = out['torch']['median_ms'] / out['columns']['median_ms']
    out['torch_over_fold'] = out['torch']['median_ms'] / out['fold']['median_ms']
    mon.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
