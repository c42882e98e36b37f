"""Time the MAPPO learner on one GPU (not bench.py: a side measurement). Writes profiles/mappo.json.

    timeout 900 python tools/bench_mappo.py [--config large8.yaml] [--batch 8192] [--out profiles/mappo.json]

Three parts, each warmed up first, medians over alternating rounds so the compared calls see the same clock state:

  head      the fused loss head (mfg_mc_returns + mfg_ppo_head, forward and backward in one pass) against the torch
            mappo_loss_terms forward + backward on the same [batch_size * n_steps, n_act] rows, device events per call,
            at batch_size 1,024 and 16,384; with the achieved GB/s of the fused head against the bytes it has to move
            (per element: 2 n_act logits + critic + action + return read, n_act + 1 gradients written, plus the
            reward / done / return rows of mfg_mc_returns)
  accuracy  maximum error against mappo_loss_terms in f64 of the fused head and of the f32 tensor code, and their ratio
  loop      env-steps/s of BatchedMAPPO with fused_head on and off, and of BatchedA2C (eager update, the same network
            sizes) as the yardstick, in alternating rounds of --loop-steps env-steps (host clock around a device
            synchronise)
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / 'marl-factory-grid_amd'))

HYP = dict(gamma=0.99, entropy_coef=0.01, vf_coef=0.5, clip_range=0.2)


def head_inputs(torch, n, t, n_act, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn((n, t, n_act), generator=g) * 1.5
    old = logits + torch.randn((n, t, n_act), generator=g) * 0.3 * (torch.rand((n, t, 1), generator=g) < 0.7)
    return dict(logits=logits.to(dev), old=old.to(dev), critic=(torch.randn((n, t), generator=g) * 0.7).to(dev),
                act=torch.randint(0, n_act, (n, t), generator=g).to(dev),
                reward=(torch.randn((n, t), generator=g) * 0.5).to(dev),
                done=(torch.rand((n, t), generator=g) < 0.1).float().to(dev))


def run_head(torch, M, x, fused, dtype=None):
    dtype = dtype or torch.float32
    lg = x['logits'].to(dtype).requires_grad_()
    cr = x['critic'].to(dtype).requires_grad_()
    args = (lg, cr, x['old'].to(dtype), x['act'], x['reward'].to(dtype), x['done'].to(dtype), HYP['gamma'],
            HYP['entropy_coef'], HYP['vf_coef'], HYP['clip_range'])
    loss = M._PPOHead.apply(*args) if fused else M.mappo_loss_terms(*args)
    dl, dc = torch.autograd.grad(loss, [lg, cr])
    return loss.detach(), dl, dc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='large8.yaml')
    ap.add_argument('--batch', type=int, default=8192)
    ap.add_argument('--n-steps', type=int, default=5)
    ap.add_argument('--buffer-size', type=int, default=20)
    ap.add_argument('--batch-size', type=int, default=1024)
    ap.add_argument('--n-updates', type=int, default=4)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--loop-steps', type=int, default=40)
    ap.add_argument('--loop-rounds', type=int, default=3)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'mappo.json'))
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_mappo needs a GPU: no timing is taken without one')
    import mfg_amd.marl as M
    from mfg_amd.factory import BatchedFactory
    dev = torch.device('cuda', 0)
    T = args.n_steps
    out = {'config': args.config, 'envs': args.batch, 'n_steps': T, 'device': torch.cuda.get_device_name(dev),
           'warmup_calls': args.warmup, 'timed_calls': args.calls}

    # ---- loop: built first so the head runs on the config's action count
    def make(kind):
        f = BatchedFactory(args.config, args.batch, seed_base=0)
        if kind == 'a2c':
            return f, M.BatchedA2C(f, n_steps=T, check_cap=True, graph=False)
        return f, M.BatchedMAPPO(f, n_steps=T, buffer_size=args.buffer_size, batch_size=args.batch_size,
                                 n_updates=args.n_updates, fused_head=(kind == 'mappo_fused'), **HYP)
    kinds = ('mappo_fused', 'mappo_torch', 'a2c')
    loops = {k: make(k) for k in kinds}
    n_act = loops['mappo_fused'][1].n_actions
    out['n_actions'] = n_act

    # ---- head
    out['head'] = {}
    for bs in (1024, 16384):
        x = head_inputs(torch, bs, T, n_act, dev)
        calls = {'fused': lambda: run_head(torch, M, x, True), 'torch': lambda: run_head(torch, M, x, False)}
        n = args.warmup + args.calls
        ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
              for k in calls}
        for i in range(n):
            for k, fn in calls.items():
                a, b = ev[k][i]
                a.record()
                fn()
                b.record()
        torch.cuda.synchronize()
        m = bs * T
        elem_bytes = 4 * (2 * n_act + 3) + 4 * (n_act + 1) + 4 * 3  # head reads + writes, returns' reward/done/ret
        res = {'rows': m, 'bytes_per_element': elem_bytes}
        for k in calls:
            tms = np.array([a.elapsed_time(b) for a, b in ev[k][args.warmup:]])
            res[k] = {'median_ms': float(np.median(tms)), 'p10_ms': float(np.percentile(tms, 10)),
                      'p90_ms': float(np.percentile(tms, 90))}
        res['torch_over_fused'] = res['torch']['median_ms'] / res['fused']['median_ms']
        res['fused_GBs_incl_launch_gaps'] = m * elem_bytes / (res['fused']['median_ms'] * 1e-3) / 1e9
        out['head'][f'batch_size_{bs}'] = res

    # ---- accuracy
    out['accuracy'] = {}
    for bs in (3, 257, 16384):
        x = head_inputs(torch, bs, T, n_act, dev, seed=1)
        ref = run_head(torch, M, x, False, torch.float64)
        e = {}
        for k, fused in (('fused', True), ('torch_f32', False)):
            got = run_head(torch, M, x, fused)
            e[k] = [float((a.double() - b).abs().max()) for a, b in zip(got, ref)]
        e['ratio_fused_over_torch_f32'] = [a / b if b else None for a, b in zip(e['fused'], e['torch_f32'])]
        e['order'] = ['loss', 'dlogits', 'dcritic']
        out['accuracy'][f'rows_{bs * T}'] = e

    # ---- loop
    fill = args.buffer_size + T  # MAPPO learns from here on
    for k, (f, tr) in loops.items():
        for _ in range(fill + 2 * T):
            tr.step()
    torch.cuda.synchronize()
    rates = {k: [] for k in kinds}
    for r in range(args.loop_rounds):
        for k in (kinds if r % 2 == 0 else kinds[::-1]):
            tr = loops[k][1]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.loop_steps):
                tr.step()
            torch.cuda.synchronize()
            rates[k].append(args.batch * args.loop_steps / (time.perf_counter() - t0))
    mp = loops['mappo_fused'][1]
    out['loop'] = {'buffer_size': args.buffer_size, 'batch_size': args.batch_size, 'n_updates': args.n_updates,
                   'loop_steps': args.loop_steps, 'rounds': args.loop_rounds,
                   'mappo_buffer_bytes': mp.buffer_bytes(), 'mappo_updates': mp.updates,
                   'mappo_skipped_updates': mp.skipped_updates, 'a2c_update': 'eager'}
    for k in kinds:
        out['loop'][k] = {'env_steps_per_s_median': float(np.median(rates[k])), 'env_steps_per_s': rates[k]}
    for f, _ in loops.values():
        f.close()
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
