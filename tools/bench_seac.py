"""Time the per-agent-network learners on one GPU (not bench.py: a side measurement). Writes profiles/seac.json.

    timeout 900 python tools/bench_seac.py [--config large8.yaml] [--batch 8192] [--out profiles/seac.json]
                                           [--figures FILE]

Two parts, each warmed up first, medians over alternating rounds so the compared calls see the same clock state:

  head   the fused loss head (mfg_seac_head: loss, dlogits and dcritic of all networks in one call) against the torch
         iac_loss_terms / seac_loss_terms forward + backward on the same window-sized logits, device events per call,
         for IAC ([A B, T+1, n_act] rows) and SEAC ([A, A B, T+1, n_act])
  loop   env-steps/s of BatchedIAC and BatchedSEAC with fused_head on and off, and of BatchedA2C (eager update, the same
         layer sizes, one shared network) as the yardstick, in alternating rounds of --loop-steps env-steps (host clock
         around a device synchronise), every round and the median

--figures: the JSON that tests/test_gpu_seac.py writes with MFG_SEAC_FIGURES set (the head's measured errors against
f64 and their ratio to the f32 tensor code's), stored as head_test_figures.
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / 'marl-factory-grid_amd'))

HYP = (0.99, 0.01, 0.5, 0.0)  # gamma, entropy_coef, vf_coef, gae_coef


def head_inputs(torch, A, B, T, n_act, cross, dev, seed=0):
    g = torch.Generator().manual_seed(seed)
    nets = A if cross else 1
    return dict(A=A, B=B, T=T, cross=cross,
                logits=(torch.randn((nets, A * B, T + 1, n_act), generator=g) * 1.5).to(dev),
                critic=(torch.randn((nets, A * B, T + 1), generator=g) * 0.7).to(dev),
                act=torch.randint(0, n_act, (T, B, A), generator=g).to(torch.int32).to(dev),
                reward=(torch.randn((T, B, A), generator=g) * 0.5).to(dev),
                done=(torch.rand((T, B), generator=g) < 0.1).float().to(dev),
                n_act=torch.full((A,), n_act, dtype=torch.int32, device=dev))


def run_head(torch, S, x, fused):
    A, B, T = x['A'], x['B'], x['T']
    lg, cr = x['logits'].clone().requires_grad_(), x['critic'].clone().requires_grad_()
    if fused:
        l2, c2 = (lg, cr) if x['cross'] else (lg[0], cr[0])
        loss = S._SEACHead.apply(l2, c2, x['act'], (B * A, A, 1), x['reward'], (B * A, A, 1), x['done'], (B, 1, 0),
                                 x['n_act'], A, B, *HYP, x['cross'])
    else:
        acts, rew = x['act'].permute(2, 1, 0).long(), x['reward'].permute(2, 1, 0)
        dn = x['done'].t()[None].expand(A, B, T)
        if x['cross']:
            loss = S.seac_loss_terms(lg.view(A, A, B, T + 1, -1)[:, :, :, :T], cr.view(A, A, B, T + 1), acts, rew, dn,
                                     *HYP)
        else:
            loss = S.iac_loss_terms(lg.view(A, B, T + 1, -1)[:, :, :T], cr.view(A, B, T + 1), acts, rew, dn, *HYP)
    dl, dc = torch.autograd.grad(loss.sum(), [lg, cr])
    return loss.detach(), dl, dc


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='large8.yaml')
    ap.add_argument('--batch', type=int, default=8192)
    ap.add_argument('--n-steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--loop-steps', type=int, default=20)
    ap.add_argument('--loop-rounds', type=int, default=3)
    ap.add_argument('--figures', default=None)
    ap.add_argument('--out', default=str(ROOT / 'profiles' / 'seac.json'))
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_seac needs a GPU: no timing is taken without one')
    import mfg_amd.marl as M
    import mfg_amd.seac as S
    from mfg_amd.factory import BatchedFactory
    dev = torch.device('cuda', 0)
    T = args.n_steps
    out = {'config': args.config, 'envs': args.batch, 'n_steps': T, 'device': torch.cuda.get_device_name(dev),
           'warmup_calls': args.warmup, 'timed_calls': args.calls}

    def make(kind):
        f = BatchedFactory(args.config, args.batch, seed_base=0)
        if kind == 'a2c':
            return f, M.BatchedA2C(f, n_steps=T, check_cap=True, graph=False)
        cls = M.BatchedSEAC if kind.startswith('seac') else M.BatchedIAC
        return f, cls(f, n_steps=T, fused_head=kind.endswith('fused'))
    kinds = ('iac_fused', 'iac_torch', 'seac_fused', 'seac_torch', 'a2c')
    loops = {k: make(k) for k in kinds}
    A, n_act = loops['iac_fused'][1].A, loops['iac_fused'][1].n_max
    out.update(n_agents=A, n_actions=n_act,
               activation_bytes={k: loops[k + '_fused'][1].activation_bytes() for k in ('iac', 'seac')})

    # ---- head
    out['head'] = {}
    for name, cross in (('iac', False), ('seac', True)):
        x = head_inputs(torch, A, args.batch, T, n_act, cross, dev)
        calls = {'fused': lambda: run_head(torch, S, x, True), 'torch': lambda: run_head(torch, S, x, False)}
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
        res = {'network_row_pairs': x['logits'].shape[0] * x['logits'].shape[1], 'elements_per_pair': T}
        for k in calls:
            tms = np.array([a.elapsed_time(b) for a, b in ev[k][args.warmup:]])
            res[k] = {'median_ms': float(np.median(tms)), 'p10_ms': float(np.percentile(tms, 10)),
                      'p90_ms': float(np.percentile(tms, 90))}
        res['torch_over_fused'] = res['torch']['median_ms'] / res['fused']['median_ms']
        res['timed'] = 'forward + backward incl. the copies of logits / critic that autograd.grad needs'
        out['head'][name] = res
        del x
    torch.cuda.empty_cache()

    # ---- loop
    for k, (f, tr) in loops.items():
        for _ in range(2 * T):
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
    out['loop'] = {'loop_steps': args.loop_steps, 'rounds': args.loop_rounds, 'a2c_update': 'eager',
                   'peak_device_bytes': int(torch.cuda.max_memory_allocated(dev))}
    for k in kinds:
        out['loop'][k] = {'env_steps_per_s_median': float(np.median(rates[k])), 'env_steps_per_s': rates[k]}
    for f, _ in loops.values():
        f.close()
    if args.figures and Path(args.figures).exists():
        out['head_test_figures'] = json.loads(Path(args.figures).read_text())
    Path(args.out).parent.mkdir(parents=True, exist_ok=True)
    Path(args.out).write_text(json.dumps(out, indent=1) + '\n')
    print(json.dumps(out))


if __name__ == '__main__':
    main()
