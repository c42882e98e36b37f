#!/usr/bin/env python3
"""Time per call of mfg_action_mask beside one k_logic launch at the same shape, from the engine's own mfg_profile
counters (device events around each launch). Windows of `--calls` mask calls and of `--calls` K = 1 steps alternate, so
both kernels see the same states and the same neighbours on the machine; the states keep moving (random actions,
auto-reset). Prints one JSON line.
usage: python tools/bench_action_mask.py [--config large8.yaml] [--envs 65536] [--windows 9] [--calls 50]"""
import argparse
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / 'marl-factory-grid_amd'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--config', default='large8.yaml')
    ap.add_argument('--envs', type=int, default=65536)
    ap.add_argument('--windows', type=int, default=9)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=100)
    args = ap.parse_args()
    import torch
    from mfg_amd.engine import Engine
    from mfg_amd.spec import compile_spec
    assert torch.cuda.is_available(), 'needs an MI355X: there is no CPU path to time'
    spec = compile_spec(args.config)
    eng = Engine(spec, args.envs)
    eng.reset(init=True, seed_base=0)
    mask = torch.zeros((eng.B, eng.A), dtype=torch.int32, device=eng.device)
    t = 0

    def steps(n):
        nonlocal t
        for _ in range(n):  # Philox actions, no obs: k_logic (+ the resets and the replay, counted apart)
            eng.step(1, philox_seed=1, step_base=t, auto_reset=True)
            t += 1

    steps(args.warmup)
    for _ in range(10):
        eng.action_mask(out=mask)
    torch.cuda.synchronize()
    eng.profile(True)
    eng.profile_read()
    m_us, l_us = [], []
    for _ in range(args.windows):
        for _ in range(args.calls):
            eng.action_mask(out=mask)
        p = eng.profile_read()
        assert p['k_action_mask'][1] == args.calls
        m_us.append(p['k_action_mask'][0] / args.calls * 1e3)
        steps(args.calls)
        p = eng.profile_read()
        assert p['k_logic'][1] % args.calls == 0  # (specs with an in-step dirt spawn launch k_logic twice per step)
        l_us.append(p['k_logic'][0] / args.calls * 1e3)
    eng.profile(False)
    bits = int(sum(bin(int(x) & 0xFFFFFFFF).count('1') for x in mask[:1024].flatten().tolist()))
    out = dict(config=args.config, envs=args.envs, agents=eng.A, n_actions=list(spec.n_actions),
               record_bytes=eng.layout['size'], step_prefix_bytes=eng.layout['o_logic'], windows=args.windows,
               calls_per_window=args.calls,
               action_mask_us=dict(median=round(statistics.median(m_us), 2), min=round(min(m_us), 2),
                                   max=round(max(m_us), 2)),
               k_logic_us=dict(median=round(statistics.median(l_us), 2), min=round(min(l_us), 2), max=round(max(l_us), 2)),
               ratio_mask_over_logic=round(statistics.median(m_us) / statistics.median(l_us), 3),
               valid_share_first_1024_envs=round(bits / (1024 * sum(spec.n_actions)), 4))
    print(json.dumps(out))
    eng.close()


if __name__ == '__main__':
    main()
