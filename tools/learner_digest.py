#!/usr/bin/env python3
"""A fingerprint and a work count of the on-GPU learners, for A/B runs of a refactor against its parent: run this file
from each tree (it imports the package next to it) and compare the JSON lines.

Per learner, with fixed seeds and explicit generators on large8.yaml:
  * digest: SHA-256 over every parameter and last_loss after a few windows of training;
  * act / update: the aten ops a TorchDispatchMode sees (views included) plus the learn_lib.call invocations, over one
    acting step and over one eager learn call (not for the graph-captured learner: a replay shows no ops).
usage: python tools/learner_digest.py [--batch 256] [--windows 3] [--only NAME ...] [--params DIR] [--ops]
"""
import argparse
import collections
import hashlib
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / 'marl-factory-grid_amd'))

T = 5  # n_steps of every learner here


def learners(M, gen):
    """name -> (constructor on a factory, env-steps that make `windows` learn calls, graph-captured?)."""
    return {
        'a2c_reuse': (lambda f: M.BatchedA2C(f, n_steps=T, generator=gen()), lambda w: w * T, False),
        'a2c_recompute': (lambda f: M.BatchedA2C(f, n_steps=T, generator=gen(), reuse_acting=False),
                          lambda w: w * T, False),
        # (no explicit generator: its draws would keep acting on the eager path; two eager warm-ups, the capture, replays)
        'a2c_graph': (lambda f: M.BatchedA2C(f, n_steps=T, graph=True, act_graph=True), lambda w: (w + 2) * T, True),
        'mappo': (lambda f: M.BatchedMAPPO(f, n_steps=T, buffer_size=2 * T, batch_size=256, generator=gen()),
                  lambda w: (w + 1) * T, False),
        'iac': (lambda f: M.BatchedIAC(f, n_steps=T, generator=gen()), lambda w: w * T, False),
        'seac': (lambda f: M.BatchedSEAC(f, n_steps=T, generator=gen()), lambda w: w * T, False),
    }


class Work:
    """Counts aten ops (a TorchDispatchMode) and learn_lib.call invocations while active."""

    def __init__(self, learn_lib):
        from torch.utils._python_dispatch import TorchDispatchMode
        self.ops, self.calls, self.lib = collections.Counter(), collections.Counter(), learn_lib
        work = self

        class Mode(TorchDispatchMode):
            def __torch_dispatch__(self, func, types, args=(), kwargs=None):
                work.ops[str(func)] += 1
                return func(*args, **(kwargs or {}))
        self.mode = Mode()

    def __enter__(self):
        self.orig = self.lib.call

        def call(name, *args):
            self.calls[name] += 1
            return self.orig(name, *args)
        self.lib.call = call
        self.mode.__enter__()
        return self

    def __exit__(self, *exc):
        self.mode.__exit__(*exc)
        self.lib.call = self.orig

    def summary(self, with_ops):
        out = dict(aten_ops=sum(self.ops.values()), learn_lib_calls=sum(self.calls.values()))
        out['total'] = out['aten_ops'] + out['learn_lib_calls']
        if with_ops:
            out['ops'], out['calls'] = dict(sorted(self.ops.items())), dict(sorted(self.calls.items()))
        return out


def run(name, args):
    import torch
    import mfg_amd.marl as M
    from mfg_amd import learn_lib
    from mfg_amd.factory import BatchedFactory
    make, steps, graphed = learners(M, lambda: torch.Generator(device='cuda').manual_seed(11))[name]
    torch.manual_seed(5)  # the network's initial weights and, without a generator, the sampling uniforms
    f = BatchedFactory('large8.yaml', args.batch, seed_base=3)
    tr = make(f)
    for _ in range(steps(args.windows)):
        tr.step()
    torch.cuda.synchronize()
    net = tr.net if hasattr(tr, 'net') else tr.nets
    params = {k: p.detach().cpu() for k, p in net.named_parameters()}
    h = hashlib.sha256()
    for k in sorted(params):
        h.update(k.encode())
        h.update(params[k].numpy().tobytes())
    h.update(tr.last_loss.detach().cpu().numpy().tobytes())
    res = dict(digest=h.hexdigest(), last_loss=[float(x) for x in tr.last_loss.detach().cpu().reshape(-1)],
               updates=int(tr.updates))
    if args.params:
        Path(args.params).mkdir(parents=True, exist_ok=True)
        torch.save(params, Path(args.params) / f'{name}.pt')
    if not graphed:  # one acting step, the rest of the window uncounted, then the learn call it leads to
        learn, tr.learn = tr.learn, (lambda: None)
        with Work(learn_lib) as act:
            tr.step()
        for _ in range(T - 1):
            tr.step()
        tr.learn = learn
        with Work(learn_lib) as upd:
            tr.learn()
        torch.cuda.synchronize()
        res['act'], res['update'] = act.summary(args.ops), upd.summary(args.ops)
    f.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--windows', type=int, default=3, help='learn calls before the digest (the graph learner: + 2)')
    ap.add_argument('--only', nargs='*', help='learner names (default: all)')
    ap.add_argument('--params', help='directory to save every learner\'s parameters to (torch.save)')
    ap.add_argument('--ops', action='store_true', help='list the counts per aten op and per kernel')
    args = ap.parse_args()
    import mfg_amd.marl as M
    names = args.only or list(learners(M, None))
    print(json.dumps({'batch': args.batch, 'windows': args.windows, 'learners': {n: run(n, args) for n in names}}))


if __name__ == '__main__':
    main()
