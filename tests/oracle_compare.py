"""The call-level comparison loop of tests/test_gpu_resume.py and tests/test_gpu_engine_calls.py (test helper).

One side is a batch of C-oracle envs stepped without interruption (`OracleBatch`), the other the rows an engine call
wrote: `compare_call` checks every env and step of a call (reward lists with ==, done, the event fields, f64 obs bit
for bit, the first observation of an auto-reset episode included), `check_state` the records after a call whose replay
has run (MT19937 state and index, floor order, PCG64 state, no debt left). Nothing here needs a GPU.
"""
import numpy as np

import oracle as O
from philox import synthetic_actions
from mfg_amd import abi
from mfg_amd.engine import EV_MISC, RecordView, events_from_rows

EV_FIELDS = ('door_coll', 'door_coll_hi', 'maint_coll', 'done_mask', 'step')


def max_steps(spec):
    """The episode length of the config's DoneAtMaxStepsReached rule."""
    for r in list(spec.c.rules)[:spec.c.n_rules]:
        if r.op == abi.RULE_DONE_MAXSTEPS:
            return int(r.i[0])
    raise AssertionError('the config has no DoneAtMaxStepsReached rule')


class OracleBatch:
    """Oracle envs of the global indices `ids`: env i is OracleEnv(spec, base + i), its actions at step t are the
    engine's Philox actions keyed (pseed, i) at counter t. Auto-reset like the engine's. No env may crash."""

    def __init__(self, spec, ids, base, pseed):
        self.spec, self.pseed = spec, pseed
        self.ids = np.asarray(ids, np.int64)
        self.envs = [O.OracleEnv(spec, base + int(i)) for i in self.ids]
        self.t = 0
        self.ended = np.zeros(len(self.ids), np.int64)  # episode ends seen by step()
        self.dirt_rises = 0  # steps of step() after which an env held more dirt piles than before

    def close(self):
        for e in self.envs:
            e.close()

    def reset(self, odd_only=False):
        """mfg_reset on every env (odd_only: on the envs of odd index, the staggering mask); the obs of every env."""
        return [e.reset() if (i % 2 or not odd_only) else e.obs_list() for i, e in zip(self.ids, self.envs)]

    def odd_mask(self):
        return (self.ids % 2).astype(np.uint8)

    def run(self, n, auto_reset=True):
        """n steps without obs; returns the done flags of the last one."""
        done = np.zeros(len(self.ids), bool)
        for _ in range(n):
            acts = synthetic_actions(self.pseed, self.ids, self.t, self.spec.n_actions)
            for j, e in enumerate(self.envs):
                _, done[j], ev = e.step(acts[j], with_obs=False)
                assert not ev.crashed, f'oracle env {self.ids[j]} crashed at step {self.t}'
                if done[j] and auto_reset:
                    e.reset()
            self.t += 1
        return done

    def step(self):
        """One step with auto-reset: per env (reward, done, event fields, obs after the step or of the new episode)."""
        A, out = self.spec.n_agents, []
        acts = synthetic_actions(self.pseed, self.ids, self.t, self.spec.n_actions)
        dirt = bool(self.spec.c.has_dirt)
        for j, e in enumerate(self.envs):
            n0 = len(e.group(3)) if dirt else 0
            r, d, ev = e.step(acts[j])
            assert not ev.crashed, f'oracle env {self.ids[j]} crashed at step {self.t}'
            fields = {k: getattr(ev, k) for k in EV_FIELDS}
            fields['act'], fields['watch'] = list(ev.act[:A]), list(ev.watch[:A])
            self.dirt_rises += bool(dirt and len(e.group(3)) > n0)
            self.ended[j] += d
            out.append((r, d, fields, e.reset() if d else e.obs_list()))
        self.t += 1
        return out


def make_buffers(torch, eng, K):
    """The output buffers of a K-step call, obs in f64 (the reference's precision)."""
    B, A, dev = eng.B, eng.A, eng.device
    return dict(obs=torch.zeros((K,) + eng.obs_shape(), dtype=torch.float64, device=dev),
                reward=torch.zeros((K, B, A), dtype=torch.float64, device=dev),
                done=torch.zeros((K, B), dtype=torch.uint8, device=dev),
                ev_act=torch.zeros((K, B, A), dtype=torch.uint8, device=dev),
                ev_watch=torch.zeros((K, B, A), dtype=torch.uint8, device=dev),
                ev_misc=torch.zeros((K, B, EV_MISC), dtype=torch.int32, device=dev))


def rows_of(buf, K):
    """The first K rows of every buffer as numpy arrays (copies on the current stream, which they wait for)."""
    return {k: v[:K].cpu().numpy() for k, v in buf.items()}


def compare_obs(tag, spec, got, want):
    """One env's obs [A, lmax, h, w] against the oracle's per-agent list, as f64 bit patterns."""
    for a, n in enumerate(spec.n_layers):
        g, w = np.ascontiguousarray(got[a, :n]), np.ascontiguousarray(want[a])
        if not (g.view(np.uint64) == w.view(np.uint64)).all():
            dif = np.argwhere(g.view(np.uint64) != w.view(np.uint64))
            raise AssertionError(f'{tag} agent {a} obs: {len(dif)} diffs, first '
                                 f'{[(tuple(x), g[tuple(x)], w[tuple(x)]) for x in dif[:4]]}')


def compare_call(tag, ob, rows, K):
    """The K steps of one engine call (`rows`: numpy [K, n, ...] per output, env j of the batch in row j) against the
    next K steps of the oracle batch `ob`."""
    spec = ob.spec
    for k in range(K):
        t = ob.t
        for j, (r, d, want, ro) in enumerate(ob.step()):
            at = f'{tag} step {t} env {ob.ids[j]}'
            assert list(rows['reward'][k, j]) == list(r), f"{at} reward {rows['reward'][k, j]} vs {r}"
            assert bool(rows['done'][k, j]) == d, f'{at} done'
            ev = events_from_rows(rows['ev_act'][k, j], rows['ev_watch'][k, j], rows['ev_misc'][k, j])
            assert not ev['crashed'], f'{at} crashed'
            for f in ('act', 'watch') + EV_FIELDS:
                assert ev[f] == want[f], f'{at} events {f}: {ev[f]} vs {want[f]}'
            compare_obs(at, spec, rows['obs'][k, j], ro)


def state_errors(state, layout, ob):
    """What differs between the records `state` (numpy [n, size], the replay has run) and the oracle envs' RNG state:
    a list of messages, empty when MT19937 state and index, floor order and PCG64 state are equal and no debt is left."""
    bad = []
    for j, env in enumerate(ob.envs):
        rv = RecordView(state[j], layout, ob.spec)
        mt = env.mt_state()
        if not np.array_equal(rv.mt(), mt):
            bad.append(f'env {ob.ids[j]} MT state')
        if rv.hdr('mt_idx') != int(mt[624]):
            bad.append(f'env {ob.ids[j]} mt_idx')
        if not np.array_equal(rv.perm(), env.floor()):
            bad.append(f'env {ob.ids[j]} floor order')
        if not np.array_equal(rv.pcg(), env.pcg_state()):
            bad.append(f'env {ob.ids[j]} PCG state')
        if rv.hdr('debt') != 0:
            bad.append(f"env {ob.ids[j]} debt {rv.hdr('debt')}")
    return bad


def check_state(tag, state, layout, ob):
    bad = state_errors(state, layout, ob)
    assert not bad, f'{tag}: ' + '; '.join(bad[:8])
