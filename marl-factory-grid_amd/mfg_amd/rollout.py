"""The loop around the engine that the on-device learners share (``BatchedA2C``, ``BatchedMAPPO``: mfg_amd/marl.py;
``BatchedIAC`` / ``BatchedSEAC``: mfg_amd/seac.py): the packed-obs slots and target buffers, the engine reset and step,
the next entry's inputs after a step, the learn call's checks and counters, the window slide, the re-projection of a
slot after an update, and the warm-up / capture / replay of a HIP graph.

The memory is aligned: slot k holds (o_k, a_{k-1}) as the network input and a_k, r_k, d_k as targets. After a done the
next entry's action input is -1 (padding) and its recurrent state zero, as the reference restarts both at every
``env.reset()`` (``base_ac.py:98-100``); the engine auto-resets. ``Rollout`` is the part every learner uses (MAPPO's
ring builds on it directly), ``WindowRollout`` adds the window of n_steps + 1 slots that slides by n_steps per update.
The policy forward, the sampling, the losses and the optimisers stay with the learners.
"""
import torch

from . import learn_lib


def _project_dense(idx, val, proj):
    """obs_proj over packed rows without grad: the rows scattered to dense blocks (<= 512 MiB) and one GEMM each
    (embedding_bag with per-sample weights ran 0.77 ms for C3's 65,536 rows on the MI355X)."""
    lead, cap = idx.shape[:-1], idx.shape[-1]
    idx2, val2 = idx.reshape(-1, cap).long(), val.reshape(-1, cap)
    k = proj.weight.shape[1]
    out = torch.empty((idx2.shape[0], proj.weight.shape[0]), dtype=proj.weight.dtype, device=idx2.device)
    step = max(1, (1 << 27) // max(k, 1))
    for r0 in range(0, idx2.shape[0], step):
        d = torch.zeros((min(step, idx2.shape[0] - r0), k), dtype=proj.weight.dtype, device=idx2.device)
        d.scatter_add_(1, idx2[r0:r0 + step], val2[r0:r0 + step].to(d.dtype))
        torch.addmm(proj.bias, d, proj.weight.t(), out=out[r0:r0 + step])
    return out.view(*lead, -1)


def graph_run(dev, body, graph, warm, before_capture=None):
    """body() as a HIP graph: eager on a side stream for the first two calls (lazy library state stays outside the
    capture), captured at the third, replayed from then on. graph / warm are the caller's state (None / 0 at first);
    returns them for the next call. before_capture() runs between the warm-ups and the capture."""
    if graph is not None:
        graph.replay()
        return graph, warm
    if warm < 2:
        cur = torch.cuda.current_stream(dev)
        side = torch.cuda.Stream(dev)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            body()
        cur.wait_stream(side)
        return None, warm + 1
    graph = torch.cuda.CUDAGraph()
    if before_capture is not None:
        before_capture()
    with torch.cuda.graph(graph):
        body()
    graph.replay()  # capture records only: this call's body runs here
    return graph, warm


class Rollout:
    """The state and the steps of acting on one engine. A learner calls ``__init__`` (the engine's sizes, the ``cap``
    refusal, the counters), builds its networks on ``kdim``, then ``_alloc`` (the buffers)."""

    def __init__(self, factory, cap, check_cap, generator):
        self.f = factory
        eng = factory.engine
        self.B, self.A = eng.B, eng.A
        self.N = self.B * self.A
        self.dev = eng.device
        self.kdim = eng.lmax * eng.obs_hw[0] * eng.obs_hw[1]
        if not check_cap and cap < self.kdim:
            # a truncated row would make acting (the fused emb sums every nonzero entry) and learning (the stored
            # cap entries only) see different obs_proj inputs: skipping the check is allowed only when no row
            # can be truncated
            raise ValueError(f'check_cap=False needs cap >= lmax*h*w = {self.kdim} (rows can hold up to that many '
                             f'nonzero entries); got cap {cap}')
        self.cap, self.check_cap, self.gen = cap, check_cap, generator
        self.updates = 0
        self.episodes = torch.zeros((), dtype=torch.float64, device=self.dev)  # finished episodes, per learn call
        self.reward_sum = torch.zeros((), dtype=torch.float64, device=self.dev)
        self._started = False

    def _alloc(self, n_obs, n_tgt, hidden, proj=None, agent_major=False):
        """n_obs obs slots (packed entries; with proj, an nn.Linear, also its projection fused into the render) and
        action inputs, n_tgt slots of actions, rewards and dones, and the recurrent states ha / hc of hidden = (actor,
        critic) sizes: [N, 1, H] in the engine's (env, agent) row order for a shared network, [A, B, H] agent-major for
        stacked per-agent networks."""
        from .engine import PackedObs
        B, A, dev = self.B, self.A, self.dev
        self._proj = proj
        w, b = (None, None) if proj is None else (proj.weight, proj.bias)
        self.pobs = PackedObs(self.f.engine, K=n_obs, cap=self.cap, weight=w, bias=b)  # written by the engine
        self.slot = [self.pobs.view(k) for k in range(n_obs)]
        self.act_in = torch.full((n_obs, B, A), -1, dtype=torch.int64, device=dev)  # a_{t-1}, -1 = none
        self.act = torch.zeros((n_tgt, B, A), dtype=torch.int32, device=dev)
        self.rew = torch.zeros((n_tgt, B, A), dtype=torch.float64, device=dev)
        self.done = torch.zeros((n_tgt, B), dtype=torch.uint8, device=dev)
        # persistent, updated in place (inputs of captured graphs); keep broadcasts a done env over its agents
        if agent_major:
            self.ha, self.hc = (torch.zeros((A, B, h), device=dev) for h in hidden)
            self._keep_shape, self._rows = (1, B, 1), lambda v: v
        else:
            self.ha, self.hc = (torch.zeros((self.N, 1, h), device=dev) for h in hidden)
            self._keep_shape, self._rows = (B, 1, 1), lambda v: v.view(B, A, -1)

    def reset(self, k=0):
        """All envs reset, o_0 rendered into slot k. The action input of that slot and the recurrent states stay as
        they are (BatchedMAPPO clears them)."""
        self.f.engine.reset(obs=self.slot[k], init=0 if self.f._created else 1, seed_base=self.f.seed_base)
        self.f._created = True
        self._started = True

    def _env_step(self, k, nxt, defer_replay):
        """The engine's step on the actions of slot k: reward and done into slot k, the next obs into slot nxt, and
        that entry's action input (-1 after an episode end). Returns done [B] (bool)."""
        self.f.engine.step(1, actions=self.act[k], reward=self.rew[k], done=self.done[k], obs=self.slot[nxt],
                           auto_reset=True, step_base=self.f.t, defer_replay=defer_replay)
        self.f.t += 1
        d = self.done[k].bool()
        a = self.act[k].long()
        self.act_in[nxt].copy_(torch.where(d.view(-1, 1), torch.full_like(a, -1), a))
        return d

    def _carry(self, d, ha_new, hc_new):
        """The next entry's recurrent states: the policy step's new ones (ha's layout), zero where the episode ended."""
        keep = (~d).to(self.ha.dtype).view(self._keep_shape)
        torch.mul(self._rows(ha_new), keep, out=self._rows(self.ha))
        torch.mul(self._rows(hc_new), keep, out=self._rows(self.hc))

    def _check(self, name, where):
        """With check_cap a learn call raises on truncated packed rows and on non-finite acting logits (one host sync
        each)."""
        if not self.check_cap:
            return
        self.pobs.check()
        if self.gen is None and self.dev.type == 'cuda' and bool((self.act < 0).any()):
            # mfg_sample_categorical marks rows with non-finite logits -1 (the engine took them as crash actions)
            raise RuntimeError(f'{name}: non-finite policy logits {where} (training diverged)')

    def _fold(self, slots=None):
        """The episode and reward counters, once per learn call over its target slots (default: all; two reductions
        instead of two per step)."""
        self.episodes += (self.done if slots is None else self.done[slots]).sum()
        self.reward_sum += (self.rew if slots is None else self.rew[slots]).sum()

    @torch.no_grad()
    def project_slot(self, k):
        """After an update: the engine projects with the new weights from now on, and slot k's fused projection (the
        engine rendered it with the old ones) is redone, one mfg_packed_project over its packed rows on the GPU."""
        pb = self.pobs
        pb.set_projection(self._proj.weight, self._proj.bias)
        if not pb.idx.is_cuda:
            pb.emb[k].copy_(_project_dense(pb.idx[k], pb.val[k], self._proj))
            return
        learn_lib.call('mfg_packed_project', pb.idx[k].data_ptr(), pb.val[k].data_ptr(), self.N, pb.cap,
                       pb.wt.data_ptr(), pb.bias.data_ptr(), pb.E, pb.kdim, pb.emb[k].data_ptr(), pb.E,
                       learn_lib.stream(self.dev))

    def train(self, n_steps):
        """n_steps env-steps (with the learn calls that fall into them); returns the last loss."""
        for _ in range(n_steps):
            self.step()
        return self.last_loss


class WindowRollout(Rollout):
    """A window of T = n_steps entries and the bootstrap entry T: slots 0..T, position t; ``learn`` at t == T, then the
    window slides (o_T becomes o_0, with the states h0a / h0c fed at entry 0). The engine's floor-shuffle replay is
    deferred to the window's last step (MFG_STEP_DEFER_REPLAY)."""

    def _alloc(self, hidden, proj=None, agent_major=False):
        super()._alloc(self.T + 1, self.T, hidden, proj, agent_major)
        self.h0a, self.h0c = self.ha.clone(), self.hc.clone()
        self.t = 0

    def reset(self):
        super().reset(0)
        self.t = 0

    def _window_step(self, ha_new, hc_new):
        """The env-step of window position t after its policy step, and the learn call at the window's end."""
        t = self.t
        self._carry(self._env_step(t, t + 1, defer_replay=t + 1 < self.T), ha_new, hc_new)
        self.t += 1
        if self.t == self.T:
            self.learn()

    def _slide(self):
        """Entry T becomes entry 0 (on static buffers: part of the body BatchedA2C captures)."""
        T, pb = self.T, self.pobs
        pb.idx[0].copy_(pb.idx[T])
        pb.val[0].copy_(pb.val[T])
        pb.count[0].copy_(pb.count[T])
        self.act_in[0].copy_(self.act_in[T])
        self.h0a.copy_(self.ha)
        self.h0c.copy_(self.hc)

    def train(self, n_updates):
        return super().train(n_updates * self.T)
