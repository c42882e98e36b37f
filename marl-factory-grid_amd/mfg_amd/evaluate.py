"""Evaluation of a trained policy over the batched engine, and loading of reference checkpoints (re-exported by
mfg_amd.marl).

Reference anchors:
  * ``algorithms/marl/base_ac.py:152-183`` ``BaseActorCritic.eval_loop``: per episode, act with
    ``Categorical(logits).sample()`` on (obs, last action, recurrent state) until the env is done, summing the rewards
    per agent in f32 (``eps_rew = torch.zeros(n_agents)``, ``eps_rew += torch.tensor(reward)``); one result row per
    episode (the agents' sums, then Python's ``sum`` over that tensor: a left-to-right f32 chain), melted into a frame
    with the columns ``episode``, ``agent``, ``reward``;
  * ``snac.py:12-15`` / ``iac.py:22-25`` ``load_state_dict``: a checkpoint directory as ``Checkpointer.save_experiment``
    writes it (``algorithms/utils.py:73-77``): one ``state_dict`` per ``*.pt``.

``BatchedEvaluator`` runs that loop for B envs at once: every env plays ``n_episodes`` episodes (the engine auto-resets;
after a done the next step's action input is -1 and the recurrent state zero, as at every ``env.reset()`` of the
reference loop). Evaluation needs the actor only: no critic GRU, no stored activations, no window. On the GPU a fused
step is one ``mfg_policy_act`` (the whole actor and the sampling as one kernel, include/mfg_learn.h), one ``engine.step``
and one ``mfg_eval_fold``; the host reads one integer every ``poll_every`` steps. Which acting path is the default
follows the measurement.
"""
import ctypes
import re
from pathlib import Path

import torch

from . import learn_lib
from .action_mask import masked_logits
from .marl import RecurrentAC
from .seac import AgentNets

_act_lib = learn_lib.lib  # the former binder's name, for callers written against it

# mfg_policy_act's size limits (include/mfg_learn.h)
ACT_MAX_E, ACT_MAX_AE, ACT_MAX_H, ACT_MAX_ACT = 128, 32, 128, 32


def _weights_struct(w):
    """mfg_actor_weights of an ``actor_weights`` dict, built once per dict."""
    if '_struct' not in w:
        w['_struct'] = learn_lib.ActorWeights(**{k: w[k].data_ptr() for k in learn_lib.ACTOR_FIELDS})
    return w['_struct']


def _resolve(policy):
    """(networks, shared): a RecurrentAC (shared) or an AgentNets, given directly or as a learner's .net / .nets."""
    if not isinstance(policy, (RecurrentAC, AgentNets)):
        inner = getattr(policy, 'nets', None)
        policy = inner if inner is not None else getattr(policy, 'net', None)
    if isinstance(policy, AgentNets):
        return policy, False
    if isinstance(policy, RecurrentAC):
        return policy, True
    raise TypeError('policy must be a RecurrentAC, an AgentNets, or a learner holding one as .net / .nets')


def actor_weights(policy):
    """The actor's parameters as mfg_policy_act reads them (mfg_actor_weights): stacked over the g networks, every
    matrix K-major [g, in, out], contiguous f32 copies on the parameters' device."""
    net, shared = _resolve(policy)
    if shared:
        sd = {k: v.detach()[None] for k, v in net.state_dict().items()}
    else:
        sd = {k: v.detach() for k, v in net.P.items()}

    def t(k):
        return sd[k].float().transpose(1, 2).contiguous()

    def c(k):
        return sd[k].float().contiguous()

    return dict(action_emb=c('action_emb.weight'), w1t=t('mix.1.weight'), b1=c('mix.1.bias'), w3t=t('mix.3.weight'),
                b3=c('mix.3.bias'), wiht=t('gru_actor.weight_ih_l0'), bih=c('gru_actor.bias_ih_l0'),
                whht=t('gru_actor.weight_hh_l0'), bhh=c('gru_actor.bias_hh_l0'), wat=t('action_head.0.weight'),
                ba=c('action_head.0.bias'), wbt=t('action_head.2.weight'), bb=c('action_head.2.bias'))


def act_supported(e_dim, ae_dim, hd, n_max):
    """Sizes mfg_policy_act covers (it returns -1 and launches nothing outside them)."""
    return 1 <= e_dim <= ACT_MAX_E and 1 <= ae_dim <= ACT_MAX_AE and 1 <= hd <= ACT_MAX_H and 1 <= n_max <= ACT_MAX_ACT


def policy_act(w, emb, emb_strides, n_envs, n_agents, n_act, prev_action, prev_done, h, h_strides, u, act_out,
               logits_out=None, greedy=False, check=False, mask=None):
    """One ``mfg_policy_act`` call on the current stream. w: ``actor_weights``; emb / h: f32 device tensors read at
    env * strides[0] + agent * strides[1] (elements); n_act i32 [g] on the device; prev_action / prev_done None: an
    episode start. mask: the action-mask words, int32 [n_envs, n_agents] on the device (``Engine.action_mask``): the
    call is ``mfg_policy_act_masked`` and an action whose bit is clear is never picked. Returns the kernel's return code
    (-1: sizes outside its limits, nothing launched), or with ``check`` raises on it."""
    g, k_in, e_dim = w['w1t'].shape
    hd, n_max = w['wbt'].shape[1:]
    ptr = learn_lib.ptr
    args = (emb.data_ptr(), emb_strides[0], emb_strides[1], n_envs, n_agents, g, e_dim, k_in - e_dim, hd, n_max,
            ctypes.byref(_weights_struct(w)), n_act.data_ptr(), ptr(prev_action), ptr(prev_done), h.data_ptr(),
            h_strides[0], h_strides[1], ptr(u), 1 if greedy else 0)
    name = 'mfg_policy_act'
    if mask is not None:
        if mask.dtype != torch.int32 or mask.numel() != n_envs * n_agents or not mask.is_contiguous():
            raise ValueError(f'mask must be a contiguous int32 tensor [{n_envs}, {n_agents}]')
        name, args = 'mfg_policy_act_masked', args + (mask.data_ptr(),)
    args += (act_out.data_ptr(), ptr(logits_out), learn_lib.stream(emb.device))
    if check:
        return learn_lib.call(name, *args)
    return getattr(learn_lib.lib(), name)(*args)


# ---------------------------------------------------------------------------------------------------------------------
# the same formulas in tensor code
# ---------------------------------------------------------------------------------------------------------------------
def actor_step(policy, emb, a_in, h):
    """One acting step in tensor code, the actor of ``forward_emb`` with T = 1. Shared network: emb [N, E], a_in [N]
    (long, -1 = none), h [N, H] -> (logits [N, n_act], h' [N, H]), the very layer calls of ``RecurrentAC.forward_emb``.
    ``AgentNets``: emb [A, B, E], a_in [A, B], h [A, B, H] -> (logits [A, B, n_max], h' [A, B, H]) through
    ``AgentNets.forward_emb`` (its critic runs on a zero state and is dropped)."""
    net, shared = _resolve(policy)
    if shared:
        if net.use_agent_embedding:
            raise ValueError('actor_step: the agent embedding needs forward_emb (agent ids)')
        mixed = net.mixed(emb[:, None], a_in[:, None])
        g = net.gru_actor
        hn = torch.gru_cell(mixed[:, 0], h, g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0)
        return net.action_head(hn), hn
    hc = torch.zeros(h.shape[:2] + (net.hidden_size_critic,), dtype=h.dtype, device=h.device)
    out = net.forward_emb(emb[:, :, None], a_in[:, :, None], h, hc)
    return out['logits'][:, :, 0], out['hidden_actor'][:, :, 0]


def sample_inversion(logits, u, n_act=None, mask=None):
    """``mfg_sample_categorical`` in tensor code: the action whose CDF bin holds u * sum(exp(l - max)) over the first
    n_act columns (all by default); the last action when rounding passes the last bin; -1 for non-finite logits.
    mask: action-mask words, int32 of u's shape: a logit whose bit is clear counts as -inf; a row whose word has no
    bit set among its columns is sampled unmasked (``mfg_policy_act_masked``'s rule)."""
    lg = logits if n_act is None else logits[..., :n_act]
    if mask is not None:
        lg = masked_logits(lg, mask)
    ex = torch.exp(lg - lg.max(-1, keepdim=True).values)
    cdf = torch.cumsum(ex, -1)
    s = cdf[..., -1]
    pick = (u[..., None] * s[..., None] >= cdf).sum(-1).clamp(max=lg.shape[-1] - 1)
    bad = ~(s > 0) | torch.isinf(s)
    return torch.where(bad, torch.full_like(pick, -1), pick).to(torch.int32)


def eval_fold(reward, done, n_episodes, eps_rew, length, count, rows, lengths, finished):
    """``mfg_eval_fold`` in tensor code (no host sync): reward [B, A] (f64), done [B]; the state tensors eps_rew f32
    [B, A], length / count i32 [B], rows f32 [B, n_episodes, A + 1], lengths i32 [B, n_episodes] and finished i32 []
    are updated in place."""
    B, A = eps_rew.shape
    eps_rew += reward.to(torch.float32)
    length += 1
    d = done.bool()
    store = d & (count < n_episodes)
    s = torch.zeros(B, dtype=torch.float32, device=eps_rew.device)
    for i in range(A):  # Python's sum over the tensor: a left-to-right chain, no tree
        s = s + eps_rew[:, i]
    k = count.clamp(max=n_episodes - 1).long()
    b = torch.arange(B, device=eps_rew.device)
    new = torch.cat([eps_rew, s[:, None]], 1)
    rows[b, k] = torch.where(store[:, None], new, rows[b, k])
    lengths[b, k] = torch.where(store, length, lengths[b, k])
    count += store.to(count.dtype)
    finished += (store & (count == n_episodes)).sum().to(finished.dtype)
    eps_rew.masked_fill_(d[:, None], 0.0)
    length.masked_fill_(d, 0)


# ---------------------------------------------------------------------------------------------------------------------
# the evaluator
# ---------------------------------------------------------------------------------------------------------------------
class BatchedEvaluator:
    """``eval_loop`` (base_ac.py:152-183) over the B envs x A agents of one engine: every env plays ``n_episodes``
    episodes with the policy, everything on the device.

    policy: a ``RecurrentAC`` (shared, ``LoopSNAC``), an ``AgentNets`` (one network per agent, ``LoopIAC``), or a learner
    (its ``.net`` / ``.nets``). The weights are read at construction; ``refresh()`` re-reads them.
    fused: on the GPU a step's acting is one ``mfg_policy_act``; ``fused=False``, any CPU device, a network with the agent
    embedding and layer sizes over the kernel's limits run the same formulas in tensor code (``actor_step``,
    ``sample_inversion`` / ``mfg_sample_categorical``, ``eval_fold``). None takes the path whose loop measured faster
    on the MI355X (profiles/eval.json): the kernel for per-agent networks, the tensor path for a shared network.
    greedy: argmax instead of sampling. generator: draws the sampling uniforms (default: the device's global one).
    record: keep every step's actions, rewards and dones (``actions`` [steps, B, A] i32, ``rewards`` f64, ``dones``
    [steps, B] u8 after ``run``). poll_every: steps between two reads of the finished-env counter (the only host sync).
    mask_invalid: every step takes the engine's action mask (``Engine.action_mask``, one more kernel) and acts masked, on
    both paths: an action that would be invalid if the agent acted first is never picked, unless none of the agent's
    actions is valid (a crashed env, a paralysed agent), which acts unmasked.

    After ``run``: ``rows`` f32 [B, n_episodes, A + 1] (per episode the agents' reward sums, then their f32 sum),
    ``lengths`` i32 [B, n_episodes], ``steps``; ``frame(env=b)`` is the reference's melted frame of env b."""

    def __init__(self, factory, policy, n_episodes, fused=None, greedy=False, generator=None, record=False,
                 poll_every=None, cap=32, check_cap=True, mask_invalid=False):
        from .engine import PackedObs
        self.f = factory
        eng = factory.engine
        self.B, self.A = eng.B, eng.A
        self.N = self.B * self.A
        self.dev = torch.device(eng.device)
        self.n_episodes = int(n_episodes)
        if self.n_episodes < 1:
            raise ValueError('n_episodes must be at least 1')
        self.net, self.shared = _resolve(policy)
        self.net.to(self.dev)
        net = self.net
        spec_n = [int(x) for x in factory.spec.n_actions]
        self.n_act = [int(net.n_actions)] * self.A if self.shared else list(net.n_act)
        if self.n_act != spec_n:
            raise ValueError(f'the policy\'s action counts {self.n_act} differ from the spec\'s {spec_n}')
        if not self.shared and net.A != self.A:
            raise ValueError(f'{net.A} networks for {self.A} agents')
        self.n_max = max(self.n_act)
        self.E = net.obs_proj.weight.shape[0] if self.shared else net.obs_emb_size
        self.H = net.hidden_size_actor
        self.greedy, self.gen, self.record = bool(greedy), generator, bool(record)
        self.mask_invalid = bool(mask_invalid)
        self.mask = torch.zeros((self.B, self.A), dtype=torch.int32, device=self.dev) if self.mask_invalid else None
        self.poll_every = max(1, int(poll_every)) if poll_every is not None else 16
        if fused is None:  # measured (profiles/eval.json): fused 1.25-1.44x with AgentNets, 0.88-1.04x with a shared net
            fused = not self.shared
        self.fused = (bool(fused) and self.dev.type == 'cuda' and not net.use_agent_embedding
                      and act_supported(self.E, net.action_emb_size, self.H, self.n_max))
        B, A, dev = self.B, self.A, self.dev
        kdim = eng.lmax * eng.obs_hw[0] * eng.obs_hw[1]
        # the obs slot: packed rows, plus the render's fused obs_proj for a shared network (per-agent networks project
        # the stored entries themselves, so a truncated row matters there: check_cap)
        if self.shared:
            self.pobs = PackedObs(eng, K=1, cap=cap, weight=net.obs_proj.weight, bias=net.obs_proj.bias)
        else:
            if not check_cap and cap < kdim:
                raise ValueError(f'check_cap=False needs cap >= lmax*h*w = {kdim}; got cap {cap}')
            self.pobs = PackedObs(eng, K=1, cap=cap)
            self._emb = torch.zeros((A, B, self.E), device=dev)  # agent-major, mfg_packed_project_grouped's output
        self.check_cap = bool(check_cap) and not self.shared
        self._cmax = torch.zeros((), dtype=torch.int32, device=dev)
        self.act = torch.zeros((B, A), dtype=torch.int32, device=dev)
        self.rew = torch.zeros((B, A), dtype=torch.float64, device=dev)
        self.done = torch.zeros(B, dtype=torch.uint8, device=dev)
        # the recurrent state: engine order [B, A, H] for a shared network, agent-major [A, B, H] for AgentNets
        self.h = torch.zeros((B, A, self.H) if self.shared else (A, B, self.H), device=dev)
        self._u = torch.zeros((B, A), device=dev)
        self.n_act_dev = torch.tensor(self.n_act[:1] if self.shared else self.n_act, dtype=torch.int32, device=dev)
        self.eps_rew = torch.zeros((B, A), dtype=torch.float32, device=dev)
        self.len = torch.zeros(B, dtype=torch.int32, device=dev)
        self.count = torch.zeros(B, dtype=torch.int32, device=dev)
        self.rows = torch.zeros((B, self.n_episodes, A + 1), dtype=torch.float32, device=dev)
        self.lengths = torch.zeros((B, self.n_episodes), dtype=torch.int32, device=dev)
        self.finished = torch.zeros((), dtype=torch.int32, device=dev)
        self.first_logits = None  # the first acting step's logits [B, A, n_max] (engine order), kept by run()
        self.steps = 0
        self.actions = self.rewards = self.dones = None
        self.refresh()

    def refresh(self):
        """Re-read the policy's weights (after training or loading a checkpoint)."""
        if self.fused:
            self.w = actor_weights(self.net)
        if self.shared:
            self.pobs.set_projection(self.net.obs_proj.weight, self.net.obs_proj.bias)
        else:
            P = self.net.P
            self._wt = P['obs_proj.weight'].detach().transpose(1, 2).contiguous()  # [A, k, E]
            self._pb = P['obs_proj.bias'].detach().contiguous()

    # ---- acting ----
    def _project(self):
        """AgentNets: obs_proj of the slot's packed rows by every agent's own weights -> _emb [A, B, E]."""
        idx, val = self.pobs.idx[0], self.pobs.val[0]
        if self.dev.type == 'cuda':
            learn_lib.call('mfg_packed_project_grouped', idx.data_ptr(), val.data_ptr(), self.N, self.pobs.cap, self.A,
                           self._wt.data_ptr(), self._pb.data_ptr(), self.E, self._wt.shape[1], 0, self._emb.data_ptr(),
                           self.E, learn_lib.stream(self.dev))
        else:
            self._emb.copy_(self.net.project(self.pobs.idx, self.pobs.val)[:, :, 0])
        if self.check_cap:
            torch.maximum(self._cmax, self.pobs.count.max(), out=self._cmax)

    def _uniforms(self):
        if self.greedy:
            return None
        return self._u.uniform_(generator=self.gen)

    @torch.no_grad()
    def _act(self, first, logits_out=None):
        """The policy's actions for the obs in the slot into ``act`` [B, A]; first: an episode start for every env."""
        B, A = self.B, self.A
        if not self.shared:
            self._project()
        u = self._uniforms()
        mask = self.f.engine.action_mask(out=self.mask) if self.mask_invalid else None
        if self.fused:
            if self.shared:
                emb, es, hs = self.pobs.emb, (A * self.E, self.E), (A * self.H, self.H)
            else:
                emb, es, hs = self._emb, (self.E, B * self.E), (self.H, B * self.H)
            policy_act(self.w, emb, es, B, A, self.n_act_dev, None if first else self.act,
                       None if first else self.done, self.h, hs, u, self.act, logits_out, self.greedy, check=True,
                       mask=mask)
            return
        keep = torch.zeros(B, dtype=torch.bool, device=self.dev) if first else ~self.done.bool()
        a_in = torch.where(keep[:, None], self.act.long(), torch.full_like(self.act, -1, dtype=torch.long))
        if self.shared:
            h = self.h * keep.view(B, 1, 1).to(self.h.dtype)
            if self.net.use_agent_embedding:
                ids = torch.arange(A, device=self.dev).repeat(B)
                out = self.net.forward_emb(self.pobs.emb[0].view(self.N, 1, -1), a_in.view(self.N, 1),
                                           h.view(self.N, 1, -1),
                                           torch.zeros((self.N, 1, self.net.hidden_size_critic), device=self.dev),
                                           agent_ids=ids)
                logits, hn = out['logits'][:, 0], out['hidden_actor'][:, 0]
            else:
                logits, hn = actor_step(self.net, self.pobs.emb[0].view(self.N, -1), a_in.view(-1), h.view(self.N, -1))
            self.h.copy_(hn.view(B, A, -1))
            logits = logits.view(B, A, -1)
        else:
            h = self.h * keep.view(1, B, 1).to(self.h.dtype)
            logits, hn = actor_step(self.net, self._emb, a_in.t(), h)
            self.h.copy_(hn)
            logits = logits.transpose(0, 1)  # [B, A, n_max]
        if logits_out is not None:
            logits_out[..., :logits.shape[-1]].copy_(logits)
        self._pick(logits.contiguous(), u, mask)

    def _pick(self, logits, u, mask=None):
        """Actions from logits [B, A, n] (engine order) into ``act``; mask: action-mask words [B, A] or None."""
        uniform = len(set(self.n_act)) == 1
        groups = [(0, self.A, self.n_act[0])] if uniform else [(i, i + 1, c) for i, c in enumerate(self.n_act)]
        if mask is not None:  # the raw logits decide whether a row is a distribution; the filled ones, what is picked
            raw, logits = logits, logits.clone()
            for lo, hi, n in groups:
                logits[:, lo:hi, :n] = masked_logits(raw[:, lo:hi, :n], mask[:, lo:hi])
        if self.greedy:
            for lo, hi, n in groups:
                lg = logits[:, lo:hi, :n]
                a = lg.argmax(-1).to(torch.int32)
                ok = torch.isfinite(lg if mask is None else raw[:, lo:hi, :n]).all(-1)
                self.act[:, lo:hi] = torch.where(ok, a, torch.full_like(a, -1))
            return
        if logits.is_cuda and uniform:
            learn_lib.call('mfg_sample_categorical', logits.data_ptr(), logits.shape[-1], self.n_act[0], u.data_ptr(),
                           self.N, self.act.data_ptr(), learn_lib.stream(self.dev))
            return
        for lo, hi, n in ([(0, self.A, self.n_act[0])] if uniform else [(i, i + 1, c) for i, c in enumerate(self.n_act)]):
            self.act[:, lo:hi] = sample_inversion(logits[:, lo:hi], u[:, lo:hi], n)

    # ---- the fold ----
    def _fold(self):
        if self.dev.type == 'cuda':
            learn_lib.call('mfg_eval_fold', self.rew.data_ptr(), self.done.data_ptr(), self.B, self.A, self.n_episodes,
                           self.eps_rew.data_ptr(), self.len.data_ptr(), self.count.data_ptr(), self.rows.data_ptr(),
                           self.lengths.data_ptr(), self.finished.data_ptr(), learn_lib.stream(self.dev))
        else:
            eval_fold(self.rew, self.done, self.n_episodes, self.eps_rew, self.len, self.count, self.rows, self.lengths,
                      self.finished)

    # ---- the loop ----
    def reset(self):
        """Clear the results and the recurrent state and reset every env into the obs slot (``run`` starts with it)."""
        for t in (self.eps_rew, self.len, self.count, self.rows, self.lengths, self.finished, self.h, self._cmax):
            t.zero_()
        self.first_logits = None
        self.steps = 0
        self.f.engine.reset(obs=self.pobs, init=0 if self.f._created else 1, seed_base=self.f.seed_base)
        self.f._created = True

    @torch.no_grad()
    def step(self, actions=None, first=False):
        """One env-step of every env after ``reset``: the policy's actions (or ``actions`` i32 [B, A] on the device), the
        engine step into the obs slot and the fold; no host sync. first: every env is at an episode start (the step
        after ``reset``; its logits are kept as ``first_logits``). Returns the actions taken."""
        if actions is None:
            lg = None
            if first:
                lg = self.first_logits = torch.zeros((self.B, self.A, self.n_max), device=self.dev)
            self._act(first, lg)
            actions = self.act
        self.f.engine.step(1, actions=actions, reward=self.rew, done=self.done, obs=self.pobs, auto_reset=True,
                           step_base=self.f.t)
        self.f.t += 1
        self._fold()
        return actions

    @torch.no_grad()
    def run(self, actions=None, max_steps=None):
        """Reset every env and step until each has ``n_episodes`` episodes (or ``max_steps`` steps). actions: an int
        tensor [steps, B, A] replayed in place of the policy (the run ends with it at the latest). Returns ``rows``."""
        self.reset()
        if actions is not None:
            actions = torch.as_tensor(actions).to(device=self.dev, dtype=torch.int32).contiguous()
            if actions.dim() != 3 or tuple(actions.shape[1:]) != (self.B, self.A):
                raise ValueError(f'actions must be [steps, {self.B}, {self.A}]')
            limit = actions.shape[0] if max_steps is None else min(actions.shape[0], int(max_steps))
        else:
            limit = None if max_steps is None else int(max_steps)
        rec = ([], [], []) if self.record else None
        k = 0
        while limit is None or k < limit:
            act = self.step(None if actions is None else actions[k], first=k == 0)
            if rec is not None:
                for lst, t in zip(rec, (act, self.rew, self.done)):
                    lst.append(t.clone())
            k += 1
            if k % self.poll_every == 0 and int(self.finished) >= self.B:
                break
        self.steps = k
        if rec is not None and k:
            self.actions, self.rewards, self.dones = (torch.stack(x) for x in rec)
        if self.check_cap and int(self._cmax) > self.pobs.cap:
            raise RuntimeError(f'packed obs row has {int(self._cmax)} nonzero entries > cap {self.pobs.cap}')
        return self.rows

    def complete(self):
        """Whether every env has its ``n_episodes`` rows (one sync)."""
        return int(self.finished) >= self.B

    # ---- results ----
    def frame(self, env=None):
        """The reference's result frame (base_ac.py:179-183): ``pd.melt`` of one row per episode into the columns
        ``episode``, ``agent`` (``agent#i``, then ``sum``), ``reward``. env=b: env b alone, exactly the reference's
        frame; None: all envs, with a leading ``env`` column."""
        import pandas as pd
        agent_columns = [f'agent#{i}' for i in range(self.A)]
        rows, count = self.rows.cpu(), self.count.cpu()
        if env is not None:
            res = [rows[env, e].tolist() + [e] for e in range(int(count[env]))]
            res = pd.DataFrame(res, columns=agent_columns + ['sum', 'episode'])
            return pd.melt(res, id_vars=['episode'], value_vars=agent_columns + ['sum'], value_name='reward',
                           var_name='agent')
        res = pd.DataFrame(rows.reshape(-1, self.A + 1).double().numpy(), columns=agent_columns + ['sum'])
        res.insert(0, 'episode', torch.arange(self.n_episodes).repeat(self.B).numpy())
        res.insert(0, 'env', torch.arange(self.B).repeat_interleave(self.n_episodes).numpy())
        res = res[(res['episode'].to_numpy() < count.repeat_interleave(self.n_episodes).numpy())]
        return pd.melt(res, id_vars=['env', 'episode'], value_vars=agent_columns + ['sum'], value_name='reward',
                       var_name='agent')


# ---------------------------------------------------------------------------------------------------------------------
# reference checkpoints
# ---------------------------------------------------------------------------------------------------------------------
def natural_key(name):
    """Sort key that orders digit runs by value: ``agent#2`` before ``agent#10`` (what natsort does for the reference,
    iac.py:23)."""
    return [(0, int(p), '') if p.isdigit() else (1, 0, p.lower()) for p in re.split(r'(\d+)', str(name)) if p != '']


def load_reference_checkpoint(policy, path):
    """Load a checkpoint directory written by the reference (``Checkpointer.save_experiment``: one ``state_dict`` per
    ``*.pt``) into a ``RecurrentAC`` (exactly one file, snac.py:13-14), an ``AgentNets`` (the files in natural order,
    zipped with the networks, iac.py:23-25) or a learner's networks. Returns the files read."""
    net, shared = _resolve(policy)
    files = sorted(Path(path).glob('*.pt'), key=lambda p: natural_key(p.name))
    if shared:
        if len(files) != 1:
            raise ValueError(f'Expected a single set of weights but got {len(files)}')
        net.load_state_dict(torch.load(files[0], map_location='cpu'))
        return files
    dicts = net.state_dicts()
    files = files[:len(dicts)]
    for g, f in enumerate(files):
        dicts[g] = torch.load(f, map_location='cpu')
    net.load_state_dicts(dicts)
    return files
