"""Independent and shared-experience actor-critic on per-agent networks (re-exported by mfg_amd.marl).

Reference anchors:
  * ``algorithms/marl/iac.py`` ``LoopIAC``: one ``RecurrentAC`` and one RMSprop(3e-4, eps 1e-5) per agent, each trained
    on its own agent's window with ``BaseActorCritic.actor_critic`` (``base_ac.py:200-217``) and
    ``clip_grad_norm_(0.5)`` over its own parameters (``iac.py:50-57``);
  * ``algorithms/marl/seac.py`` ``LoopSEAC``: the same networks, each evaluated on every agent's window; the other
    agents' elements enter the policy and value terms with the importance weight pi_j(a) / pi_i(a), a constant
    (``seac.py:12-47``); the entropy runs over the network's own agent only (``seac.py:29``).

``AgentNets`` holds the A networks with their parameters stacked on a leading agent axis, so every layer is one
``baddbmm`` over agents. Activations are agent-major ``[A, rows, T, ...]``: one network's rows are contiguous. The
engine's order is ``[B][A]``; the transposition happens in ``mfg_packed_project_grouped`` (include/mfg_learn.h) and in
one small copy of the sampled actions back to the engine's ``[B][A]`` buffer. ``BatchedIAC`` / ``BatchedSEAC`` take
``BatchedA2C``'s loop unchanged, from the same core (mfg_amd/rollout.py: window alignment, restarts after a done,
auto-reset, deferred replay, ``check_cap``, the ``episodes`` / ``reward_sum`` counters); the learner recomputes the window
with grad.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.distributions import Categorical

from . import gru_window, learn_lib
from .gru_window import blin as _blin  # per-agent x W^T + b, the layers' GEMM (and the grouped GRU step's)
from .marl import RecurrentAC, compute_advantages, nonfinite_to_nan
from .rollout import WindowRollout

_seac_lib = learn_lib.lib  # the former binder's name, for callers written against it

_PAD_KEYS = ('action_emb.weight', 'action_head.2.weight', 'action_head.2.bias')  # rows follow the action count


def seac_ws_bytes(n_agents):
    """MFG_SEAC_WS_BYTES(g) (include/mfg_learn.h)."""
    return 4096 * n_agents


# ---------------------------------------------------------------------------------------------------------------------
# obs_proj of packed rows by per-agent weights
# ---------------------------------------------------------------------------------------------------------------------
def _dense_rows(idx, val, k):
    """Packed rows [M, cap] as dense f32 rows [M, k] (mfg_packed_densify on the GPU, scatter_add otherwise)."""
    m, cap = idx.shape
    if val.is_cuda and idx.dtype == torch.uint16 and k <= 4096:
        d = torch.empty((m, k), dtype=torch.float32, device=val.device)
        learn_lib.call('mfg_packed_densify', idx.data_ptr(), val.data_ptr(), m, cap, k, d.data_ptr(), k,
                       learn_lib.stream(val.device))
        return d
    d = torch.zeros((m, k), dtype=torch.float32, device=val.device)
    ix = idx.view(torch.int16).long() & 0xFFFF if idx.dtype == torch.uint16 else idx.long()
    return d.scatter_add_(1, ix, val)


def _agent_major(t):
    """[S, B, A, cap] -> contiguous [A, B, S, cap] (uint16 through its int16 bit view)."""
    if t.dtype == torch.uint16:
        return t.view(torch.int16).permute(2, 1, 0, 3).contiguous().view(torch.uint16)
    return t.permute(2, 1, 0, 3).contiguous()


class _GroupedProj(torch.autograd.Function):
    """obs_proj of the packed window idx / val [S, B, A, cap] (engine order) by the stacked weight [A, E, k] and bias
    [A, E]: own -> [A, B, S, E] (agent g's rows by network g), all -> [A, A, B, S, E] (network, agent, env, slot).
    Forward on the GPU: one mfg_packed_project_grouped per slot, written straight into the agent-major window (row
    stride S E). Backward: the weight gradient is g^T D per agent block of dense rows D (mfg_packed_densify)."""

    @staticmethod
    def forward(ctx, weight, bias, idx, val, all_):
        S, B, A, cap = idx.shape
        E, k = weight.shape[1], weight.shape[2]
        ctx.save_for_backward(idx, val)
        ctx.all, ctx.k = all_, k
        wt = weight.detach().transpose(1, 2).contiguous()  # [A, k, E]
        shape = (A, A, B, S, E) if all_ else (A, B, S, E)
        if val.is_cuda:
            out = torch.empty(shape, dtype=torch.float32, device=val.device)
            st = learn_lib.stream(val.device)
            idx, val, b = idx.contiguous(), val.contiguous(), bias.detach().contiguous()
            for s in range(S):
                learn_lib.call('mfg_packed_project_grouped', idx[s].data_ptr(), val[s].data_ptr(), B * A, cap, A,
                               wt.data_ptr(), b.data_ptr(), E, k, 1 if all_ else 0, out.view(-1)[s * E:].data_ptr(),
                               S * E, st)
            return out
        d = _dense_rows(_agent_major(idx).view(-1, cap), _agent_major(val).view(-1, cap), k).view(A, B * S, k)
        if all_:
            out = torch.matmul(d[None], wt[:, None]) + bias.detach()[:, None, None]  # [A, A, B S, E]
        else:
            out = torch.baddbmm(bias.detach()[:, None], d, wt)
        return out.view(shape)

    @staticmethod
    def backward(ctx, g):
        idx, val = ctx.saved_tensors
        S, B, A, cap = idx.shape
        k, E = ctx.k, g.shape[-1]
        idx_am, val_am = _agent_major(idx).view(A, B * S, cap), _agent_major(val).view(A, B * S, cap)
        gw = torch.zeros((A, E, k), dtype=g.dtype, device=g.device)
        step = max(1, (1 << 27) // k)  # <= 512 MiB of dense rows at a time
        for a in range(A):
            for r0 in range(0, B * S, step):
                d = _dense_rows(idx_am[a, r0:r0 + step], val_am[a, r0:r0 + step], k)
                if ctx.all:  # every network's gradient on agent a's rows
                    gw += torch.matmul(g[:, a].reshape(A, B * S, E)[:, r0:r0 + step].transpose(1, 2), d)
                else:
                    gw[a] += g[a].reshape(B * S, E)[r0:r0 + step].t() @ d
        gb = g.sum((1, 2, 3)) if ctx.all else g.sum((1, 2))
        return gw, gb, None, None, None


# ---------------------------------------------------------------------------------------------------------------------
# one GRU of every network over a window
# ---------------------------------------------------------------------------------------------------------------------
class _GRUWindowG(torch.autograd.Function):
    """One GRU of A networks over a window: gi [A, n, T, 3hd] (the input gates, with grad), keep [A, n, T] (0 = a
    restart at that entry), h0 [A, n, hd] (no gradient), wh [A, 3hd, hd], bh [A, 3hd] -> hs [A, n, T, hd]. The
    recurrence is gru_window's on the A n rows with the stacked weight (per step one bmm over agents and, on the GPU,
    one elementwise kernel: mfg_gru_fwd_step_grouped takes a row's recurrent bias from its agent block, mfg_gru_bwd_step
    reads no bias); the recurrent-weight gradient is one bmm over the window."""

    @staticmethod
    def forward(ctx, gi, keep, h0, wh, bh):
        A, n, T, g3 = gi.shape
        hd = g3 // 3
        if gru_window.use_kernels(gi) and (gi.stride(3) != 1 or gi.stride(0) != n * gi.stride(1)):
            gi = gi.contiguous()  # (a column slice of both GRUs' gates is read in place)
        hs = torch.empty((A, n, T, hd), dtype=gi.dtype, device=gi.device)
        sv = torch.empty((5, A, n, T, hd), dtype=gi.dtype, device=gi.device)  # hp, r, z, n, gh_n
        gru_window.forward_steps(gi.flatten(0, 1), keep.flatten(0, 1), h0.flatten(0, 1), wh, bh, hs.flatten(0, 1),
                                 sv.flatten(1, 2))
        ctx.save_for_backward(keep, wh, *sv.unbind(0))
        return hs

    @staticmethod
    def backward(ctx, dout):
        keep, wh, *sv = ctx.saved_tensors
        A, n, T, hd = sv[0].shape
        dgi = torch.empty((A, n, T, 3 * hd), dtype=dout.dtype, device=dout.device)
        dgh = torch.empty_like(dgi)
        gru_window.backward_steps(dout.contiguous().flatten(0, 1), keep.flatten(0, 1), [v.flatten(0, 1) for v in sv],
                                  wh, dgi.flatten(0, 1), dgh.flatten(0, 1))
        dgh2 = dgh.view(A, n * T, 3 * hd)
        return dgi, None, None, torch.bmm(dgh2.transpose(1, 2), sv[0].reshape(A, n * T, hd)), dgh2.sum(1)


# ---------------------------------------------------------------------------------------------------------------------
# the networks
# ---------------------------------------------------------------------------------------------------------------------
class AgentNets(nn.Module):
    """A ``RecurrentAC``s (networks.py:7-69, ``use_agent_embedding=False``) with every parameter stacked on a leading
    agent axis: parameter ``obs_proj.weight`` of the reference is ``P['obs_proj.weight'] [A, E, k]`` here. n_actions
    may be a list (one count per agent): the action embedding and the action head are stacked at the largest count,
    agent g uses its first n_actions[g] logits / n_actions[g] + 1 embedding rows and the padded rows stay zero
    (they receive no gradient). ``state_dicts`` / ``load_state_dicts`` / ``to_modules`` / ``from_modules`` read and
    write one reference state dict per agent (the reference keeps one ``.pt`` per agent, iac.py:22-25)."""

    def __init__(self, observation_size, n_actions, obs_emb_size, action_emb_size, hidden_size_actor,
                 hidden_size_critic, n_agents, use_agent_embedding=False):
        super().__init__()
        if use_agent_embedding:
            raise ValueError('AgentNets: use_agent_embedding=True is not supported (the reference sizes the mix input '
                             'inconsistently there, networks.py:22)')
        counts = [int(n_actions)] * n_agents if np.ndim(n_actions) == 0 else [int(x) for x in n_actions]
        if len(counts) != n_agents or min(counts) < 1:
            raise ValueError('AgentNets: n_actions needs one positive count per agent')
        self.A, self.n_act, self.n_max = n_agents, counts, max(counts)
        self.cfg = dict(observation_size=observation_size, obs_emb_size=obs_emb_size, action_emb_size=action_emb_size,
                        hidden_size_actor=hidden_size_actor, hidden_size_critic=hidden_size_critic, n_agents=n_agents)
        self.hidden_size_actor, self.hidden_size_critic = hidden_size_actor, hidden_size_critic
        self.obs_emb_size, self.action_emb_size = obs_emb_size, action_emb_size
        self.use_agent_embedding = False
        self._keys = []
        self._stack([self._module(g).state_dict() for g in range(n_agents)])

    def _module(self, g):
        return RecurrentAC(n_actions=self.n_act[g], use_agent_embedding=False, **self.cfg)

    @staticmethod
    def _attr(key):
        return 'p_' + key.replace('.', '__')

    def _stack(self, dicts):
        """The A state dicts stacked (padded keys at n_max rows, zero filled) into this module's parameters."""
        self._keys = list(dicts[0].keys())
        for k in self._keys:
            vs = [d[k].detach().float() for d in dicts]
            if k in _PAD_KEYS:
                rows = self.n_max + (1 if k == 'action_emb.weight' else 0)
                vs = [torch.cat([v, v.new_zeros((rows - v.shape[0],) + tuple(v.shape[1:]))], 0) for v in vs]
            new = torch.stack(vs, 0)
            if hasattr(self, self._attr(k)):
                with torch.no_grad():
                    getattr(self, self._attr(k)).copy_(new)
            else:
                self.register_parameter(self._attr(k), nn.Parameter(new.clone()))

    @property
    def P(self):
        return {k: getattr(self, self._attr(k)) for k in self._keys}

    def state_dicts(self):
        """One reference ``RecurrentAC`` state dict per agent (padded rows cut off)."""
        out = []
        for g in range(self.A):
            d = {}
            for k, p in self.P.items():
                v = p.detach()[g]
                if k in _PAD_KEYS:
                    v = v[:self.n_act[g] + (1 if k == 'action_emb.weight' else 0)]
                d[k] = v.clone()
            out.append(d)
        return out

    def load_state_dicts(self, dicts):
        dicts = list(dicts)
        if len(dicts) != self.A:
            raise ValueError(f'AgentNets: {len(dicts)} state dicts for {self.A} agents')
        for g, d in enumerate(dicts):
            self._module(g).load_state_dict(d)  # the reference module's own shape and key check
        self._stack(dicts)

    def to_modules(self):
        mods = []
        for g, d in enumerate(self.state_dicts()):
            m = self._module(g)
            m.load_state_dict(d)
            mods.append(m.to(d['obs_proj.weight'].device))
        return mods

    @classmethod
    def from_modules(cls, modules):
        modules = list(modules)
        m0 = modules[0]
        if any(m.use_agent_embedding for m in modules):
            raise ValueError('AgentNets: use_agent_embedding=True is not supported')
        nets = cls(m0.obs_proj.weight.shape[1], [m.n_actions for m in modules], m0.obs_proj.weight.shape[0],
                   m0.action_emb_size, m0.hidden_size_actor, m0.hidden_size_critic, len(modules))
        nets.load_state_dicts([m.state_dict() for m in modules])
        return nets.to(m0.obs_proj.weight.device)

    def agent_params(self):
        """The trained parameters (the agent embedding is unused without use_agent_embedding)."""
        return [p for k, p in self.P.items() if k != 'agent_emb.weight']

    def clip_grad_norm_per_agent(self, max_norm):
        """``clip_grad_norm_(net.parameters(), max_norm)`` of every agent's network (iac.py:55, seac.py:52): one norm
        per agent slice over all its parameters. Returns the norms [A]."""
        ps = [p for p in self.parameters() if p.grad is not None]
        sq = sum(p.grad.reshape(self.A, -1).pow(2).sum(1) for p in ps)
        total = sq.sqrt()
        coef = (max_norm / (total + 1e-6)).clamp(max=1.0)
        for p in ps:
            p.grad.mul_(coef.view((self.A,) + (1,) * (p.dim() - 1)))
        return total

    def project(self, idx, val, all_=False):
        """obs_proj on a packed window idx / val [S, B, A, cap] in engine order: [A, B, S, E], or with all_ every
        network on every agent's rows [A(network), A(agent), B, S, E]."""
        P = self.P
        return _GroupedProj.apply(P['obs_proj.weight'], P['obs_proj.bias'], idx, val, bool(all_))

    def forward_emb(self, obs_emb, actions, hidden_actor, hidden_critic, starts=None):
        """networks.py:50-69 for every network on its rows: obs_emb [A, n, T, E] (obs_proj output), actions [A, n, T]
        (last action, -1 = none), hidden [A, n, H]; starts [A, n, T] bool: the recurrent state restarts from zero at
        these entries. Returns logits [A, n, T, n_max] (agent g: the first n_act[g] columns), critic [A, n, T] and
        the recurrent outputs [A, n, T, H]."""
        if obs_emb.is_cuda or self.A == 1:
            return self._forward(self.P, obs_emb, actions, hidden_actor, hidden_critic, starts)
        # CPU: agent by agent through the same code (elementwise CPU kernels round an element by its position in
        # the tensor, so only equal shapes give the separate modules' bits)
        outs = []
        for g in range(self.A):
            na = self.n_act[g]  # the agent's own head size: a GEMM's rounding follows its shape
            P = {k: p[g:g + 1, :na + (k == 'action_emb.weight')] if k in _PAD_KEYS else p[g:g + 1]
                 for k, p in self.P.items()}
            o = self._forward(P, obs_emb[g:g + 1], actions[g:g + 1], hidden_actor[g:g + 1], hidden_critic[g:g + 1],
                              None if starts is None else starts[g:g + 1])
            o['logits'] = F.pad(o['logits'], (0, self.n_max - na))  # the padded head rows are zero
            outs.append(o)
        return {k: torch.cat([o[k] for o in outs], 0) for k in outs[0]}

    def _forward(self, P, obs_emb, actions, hidden_actor, hidden_critic, starts):
        A, n, T, E = obs_emb.shape
        aw = P['action_emb.weight']
        aw = torch.cat([aw[:, :1].detach(), aw[:, 1:]], 1)  # padding_idx 0: that row gets no gradient
        oh = F.one_hot(actions.reshape(A, n * T) + 1, aw.shape[1]).to(obs_emb.dtype)
        x = torch.cat((obs_emb.reshape(A, n * T, E), torch.bmm(oh, aw)), -1)
        x = _blin(torch.tanh(x), P['mix.1.weight'], P['mix.1.bias'])
        x = _blin(torch.tanh(x), P['mix.3.weight'], P['mix.3.bias'])
        keep = torch.ones((A, n, T), dtype=x.dtype, device=x.device) if starts is None else (~starts).to(x.dtype)
        # the input gates of both GRUs as one GEMM per agent, as marl._GRUWindow forms them
        gi = _blin(x, torch.cat([P['gru_actor.weight_ih_l0'], P['gru_critic.weight_ih_l0']], 1),
                   torch.cat([P['gru_actor.bias_ih_l0'], P['gru_critic.bias_ih_l0']], 1)).view(A, n, T, -1)
        sa = 3 * self.hidden_size_actor
        out_p = _GRUWindowG.apply(gi[..., :sa], keep, hidden_actor.detach(), P['gru_actor.weight_hh_l0'],
                                  P['gru_actor.bias_hh_l0'])
        out_c = _GRUWindowG.apply(gi[..., sa:], keep, hidden_critic.detach(), P['gru_critic.weight_hh_l0'],
                                  P['gru_critic.bias_hh_l0'])
        hp = torch.tanh(_blin(out_p.reshape(A, n * T, -1), P['action_head.0.weight'], P['action_head.0.bias']))
        logits = _blin(hp, P['action_head.2.weight'], P['action_head.2.bias']).view(A, n, T, -1)
        hc = torch.tanh(_blin(out_c.reshape(A, n * T, -1), P['critic_head.0.weight'], P['critic_head.0.bias']))
        critic = _blin(hc, P['critic_head.2.weight'], P['critic_head.2.bias']).view(A, n, T)
        return dict(logits=logits, critic=critic, hidden_actor=out_p, hidden_critic=out_c)

    def entry_floats(self):
        """f32 values the learner keeps per (network, row, entry) of a window for the backward pass."""
        E, AE, Ha, Hc = self.obs_emb_size, self.action_emb_size, self.hidden_size_actor, self.hidden_size_critic
        mix = (self.n_max + 1) + 2 * (E + AE) + 4 * E  # one-hot, cat and its tanh, two layers and the tanh between
        gru = 3 * (Ha + Hc) + 6 * (Ha + Hc)  # input gates, outputs and the five saved activations
        heads = 2 * (Ha + Hc) + self.n_max + 1
        return E + mix + gru + heads


# ---------------------------------------------------------------------------------------------------------------------
# the losses
# ---------------------------------------------------------------------------------------------------------------------
def _adv(critic, reward, done, gamma, gae_coef):
    lead = critic.shape[:-1]
    t = reward.shape[-1]
    return compute_advantages(critic.reshape(-1, t + 1), reward.reshape(-1, t), done.reshape(-1, t), gamma,
                              gae_coef).view(*lead, t)


def iac_loss_terms(logits, critic, actions, reward, done, gamma, entropy_coef, vf_coef, gae_coef=0.0, n_act=None,
                   terms=False):
    """``base_ac.py:200-217`` per agent (iac.py:50-57), every agent by its own network: logits [A, B, T, n_max]
    (entries 0..T-1), critic [A, B, T+1], actions (long) / reward / done [A, B, T] -> loss [A]. n_act: per-agent action
    counts (agent g's distribution runs over its first n_act[g] logits). terms=True returns (policy, value, entropy)
    [A] instead."""
    A = logits.shape[0]
    adv = _adv(critic, reward, done, gamma, gae_coef)
    value = adv.pow(2).mean((1, 2))
    if n_act is None or all(int(c) == logits.shape[-1] for c in n_act):
        lp = torch.log_softmax(logits, -1)
        ent = Categorical(logits=logits, validate_args=False).entropy().mean((1, 2))
        log_ap = torch.gather(lp, -1, actions.unsqueeze(-1)).squeeze(-1) + nonfinite_to_nan(logits)
    else:
        ents, laps = [], []
        for g in range(A):
            lg = logits[g, ..., :int(n_act[g])]
            ents.append(Categorical(logits=lg, validate_args=False).entropy().mean())
            laps.append(torch.gather(torch.log_softmax(lg, -1), -1, actions[g].unsqueeze(-1)).squeeze(-1) +
                        nonfinite_to_nan(lg))
        ent, log_ap = torch.stack(ents), torch.stack(laps)
    policy = -(adv.detach() * log_ap).mean((1, 2))
    if terms:
        return policy, value, ent
    return policy + vf_coef * value - entropy_coef * ent


def seac_loss_terms(logits, critic, actions, reward, done, gamma, entropy_coef, vf_coef, gae_coef=0.0, terms=False):
    """``seac.py:12-47``: logits [A, A, B, T, n_act] (network, agent, env; entries 0..T-1), critic [A, A, B, T+1],
    actions (long) / reward / done [A, B, T] of the (agent, env) rows -> loss [A] per network. The importance weight
    iw = exp(logp_network - logp_(row's own network)) is a constant (1 on the diagonal); the entropy runs over the
    network's own agent. terms=True returns (policy, value, entropy) [A] instead."""
    A = logits.shape[0]
    lp = torch.log_softmax(logits, -1)
    log_ap = torch.gather(lp, -1, actions[None].expand(A, *actions.shape).unsqueeze(-1)).squeeze(-1)  # [A, A, B, T]
    log_ap = log_ap + nonfinite_to_nan(logits)  # NaN; in the row's own network it spoils every network's iw
    ar = torch.arange(A, device=logits.device)
    true_lp = log_ap[ar, ar]  # [A(agent), B, T]: the behaviour policy
    iw = (log_ap - true_lp[None]).exp().detach()
    adv = _adv(critic, reward[None].expand(A, *reward.shape), done[None].expand(A, *done.shape), gamma, gae_coef)
    policy = (-iw * log_ap * adv.detach()).mean((1, 2, 3))
    value = (iw * adv.pow(2)).mean((1, 2, 3))
    ent = Categorical(logits=logits[ar, ar], validate_args=False).entropy().mean((1, 2))
    if terms:
        return policy, value, ent
    return policy + vf_coef * value - entropy_coef * ent


class _SEACHead(torch.autograd.Function):
    """iac_loss_terms / seac_loss_terms on the GPU as one HIP call (mfg_seac_head, include/mfg_learn.h): the loss [A]
    with dlogits and dcritic for a loss gradient of 1 per network; the backward scales them per network. logits
    [A, n, T+1, n_max] / critic [A, n, T+1] (cross) or [n, T+1, n_max] / [n, T+1] (own), n = A B agent-major rows, all
    T+1 entries (entry T's gradients are zero); action i32 / reward f32 / done f32 are indexed (step, env, agent) by
    the given element strides. A NaN loss marks an action outside the range or non-finite logits."""

    @staticmethod
    def forward(ctx, logits, critic, action, a_str, reward, r_str, done, d_str, n_act, A, B, gamma, entropy_coef,
                vf_coef, gae_coef, cross):
        dev = logits.device
        t, n_max = logits.shape[-2] - 1, logits.shape[-1]
        lg, cr = logits.detach().float().contiguous(), critic.detach().float().contiguous()
        loss = torch.empty(A, dtype=torch.float32, device=dev)
        dlogits, dcritic = torch.empty_like(lg), torch.empty_like(cr)
        ws = torch.empty(seac_ws_bytes(A) // 8, dtype=torch.float64, device=dev)
        learn_lib.call('mfg_seac_head', lg.data_ptr(), cr.data_ptr(), A, B, t, n_max, action.data_ptr(), *a_str,
                       reward.data_ptr(), *r_str, done.data_ptr(), *d_str, n_act.data_ptr(), gamma, gae_coef, vf_coef,
                       entropy_coef, 1 if cross else 0, loss.data_ptr(), dlogits.data_ptr(), dcritic.data_ptr(),
                       ws.data_ptr(), learn_lib.stream(dev))
        ctx.save_for_backward(dlogits, dcritic)
        ctx.A, ctx.cross = A, cross
        return loss

    @staticmethod
    def backward(ctx, g):
        dlogits, dcritic = ctx.saved_tensors
        A = ctx.A
        if ctx.cross:
            gl, gc = g.view(A, 1, 1, 1) * dlogits, g.view(A, 1, 1) * dcritic
        else:
            n = dcritic.shape[0]
            gl = (g.view(A, 1, 1, 1) * dlogits.view(A, n // A, *dlogits.shape[1:])).view_as(dlogits)
            gc = (g.view(A, 1, 1) * dcritic.view(A, n // A, -1)).view_as(dcritic)
        return (gl, gc) + (None,) * 14


# ---------------------------------------------------------------------------------------------------------------------
# the learners
# ---------------------------------------------------------------------------------------------------------------------
class BatchedIAC(WindowRollout):
    """Independent actor-critic (``algorithms/marl/iac.py`` ``LoopIAC``) over B envs x A agents of one engine,
    everything on the device: one network per agent (``AgentNets``), each trained on its own agent's window with the
    A2C loss, RMSprop(3e-4, eps 1e-5) on the stacked parameters (elementwise, so it equals A separate optimisers) and
    ``clip_grad_norm_(0.5)`` per agent. Agents may have different action counts (``spec.n_actions``).

    The loop is ``rollout.WindowRollout``'s, as ``BatchedA2C``'s: entry t of the window holds (o_t, a_{t-1}) as the network input and a_t, r_t, d_t as
    targets; after a done the next entry's action input is -1 and its recurrent state zero; the engine auto-resets
    and its floor-shuffle replay is deferred to the window's last step; ``episodes`` / ``reward_sum`` fold in a window
    in ``learn``; with ``check_cap`` a learn call raises on truncated packed rows and on non-finite acting logits.
    The engine renders packed rows only (a ``PackedObs`` without the fused projection: that carries one weight
    matrix); ``obs_proj`` runs in ``mfg_packed_project_grouped``. The learner recomputes the window with grad.
    ``fused_head``: the loss and its gradients by ``mfg_seac_head`` on the GPU (``iac_loss_terms`` /
    ``seac_loss_terms`` otherwise and on the CPU); None takes the class default, the head whose loop measured
    faster."""

    cross = False
    fused_default = True  # measured on the MI355X (profiles/seac.json): the loop is faster with the fused head

    def __init__(self, factory, nets=None, n_steps=5, gamma=0.99, entropy_coef=0.01, vf_coef=0.5, gae_coef=0.0,
                 lr=3e-4, cap=32, obs_emb_size=96, action_emb_size=16, hidden_size=64, use_agent_embedding=False,
                 fused_head=None, check_cap=True, generator=None):
        if use_agent_embedding:
            raise ValueError(f'{type(self).__name__}: use_agent_embedding=True is not supported')
        self.n_act = [int(x) for x in factory.spec.n_actions]
        if self.cross and len(set(self.n_act)) != 1:
            raise ValueError('BatchedSEAC evaluates every network on every agent\'s actions: all agents need the same '
                             'number of actions')
        super().__init__(factory, cap, check_cap, generator)
        self.nets = nets if nets is not None else AgentNets(self.kdim, self.n_act, obs_emb_size, action_emb_size,
                                                            hidden_size, hidden_size, self.A)
        if list(self.nets.n_act) != self.n_act:
            raise ValueError(f'the networks\' action counts {self.nets.n_act} differ from the spec\'s {self.n_act}')
        self.nets.to(self.dev)
        self.n_max = self.nets.n_max
        self.uniform = len(set(self.n_act)) == 1
        self.opt = torch.optim.RMSprop(self.nets.agent_params(), lr=lr, eps=1e-5)
        self.T, self.gamma, self.entropy_coef, self.vf_coef, self.gae_coef = n_steps, gamma, entropy_coef, vf_coef, \
            gae_coef
        self.fused_head = self.fused_default if fused_head is None else bool(fused_head)
        A, B, dev = self.A, self.B, self.dev
        # entries only (obs_proj is per agent: no fused projection); h0a / h0c: the states fed at entry 0 of the window
        self._alloc((self.nets.hidden_size_actor, self.nets.hidden_size_critic), agent_major=True)
        self._u = torch.empty((A, B), device=dev)
        self._act_am = torch.zeros((A, B), dtype=torch.int32, device=dev)  # the sampled actions, agent-major
        self.n_act_dev = torch.tensor(self.n_act, dtype=torch.int32, device=dev)
        self.last_loss = torch.zeros(A, device=dev)  # per network

    def activation_bytes(self):
        """The learner's window memory: f32 activations kept for the backward pass, per (network, row, entry) the
        layers' outputs (``AgentNets.entry_floats``) x A B rows (IAC) or A A B (SEAC: every network on every row) x
        n_steps + 1 entries."""
        rows = self.A * self.N if self.cross else self.N
        return 4 * rows * (self.T + 1) * self.nets.entry_floats()

    @torch.no_grad()
    def step(self):
        """One env-step of every env, every agent acting with its own network (no host sync)."""
        if not self._started:
            self.reset()
        t = self.t
        emb = self.nets.project(self.pobs.idx[t:t + 1], self.pobs.val[t:t + 1])  # [A, B, 1, E]
        out = self.nets.forward_emb(emb, self.act_in[t].t()[:, :, None], self.ha, self.hc)
        self._sample(out['logits'][:, :, 0], t)
        self._window_step(out['hidden_actor'][:, :, 0], out['hidden_critic'][:, :, 0])

    def _sample(self, logits, t):
        """a_t ~ Categorical(logits[g, b, :n_act[g]]) into act[t] [B, A] (base_ac.py:74-76): mfg_sample_categorical on
        the GPU, one call over all rows, or one per agent block when the action counts differ."""
        A, B = self.A, self.B
        if self.gen is not None or not logits.is_cuda:
            for g in range(A):
                lg = logits[g, :, :self.n_act[g]]
                if self.gen is not None:
                    a = torch.multinomial(torch.softmax(lg, -1), 1, generator=self.gen).squeeze(-1)
                else:
                    a = Categorical(logits=lg, validate_args=False).sample()
                self._act_am[g].copy_(a)
        else:
            logits = logits.contiguous()
            self._u.uniform_()
            st = learn_lib.stream(self.dev)
            blocks = [(0, A * B, self.n_max)] if self.uniform else [(g * B, B, self.n_act[g]) for g in range(A)]
            for r0, rows, n in blocks:
                learn_lib.call('mfg_sample_categorical', logits.view(A * B, -1)[r0].data_ptr(), logits.shape[-1], n,
                               self._u.view(-1)[r0:].data_ptr(), rows, self._act_am.view(-1)[r0:].data_ptr(), st)
        self.act[t].copy_(self._act_am.t())

    def window(self):
        """The window's learner inputs and targets, agent-major: action inputs [A, B, T+1] (long), starts [A, B, T+1]
        (bool), actions [A, B, T] (long), reward and done [A, B, T] (f32)."""
        A, B, T = self.A, self.B, self.T
        a_in = self.act_in.permute(2, 1, 0)
        d = self.done.t().to(torch.float32)[None].expand(A, B, T)
        starts = torch.cat([torch.zeros((A, B, 1), dtype=torch.bool, device=self.dev), d.bool()], 2)
        return a_in, starts, self.act.permute(2, 1, 0).long(), self.rew.permute(2, 1, 0).to(torch.float32), d

    def evaluate(self):
        """The window's forward with grad: logits [A, n, T+1, n_max] and critic [A, n, T+1], n = B rows per network
        (IAC) or A B (SEAC: every network on every agent's rows, from that agent's acting state, seac.py:14)."""
        A, B, T = self.A, self.B, self.T
        a_in, starts, _, _, _ = self.window()
        emb = self.nets.project(self.pobs.idx, self.pobs.val, all_=self.cross)
        h0a, h0c = self.h0a, self.h0c
        if self.cross:
            emb = emb.view(A, A * B, T + 1, -1)
            a_in, starts = (x[None].expand(A, A, B, T + 1).reshape(A, A * B, T + 1) for x in (a_in, starts))
            h0a, h0c = (h[None].expand(A, *h.shape).reshape(A, A * B, -1) for h in (h0a, h0c))
        return self.nets.forward_emb(emb, a_in, h0a, h0c, starts=starts)

    def loss(self):
        """The per-network losses [A] of the current window, with grad."""
        A, B, T = self.A, self.B, self.T
        with torch.enable_grad():
            out = self.evaluate()
            logits, critic = out['logits'], out['critic']
            hyp = (self.gamma, self.entropy_coef, self.vf_coef, self.gae_coef)
            if self.fused_head and logits.is_cuda:
                rew = self.rew.to(torch.float32)
                dn = self.done.to(torch.float32)
                if not self.cross:
                    logits, critic = logits.reshape(A * B, T + 1, -1), critic.reshape(A * B, T + 1)
                return _SEACHead.apply(logits, critic, self.act, (B * A, A, 1), rew, (B * A, A, 1), dn, (B, 1, 0),
                                       self.n_act_dev, A, B, *hyp, self.cross)
            _, _, acts, rew, d = self.window()
            if self.cross:
                return seac_loss_terms(logits.view(A, A, B, T + 1, -1)[:, :, :, :T], critic.view(A, A, B, T + 1), acts,
                                       rew, d, *hyp)
            return iac_loss_terms(logits[:, :, :T], critic, acts, rew, d, *hyp, n_act=self.n_act)

    def learn(self):
        """One update of every network on the window (iac.py:50-57 / seac.py:49-54), then slide: o_T becomes o_0."""
        self._check(type(self).__name__, 'in this window')
        self._fold()
        with torch.enable_grad():
            loss = self.loss()
            self.opt.zero_grad(set_to_none=True)
            loss.sum().backward()  # network j's parameters enter loss[j] only
            self.nets.clip_grad_norm_per_agent(0.5)
            self.opt.step()
        with torch.no_grad():
            self.last_loss.copy_(loss.detach())
            self._slide()
        self.updates += 1
        self.t = 0


class BatchedSEAC(BatchedIAC):
    """Shared-experience actor-critic (``algorithms/marl/seac.py`` ``LoopSEAC``): ``BatchedIAC``'s networks, acting
    and loop; the learner evaluates every network on every agent's window (A x the activations of IAC, see
    ``activation_bytes``), each pass starting from the window owner's acting state (``seac.py:14``), and weighs the
    other agents' elements by the importance weight pi_j(a) / pi_i(a) (``seac_loss_terms`` / ``mfg_seac_head``). All
    agents need the same number of actions."""

    cross = True
    # (fused_default stays True: 0.616M against 0.610M env-steps/s, profiles/seac.json; the head is ~0.4 ms of a
    # ~67 ms window there, the A x network passes are the rest)
