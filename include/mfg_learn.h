/* mfg_learn.h — learner-side helpers of the on-GPU A2C loop (mfg_amd/marl.py BatchedA2C).
 *
 * Not part of the Factory.step boundary (include/mfg.h): the elementwise half of one GRU step of the learner's
 * window (torch.nn.GRU layer 0, gate order r, z, n), forward and backward, as one kernel each. They replace the
 * ~10 / ~15 PyTorch elementwise launches per step and GRU of the reference learner's recurrent pass
 * (algorithms/marl/networks.py:50-69 forward, autograd backward; base_ac.py:200-225 update). fp32, device
 * pointers pre-offset to step s, *_row = row strides in elements, launched on `stream` (a hipStream_t);
 * return 0, or -1 on a bad size or launch error. */
#ifndef MFG_LEARN_H
#define MFG_LEARN_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* h_out = n + z (hp - n) with hp = h keep (h NULL: zero state), gh = keep gh0 + bh, gh0 = h W_hh^T [n, 3hd]
 * contiguous, gi [n, 3hd] = x W_ih^T + b_ih; also stores hp, r, z, n, gh_n (the backward's inputs). */
int mfg_gru_fwd_step(const float* gi, int64_t gi_row, const float* gh0, const float* bh, const float* h,
                     int64_t h_row, const float* keep, int64_t keep_row, float* h_out, int64_t ho_row,
                     float* hp_out, float* r_out, float* z_out, float* n_out, float* ghn_out, int64_t sv_row,
                     int64_t n, int hd, void* stream);

/* dh = dout + keep_next dhp_next (either NULL: absent); writes dgi = [dr, dz, dn], dgh = [dr, dz, dn r] and
 * dhz = dh z [n, hd] contiguous (dhp of this step = dhz + dgh W_hh, a GEMM by the caller). */
int mfg_gru_bwd_step(const float* dout, int64_t do_row, const float* dhp_next, const float* keep_next,
                     int64_t keep_row, const float* r_s, const float* z_s, const float* n_s, const float* ghn_s,
                     const float* hp_s, int64_t sv_row, float* dgi, int64_t dgi_row, float* dgh, int64_t dgh_row,
                     float* dhz, int64_t n, int hd, void* stream);

/* the packed rows (idx u16 / val f32 [m, cap], a row's entries distinct, zero vals ignored) as dense f32 rows
 * out [m][k] (row stride out_row >= k; k <= 4096): the learner's D for obs_proj's weight gradient D^T g (replaces a
 * zero fill + scatter_add; marl.py _packed_grads). */
int mfg_packed_densify(const uint16_t* idx, const float* val, int64_t m, int cap, int k, float* out, int64_t out_row,
                       void* stream);

/* out[r][:e_dim] = bias + sum_j val[r][j] wt[idx[r][j]] for the packed rows (wt [k][e_dim] = obs_proj.weight^T), the
 * projection the render fuses (mfg_packed_obs.emb), for rows held outside a render (the learner's window slide).
 * Rows front-compacted as the engine writes them (include/mfg.h: the nonzero entries first, slots >= count idx 0 /
 * val 0): the kernel stops after the first 64-entry chunk that is not all nonzero, so entries behind a zero value in
 * an earlier chunk are outside its contract (mfg_packed_project_grouped visits every entry). Entries with idx >= k are
 * skipped; the products are added in entry order, then the bias: a row without entries gives the bias exactly, and on
 * such rows the result equals mfg_packed_project_grouped's with g = 1, all = 0 bit for bit. Any e_dim >= 1; columns
 * past e_dim of a row (out_row > e_dim) are untouched. */
int mfg_packed_project(const uint16_t* idx, const float* val, int64_t m, int cap, const float* wt, const float* bias,
                       int e_dim, int k, float* out, int64_t out_row, void* stream);

/* out[r] ~ Categorical(logits = logits[r][:n_act]) by inversion at u[r] in [0, 1) (the acting step's
 * Categorical(logits).sample(), base_ac.py:74-76, with the uniforms drawn by the caller): the first action a with
 * u s < sum_{j <= a} expf(l_j - max) in f32, s the whole sum, the last action when rounding passes the last bin.
 * Columns past n_act of a row (logit_row > n_act) are not read. A common offset of the row changes nothing. An action
 * of probability 0 in f32 (a logit ~104 or more below the maximum, or -inf beside finite ones, which
 * torch.distributions.Categorical accepts as well) is never picked, at u = 0 and u = 1 - 2^-24 included. -1 for a row
 * that is no distribution: every logit -inf, any +inf or any NaN (torch.distributions would raise there). */
int mfg_sample_categorical(const float* logits, int64_t logit_row, int n_act, const float* u, int64_t n, int32_t* out,
                           void* stream);

/* ---- the PPO loss head of the MAPPO learner (marl.py BatchedMAPPO; algorithms/marl/mappo.py:30-66), mfg_ppo.hip.
 * Both calls reduce deterministically (per-block partials in `ws`, then a one-block finishing pass in a fixed order;
 * no floating-point atomics): the same input gives bit-identical output on every run. `ws` is caller-provided
 * device scratch of at least MFG_PPO_WS_BYTES bytes (8-byte aligned) for any size; one buffer can serve both calls
 * on one stream. */
#define MFG_PPO_WS_BYTES 16384

/* ret[i][s] = reward[i][s] + gamma (1 - done[i][s]) ret[i][s+1], ret[i][t] = 0 (mappo.py:30-37), rows i < n, steps
 * s < t, *_row = row strides in elements (>= t); stats[0] = the mean and stats[1] = the unbiased (n t - 1) standard
 * deviation of all n t returns (mappo.py:48, torch.std), accumulated in f64, written as device doubles.
 * -1 when n t < 2 (no unbiased deviation). */
int mfg_mc_returns(const float* reward, int64_t rew_row, const float* done, int64_t done_row, int64_t n, int t,
                   float gamma, float* ret, int64_t ret_row, double* stats, void* ws, void* stream);

/* Forward and backward of mappo.py:41-66 over m = n t elements: logits / old_logits [m][n_act] (row strides
 * logit_row / old_row), critic, ret f32 [m], action i32 [m], stats from mfg_mc_returns. With
 * R = (ret - stats[0]) / (stats[1] + 1e-8), adv = R - critic, ratio = exp(logp[a] - old_logp[a]):
 *   loss[0] = mean_i( -min(ratio adv, clamp(ratio, 1 - c, 1 + c) adv) + vf adv^2 - ent H(softmax(logits_i)) )
 * and, for a loss gradient of 1, dlogits [m][n_act] (row stride dlogit_row) and dcritic [m]. adv is a constant in
 * the surrogate and differentiated in the value term; where the surrogates tie the gradient follows torch.min (an
 * even split) and torch.clamp (gradient at and inside the bounds), so inside the clip range it is adv through ratio.
 * An action outside [0, n_act) or non-finite logits in an element: loss[0] = NaN, that element's gradients 0, and
 * nothing is read or written out of bounds. */
int mfg_ppo_head(const float* logits, int64_t logit_row, const float* old_logits, int64_t old_row,
                 const float* critic, const int32_t* action, const float* ret, const double* stats, int64_t m,
                 int n_act, float clip_range, float vf_coef, float entropy_coef, float* loss, float* dlogits,
                 int64_t dlogit_row, float* dcritic, void* ws, void* stream);

/* ---- per-agent networks (marl.py AgentNets, BatchedIAC / BatchedSEAC; algorithms/marl/iac.py, seac.py),
 * mfg_seac.hip. G networks with their parameters stacked on a leading axis. */

/* obs_proj of packed rows by per-agent weights: idx u16 / val f32 [m][cap] in engine order (row r belongs to agent
 * r % g, m % g == 0), wt [g][k][e_dim] (= obs_proj.weight^T per network), bias [g][e_dim]. Written agent-major with
 * mb = m / g rows per agent (row stride out_row >= e_dim, columns past e_dim untouched):
 *   all == 0:  out[r % g][r / g]       = bias[r % g] + sum_j val[r][j] wt[r % g][idx[r][j]]
 *   all != 0:  out[n][r % g][r / g]    = bias[n] + sum_j val[r][j] wt[n][idx[r][j]]  for every network n < g
 * (the row's entries are read once for all g projections). Every one of the cap entries is visited; zero values and
 * indices >= k are skipped. -1 for m % g != 0, k > 4096, e_dim > 128 or cap > 2048. */
int mfg_packed_project_grouped(const uint16_t* idx, const float* val, int64_t m, int cap, int g, const float* wt,
                               const float* bias, int e_dim, int k, int all, float* out, int64_t out_row,
                               void* stream);

/* mfg_gru_fwd_step with one recurrent bias per block of rows: row r uses bh[r / rows_per_group][3 hd]
 * (n % rows_per_group == 0). The same arithmetic otherwise. (mfg_gru_bwd_step reads no bias: it serves grouped rows
 * unchanged.) */
int mfg_gru_fwd_step_grouped(const float* gi, int64_t gi_row, const float* gh0, const float* bh,
                             int64_t rows_per_group, const float* h, int64_t h_row, const float* keep,
                             int64_t keep_row, float* h_out, int64_t ho_row, float* hp_out, float* r_out,
                             float* z_out, float* n_out, float* ghn_out, int64_t sv_row, int64_t n, int hd,
                             void* stream);

/* Device scratch of mfg_seac_head for g networks (8-byte aligned), whatever the number of rows. */
#define MFG_SEAC_WS_BYTES(g) ((g) * 4096)

/* The IAC / SEAC loss of all A = n_agents networks with its gradients, for a loss gradient of 1 per network. Rows are
 * agent-major: row = agent * n_envs + env, n = n_agents * n_envs; entries 0..t of a row (t targets, t <= 255).
 *   cross != 0 (SEAC, seac.py:12-47):  logits [A][n][t+1][n_max], critic [A][n][t+1]: every network on every row;
 *   cross == 0 (IAC, base_ac.py:200-217 per agent):  logits [n][t+1][n_max], critic [n][t+1]: a row by its own network;
 * dlogits / dcritic have the shapes of logits / critic, loss is [A]. action i32, reward f32, done f32 of step s < t,
 * env b, agent i are read at s * x_step + b * x_env + i * x_agent (elements), so [T][B][A] engine buffers are read in
 * place. n_act [A] (device): network j's head uses its first n_act[j] <= n_max logits.
 *   td_s = reward_s + gamma (1 - done_s) critic[s+1] - critic[s]   (critic[s+1] a constant)
 *   adv_s = td_s (gae_coef <= 0), else adv_s = td_s + gamma gae_coef (1 - done_s) adv_{s+1}
 *   logp = log_softmax(logits[j][row][s])[action];  iw = exp(logp_j - logp_{agent(row)}) (a constant; 1 for cross == 0)
 *   cross:  loss[j] = mean_{row,s}(-iw logp adv + vf iw adv^2) - ent mean_{row of agent j, s} H(softmax(logits))
 *   own:    loss[j] = mean_{row of agent j, s}(-logp adv + vf adv^2 - ent H)
 * adv is a constant in the policy term and differentiated in the value term through critic[s] only. dcritic of entry
 * t, dlogits of entry t and of columns >= n_act[j] are 0. An action outside [0, n_act[j]), a non-finite logit (of
 * network j or, for iw, of the row's own network) or n_act[j] outside [1, n_max]: that element's gradients are 0
 * and every loss it enters is NaN; nothing is read or written out of bounds. Deterministic: per-block f64 partials
 * in `ws` (>= MFG_SEAC_WS_BYTES(n_agents) bytes), added in a fixed order; no floating-point atomics. */
int mfg_seac_head(const float* logits, const float* critic, int n_agents, int64_t n_envs, int t, int n_max,
                  const int32_t* action, int64_t act_step, int64_t act_env, int64_t act_agent,
                  const float* reward, int64_t rew_step, int64_t rew_env, int64_t rew_agent,
                  const float* done, int64_t done_step, int64_t done_env, int64_t done_agent,
                  const int32_t* n_act, float gamma, float gae_coef, float vf_coef, float entropy_coef, int cross,
                  float* loss, float* dlogits, float* dcritic, void* ws, void* stream);

/* ---- evaluation (mfg_amd/evaluate.py BatchedEvaluator; algorithms/marl/base_ac.py:152-183 eval_loop), mfg_act.hip. */

/* The actor of g stacked RecurrentAC networks (use_agent_embedding = False) for mfg_policy_act, every matrix K-major
 * (the transpose of the nn.Linear / nn.GRU parameter: wt[net][in][out]), contiguous f32 device arrays:
 *   action_emb [g][n_max + 1][AE]                          (row 0 = "no action", read like any other row)
 *   w1t [g][E + AE][E], b1 [g][E];  w3t [g][E][E], b3 [g][E]      (mix.1, mix.3)
 *   wiht [g][E][3H], bih [g][3H];  whht [g][H][3H], bhh [g][3H]   (gru_actor, gate order r, z, n)
 *   wat [g][H][H], ba [g][H];  wbt [g][H][n_max], bb [g][n_max]   (action_head.0, action_head.2) */
typedef struct mfg_actor_weights {
  const float *action_emb, *w1t, *b1, *w3t, *b3, *wiht, *bih, *whht, *bhh, *wat, *ba, *wbt, *bb;
} mfg_actor_weights;

/* One acting step of the actor for every row (env b < n_envs, agent i < n_agents), as one kernel, in f32; agent i
 * uses network i % g (g == 1: shared, g == n_agents: one per agent):
 *   a_in = prev_done[b] ? -1 : prev_action[b][i];  h_in = prev_done[b] ? 0 : h[b][i]
 *          (prev_action or prev_done NULL: an episode start for every row; an a_in outside [-1, n_max) counts as -1)
 *   ax = tanh(cat(emb[b][i], action_emb[a_in + 1]));  x = W3 tanh(W1 ax + b1) + b3
 *   h' = GRU cell on (x, h_in), mfg_gru_fwd_step's arithmetic                        -> h[b][i], in place
 *   lg = Wb tanh(Wa h' + ba) + bb                                                    -> logits_out (may be NULL)
 *   act = greedy ? argmax(lg[:n_act[net]]) (lowest index on ties)
 *                : mfg_sample_categorical's inversion at u[b][i] over lg[:n_act[net]];
 *         -1 for n_act[net] outside [1, n_max] or a row that is no distribution: every logit -inf, any +inf or any
 *         NaN among lg[:n_act[net]] (a -inf logit beside finite ones is an action of probability 0, never sampled,
 *         as in mfg_sample_categorical; greedy never picks it either)                -> act_out
 * emb and h are read at b * *_env + i * *_agent (elements): engine order [B][A][..] and agent-major [A][B][..] both
 * work in place. prev_action / act_out i32, u f32 and logits_out [..][n_max] (all n_max columns are written) are
 * [n_envs][n_agents] in engine order; prev_done u8 [n_envs]; n_act i32 [g] (device). u may be NULL with greedy.
 * Every output element is one k-ordered fmaf chain: deterministic, independent of the launch shape.
 * -1 (nothing launched) unless 1 <= e_dim <= 128, 1 <= ae_dim <= 32, 1 <= hd <= 128, 1 <= n_max <= 32 and
 * g in {1, n_agents}. */
int mfg_policy_act(const float* emb, int64_t emb_env, int64_t emb_agent, int64_t n_envs, int n_agents, int g,
                   int e_dim, int ae_dim, int hd, int n_max, const mfg_actor_weights* w, const int32_t* n_act,
                   const int32_t* prev_action, const uint8_t* prev_done, float* h, int64_t h_env, int64_t h_agent,
                   const float* u, int greedy, int32_t* act_out, float* logits_out, void* stream);

/* eval_loop's bookkeeping after one step, per env b (reward f64 [n_envs][n_agents], done u8 [n_envs] of that step):
 *   eps_rew[b][i] (f32) += (float) reward[b][i];  len[b] += 1
 *   if done[b]:  k = count[b]
 *       if k < n_episodes:  rows[b][k][i] = eps_rew[b][i];  rows[b][k][n_agents] = ((0 + e_0) + e_1) + ... in f32;
 *                           lengths[b][k] = len[b];  count[b] = k + 1;  if k + 1 == n_episodes: *finished += 1
 *       eps_rew[b][:] = 0;  len[b] = 0
 * rows f32 [n_envs][n_episodes][n_agents + 1], lengths / len / count i32, finished i32 (one integer atomic per env
 * that completes). An env with n_episodes rows keeps stepping and writes no result. */
int mfg_eval_fold(const double* reward, const uint8_t* done, int64_t n_envs, int n_agents, int n_episodes,
                  float* eps_rew, int32_t* len, int32_t* count, float* rows, int32_t* lengths, int32_t* finished,
                  void* stream);

#ifdef __cplusplus
}
#endif
#endif
