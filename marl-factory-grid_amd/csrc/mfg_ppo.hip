// The PPO loss head of the on-GPU MAPPO learner (mfg_amd/marl.py BatchedMAPPO; the reference's
// algorithms/marl/mappo.py:30-66): Monte-Carlo returns with their mean / unbiased std, and the clipped-surrogate
// loss with its gradients in one pass. fp32 data, f64 accumulation of the two reductions; -ffp-contract=off keeps
// products and sums separately rounded, as in the tensor code (marl.py mappo_loss).
//
// Mapping: one thread per row (mfg_mc_returns: a row of t steps; mfg_ppo_head: one (row, step) element with its
// n_act logits), grid-stride over at most MAX_BLOCKS blocks of 256. n_act is ~10: a lane's logits are 40 contiguous
// bytes and a wave's 64 elements 2.5 KiB contiguous, so every fetched line is used whole (the three passes over a
// lane's logits hit L1); DESIGN.md has the bytes per element and the measurements.
// Both reductions are deterministic: a fixed shuffle + LDS tree per block into a partial per block (workspace), then
// a one-block finishing kernel that adds the partials in a fixed order. No floating-point atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "../../include/mfg_learn.h"
#include "mfg_learn_device.h"

namespace {

constexpr int MAX_BLOCKS = 1024;  // partials per reduction: the workspace bound (MFG_PPO_WS_BYTES = 2 * 1024 * 8)
static_assert(2 * MAX_BLOCKS * sizeof(double) == MFG_PPO_WS_BYTES, "workspace bound");

// R_s = r_s + gamma (1 - d_s) R_{s+1}, R_t = 0 (mappo.py:30-37, f32 in the reference's evaluation order), and per
// block the f64 sums of (R - c) and (R - c)^2 with the pivot c = reward[0][t-1] (one of the returns: it keeps
// sum^2 / count from cancelling against the sum of squares when the mean is far from 0)
__global__ void __launch_bounds__(256) k_mc_returns(const float* __restrict__ reward, int64_t rew_row,
                                                    const float* __restrict__ done, int64_t done_row, int64_t n, int t,
                                                    float gamma, float* __restrict__ ret, int64_t ret_row,
                                                    double* __restrict__ part) {
  __shared__ double sh[4];
  const double c = (double)reward[t - 1];
  double s1 = 0.0, s2 = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const float* r = reward + i * rew_row;
    const float* d = done + i * done_row;
    float* o = ret + i * ret_row;
    float acc = 0.0f;
    for (int s = t - 1; s >= 0; s--) {
      acc = r[s] + (gamma * (1.0f - d[s])) * acc;
      o[s] = acc;
      const double x = (double)acc - c;
      s1 += x;
      s2 += x * x;
    }
  }
  const double b1 = block_sum(s1, sh);
  const double b2 = block_sum(s2, sh);
  if (threadIdx.x == 0) {
    part[blockIdx.x] = b1;
    part[MAX_BLOCKS + blockIdx.x] = b2;
  }
}

// stats = (mean, unbiased std) of the count = n t returns from nb block partials
__global__ void __launch_bounds__(256) k_mc_finish(const double* __restrict__ part, int nb, double count,
                                                   const float* __restrict__ reward, int t,
                                                   double* __restrict__ stats) {
  __shared__ double sh[4];
  double s1 = 0.0, s2 = 0.0;
  for (int b = threadIdx.x; b < nb; b += 256) {
    s1 += part[b];
    s2 += part[MAX_BLOCKS + b];
  }
  const double t1 = block_sum(s1, sh);
  const double t2 = block_sum(s2, sh);
  if (threadIdx.x == 0) {
    const double c = (double)reward[t - 1];
    const double var = (t2 - t1 * t1 / count) / (count - 1.0);
    stats[0] = c + t1 / count;
    stats[1] = sqrt(var > 0.0 ? var : (var == var ? 0.0 : var));  // rounding below 0 is 0; NaN stays NaN
  }
}

// One element per thread: forward term and the gradients for d loss = 1 (loss = mean of the terms over m).
__global__ void __launch_bounds__(256) k_ppo_head(const float* __restrict__ logits, int64_t lrow,
                                                  const float* __restrict__ old_logits, int64_t orow,
                                                  const float* __restrict__ critic, const int32_t* __restrict__ action,
                                                  const float* __restrict__ ret, const double* __restrict__ stats,
                                                  int64_t m, int n_act, float clip, float vf, float ent,
                                                  float* __restrict__ dlogits, int64_t drow,
                                                  float* __restrict__ dcritic, double* __restrict__ part) {
  __shared__ double sh[4];
  const double mean = stats[0], sd = stats[1] + 1e-8;
  const float inv_m = 1.0f / (float)m;
  const float lo = 1.0f - clip, hi = 1.0f + clip;
  double sum = 0.0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (int64_t)gridDim.x * 256) {
    const float* l = logits + i * lrow;
    const float* q = old_logits + i * orow;
    float* dl = dlogits + i * drow;
    const int a = action[i];
    float lse, qlse;
    const bool fin = row_lse_finite(l, n_act, lse), qfin = row_lse_finite(q, n_act, qlse);  // every logit finite
    const bool ok = a >= 0 && a < n_act && fin && qfin;
    if (!ok) {  // no indexing by a: zero gradients, and a NaN term makes the loss NaN
      for (int j = 0; j < n_act; j++) dl[j] = 0.0f;
      dcritic[i] = 0.0f;
      sum += (double)NAN;
      continue;
    }
    const float rhat = (float)(((double)ret[i] - mean) / sd);
    const float adv = rhat - critic[i];
    const float ratio = expf((l[a] - lse) - (q[a] - qlse));
    const float rc = fminf(fmaxf(ratio, lo), hi);
    const float s1 = ratio * adv, s2 = rc * adv;
    // torch.min splits the gradient evenly on a tie; clamp passes it at and inside its bounds
    const float cg = (ratio >= lo && ratio <= hi) ? 1.0f : 0.0f;
    const float w = s1 < s2 ? 1.0f : (s1 > s2 ? cg : 0.5f + 0.5f * cg);
    const float g_lp = -(w * adv) * ratio;  // d(-min) / d logp[a]
    float h = 0.0f;  // entropy: -sum p logp
    for (int j = 0; j < n_act; j++) {
      const float lp = l[j] - lse;
      h -= expf(lp) * lp;
    }
    for (int j = 0; j < n_act; j++) {
      const float lp = l[j] - lse;
      const float p = expf(lp);
      // d logp[a] / d l_j = [j == a] - p_j;  d(-ent H) / d l_j = ent p_j (logp_j + H)
      const float g = g_lp * ((j == a ? 1.0f : 0.0f) - p) + ent * (p * (lp + h));
      dl[j] = g * inv_m;
    }
    dcritic[i] = (-2.0f * vf * adv) * inv_m;
    sum += (double)(-fminf(s1, s2) + vf * (adv * adv) - ent * h);
  }
  const double b = block_sum(sum, sh);
  if (threadIdx.x == 0) part[blockIdx.x] = b;
}

__global__ void __launch_bounds__(256) k_ppo_finish(const double* __restrict__ part, int nb, double count,
                                                    float* __restrict__ loss) {
  __shared__ double sh[4];
  double s = 0.0;
  for (int b = threadIdx.x; b < nb; b += 256) s += part[b];
  const double t = block_sum(s, sh);
  if (threadIdx.x == 0) loss[0] = (float)(t / count);
}

int blocks_for(int64_t rows) { return (int)((rows + 255) / 256 < MAX_BLOCKS ? (rows + 255) / 256 : MAX_BLOCKS); }

}  // namespace

extern "C" int mfg_mc_returns(const float* reward, int64_t rew_row, const float* done, int64_t done_row, int64_t n,
                              int t, float gamma, float* ret, int64_t ret_row, double* stats, void* ws, void* stream) {
  if (n <= 0 || t <= 0 || n * (int64_t)t < 2 || rew_row < t || done_row < t || ret_row < t || !ws) return -1;
  const int nb = blocks_for(n);
  double* part = (double*)ws;
  hipLaunchKernelGGL(k_mc_returns, dim3(nb), dim3(256), 0, (hipStream_t)stream, reward, rew_row, done, done_row, n, t,
                     gamma, ret, ret_row, part);
  hipLaunchKernelGGL(k_mc_finish, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)part, nb,
                     (double)n * (double)t, reward, t, stats);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int mfg_ppo_head(const float* logits, int64_t logit_row, const float* old_logits, int64_t old_row,
                            const float* critic, const int32_t* action, const float* ret, const double* stats,
                            int64_t m, int n_act, float clip_range, float vf_coef, float entropy_coef, float* loss,
                            float* dlogits, int64_t dlogit_row, float* dcritic, void* ws, void* stream) {
  if (m <= 0 || n_act <= 0 || logit_row < n_act || old_row < n_act || dlogit_row < n_act || !ws) return -1;
  const int nb = blocks_for(m);
  double* part = (double*)ws;
  hipLaunchKernelGGL(k_ppo_head, dim3(nb), dim3(256), 0, (hipStream_t)stream, logits, logit_row, old_logits, old_row,
                     critic, action, ret, stats, m, n_act, clip_range, vf_coef, entropy_coef, dlogits, dlogit_row,
                     dcritic, part);
  hipLaunchKernelGGL(k_ppo_finish, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)part, nb, (double)m,
                     loss);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
