// Kernels of the per-agent-network learners (mfg_amd/seac.py BatchedIAC / BatchedSEAC; the reference's
// algorithms/marl/iac.py and seac.py): obs_proj of packed rows by per-agent weights and the IAC / SEAC loss head
// (loss, dlogits and dcritic of all networks in one call; the GRU forward step with one recurrent bias per agent
// block is mfg_learn.hip's k_gru_fwd<true>). fp32 data, f64 accumulation of the loss sums; -ffp-contract=off keeps products and sums separately rounded,
// as in the tensor code (seac.py seac_loss_terms / iac_loss_terms).
//
// Loss head mapping: blockIdx.y = the network; a block takes 256 / (t + 1) whole (network, row) pairs at a time with
// one thread per entry of a pair, walking the n_act logits of its entry in short loops; the pair's two
// scans over its t steps run per thread on values staged in LDS, so no per-thread array exists. The behaviour
// policy's logp of a SEAC element is recomputed from the row's own network.
// Reductions are deterministic: a fixed shuffle + LDS tree per block into partials per (network, block), then a
// finishing kernel (one block per network) that adds them in a fixed order. No floating-point atomics.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>
#include "../../include/mfg_learn.h"
#include "mfg_learn_device.h"

namespace {

constexpr int SEAC_BLOCKS = 256;  // partial pairs per network: MFG_SEAC_WS_BYTES(g) = g * 256 * 2 * 8
static_assert(MFG_SEAC_WS_BYTES(1) == SEAC_BLOCKS * 2 * sizeof(double), "workspace bound");
constexpr int PROJ_MAX_CAP = 2048;  // the compacted entries of 4 rows in LDS: 4 * 2048 * 8 B = 64 KiB

// ---- packed-row projection by per-agent weights. One wave per row r (agent r % G): the row's nonzero entries are
// compacted once into a wave-private LDS list (every chunk of 64 entries is walked, zero values skipped), then each
// projection reads the list by LDS broadcast; lanes hold the columns c and c + 64 (e_dim <= 128). LDS instructions of
// one wave complete in issue order; the wave barriers keep the compiler from moving them across the phases.
__global__ void __launch_bounds__(256) k_project_grouped(const uint16_t* __restrict__ idx,
                                                         const float* __restrict__ val, int64_t m, int cap, int G,
                                                         const float* __restrict__ wt, const float* __restrict__ bias,
                                                         int e_dim, int k, int all, float* __restrict__ out,
                                                         int64_t out_row) {
  extern __shared__ uint32_t ent[];  // [4][cap][2]: (index, value bits)
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t r = (int64_t)blockIdx.x * 4 + wv;
  if (r >= m) return;  // no block-wide barrier below
  uint32_t* e = ent + (size_t)wv * cap * 2;
  int nnz = 0;
  for (int j0 = 0; j0 < cap; j0 += 64) {
    const bool in = j0 + lane < cap;
    const uint32_t my_i = in ? idx[r * cap + j0 + lane] : 0u;
    const float my_v = in ? val[r * cap + j0 + lane] : 0.0f;
    const bool keep = my_v != 0.0f && my_i < (uint32_t)k;
    const uint64_t nz = __ballot(keep);
    if (keep) {
      const int pos = nnz + __popcll(nz & ((1ull << lane) - 1ull));
      e[2 * pos] = my_i;
      e[2 * pos + 1] = __float_as_uint(my_v);
    }
    nnz += __popcll(nz);
  }
  __builtin_amdgcn_wave_barrier();
  const int g = (int)(r % G);
  const int64_t mb = m / G, q = r / G;
  const int c0 = lane, c1 = lane + 64;
  const bool on0 = c0 < e_dim, on1 = c1 < e_dim;
  const int j_lo = all ? 0 : g, j_hi = all ? G : g + 1;
  for (int j = j_lo; j < j_hi; j++) {
    const float* w = wt + (int64_t)j * k * e_dim;
    float a0 = 0.0f, a1 = 0.0f;
    for (int p = 0; p < nnz; p++) {
      const int64_t kk = e[2 * p];
      const float v = __uint_as_float(e[2 * p + 1]);
      if (on0) a0 += v * w[kk * e_dim + c0];
      if (on1) a1 += v * w[kk * e_dim + c1];
    }
    const int64_t orow = all ? ((int64_t)j * G + g) * mb + q : (int64_t)g * mb + q;
    float* o = out + orow * out_row;
    if (on0) o[c0] = bias[j * e_dim + c0] + a0;
    if (on1) o[c1] = bias[j * e_dim + c1] + a1;
  }
}

// ---- the loss head
struct Strides { int64_t step, env, agent; };

// Network j = blockIdx.y, its rows q < rows (cross: all n = A B rows, agent q / B; own: the B rows of agent j).
// logits [nets][n][t + 1][n_max] (own: nets = 1, row = j B + q), critic alike without the last axis.
// A block takes R = 256 / (t + 1) whole (network, row) pairs at a time, one thread per entry s <= t of a pair, so the
// lanes of a wave walk consecutive entries: their logits are n_max floats apart and every fetched line is used whole.
// The two scans of a pair are short (t steps): every thread runs its own over the pair's critic, reward, done and
// value-gradient terms staged in LDS, in the evaluation order of a sequential scan.
__global__ void __launch_bounds__(256) k_seac_head(const float* __restrict__ logits, const float* __restrict__ critic,
                                                   int A, int64_t B, int t, int n_max,
                                                   const int32_t* __restrict__ action, Strides sa,
                                                   const float* __restrict__ reward, Strides sr,
                                                   const float* __restrict__ done, Strides sd,
                                                   const int32_t* __restrict__ n_act, float gamma, float lam, float vf,
                                                   float ent, int cross, float* __restrict__ dlogits,
                                                   float* __restrict__ dcritic, double* __restrict__ part) {
  __shared__ double sh[4];
  __shared__ float cr_sh[256], nd_sh[256], rw_sh[256], g_sh[256];
  const int j = blockIdx.y;
  const int na_in = n_act[j];
  const bool na_ok = na_in >= 1 && na_in <= n_max;  // a bad count: every element of the network is a bad element
  const int na = na_ok ? na_in : 1;
  const int64_t n = (int64_t)A * B;
  const int64_t rows = cross ? n : B;
  const float inv_all = 1.0f / (float)((double)rows * t);  // policy and value terms: a mean over the rows x steps
  const float inv_ent = 1.0f / (float)((double)B * t);     // entropy: over the network's own agent only
  const float gl = gamma * lam;
  const int t1 = t + 1;
  const int R = 256 / t1;  // pairs per block and pass (t + 1 <= 256, checked by the caller)
  const int lp = threadIdx.x / t1, s = threadIdx.x - lp * t1;
  const int base = lp * t1;  // the pair's first LDS slot
  double s_pv = 0.0, s_h = 0.0;
  for (int64_t q0 = (int64_t)blockIdx.x * R; q0 < rows; q0 += (int64_t)gridDim.x * R) {  // uniform over the block
    const int64_t q = q0 + lp;
    const bool live = lp < R && q < rows;
    const int64_t row = cross ? q : (int64_t)j * B + q;  // the row among the n agent-major rows
    const int i = live ? (int)(row / B) : 0;             // its agent
    const int64_t b = row - (int64_t)i * B;
    const int64_t p = cross ? (int64_t)j * n + row : row;  // the (network, row) pair
    __syncthreads();  // the previous pass is done with the LDS rows
    if (live) {
      cr_sh[threadIdx.x] = critic[p * t1 + s];
      if (s < t) {
        nd_sh[threadIdx.x] = 1.0f - done[s * sd.step + b * sd.env + i * sd.agent];
        rw_sh[threadIdx.x] = reward[s * sr.step + b * sr.env + i * sr.agent];
      }
    }
    __syncthreads();
    float g_val = 0.0f;
    if (live) {
      float* d = dlogits + (p * t1 + s) * (int64_t)n_max;
      if (s == t) {
        for (int c = 0; c < n_max; c++) d[c] = 0.0f;
      } else {
        // the advantage: the reverse scan from the last step down to this one
        float adv = 0.0f;
        for (int u = t - 1; u >= s; u--) {
          const float nd = nd_sh[base + u];
          const float td = (rw_sh[base + u] + (gamma * nd) * cr_sh[base + u + 1]) - cr_sh[base + u];
          adv = lam > 0.0f ? td + (gl * nd) * adv : td;
        }
        const float* l = logits + (p * t1 + s) * (int64_t)n_max;
        const float* own = logits + (((int64_t)i * n + row) * t1 + s) * (int64_t)n_max;  // cross: behaviour network
        const int a = action[s * sa.step + b * sa.env + i * sa.agent];
        float lse, lse_own = 0.0f;
        bool ok = row_lse_finite(l, na, lse) && a >= 0 && a < na && na_ok;  // every logit of the head finite
        const bool off = cross && i != j;
        if (off) ok = row_lse_finite(own, na, lse_own) && ok;
        if (!ok) {  // nothing indexed by a: zero gradients, and a NaN term in every loss the element enters
          for (int c = 0; c < n_max; c++) d[c] = 0.0f;
          s_pv += (double)NAN;
        } else {
          const float logp = l[a] - lse;
          const float iw = off ? expf(logp - (own[a] - lse_own)) : 1.0f;
          const bool ent_on = i == j;
          float h = 0.0f;  // entropy: -sum p logp
          if (ent_on)
            for (int c = 0; c < na; c++) {
              const float lpc = l[c] - lse;
              h -= expf(lpc) * lpc;
            }
          const float g_lp = -(iw * adv);  // d(-iw logp adv) / d logp[a]
          for (int c = 0; c < na; c++) {
            const float lpc = l[c] - lse;
            const float pc = expf(lpc);
            // d logp[a] / d l_c = [c == a] - p_c;  d(-ent H) / d l_c = ent p_c (logp_c + H)
            float g = (g_lp * ((c == a ? 1.0f : 0.0f) - pc)) * inv_all;
            if (ent_on) g += (ent * (pc * (lpc + h))) * inv_ent;
            d[c] = g;
          }
          for (int c = na; c < n_max; c++) d[c] = 0.0f;
          g_val = ((-2.0f * vf) * (iw * adv)) * inv_all;
          s_pv += (double)(-(iw * logp) * adv + vf * (iw * (adv * adv)));
          if (ent_on) s_h += (double)h;
        }
      }
      g_sh[threadIdx.x] = g_val;
    }
    __syncthreads();
    if (live) {
      // the value gradient through critic[s]: the forward scan acc_u = g_u + gamma lam (1 - done_{u-1}) acc_{u-1}
      float acc = 0.0f;
      if (s < t)
        for (int u = 0; u <= s; u++)
          acc = g_sh[base + u] + ((u > 0 && lam > 0.0f) ? (gl * nd_sh[base + u - 1]) * acc : 0.0f);
      dcritic[p * t1 + s] = acc;  // entry t: 0
    }
  }
  const double b1 = block_sum(s_pv, sh);
  const double b2 = block_sum(s_h, sh);
  if (threadIdx.x == 0) {
    part[((int64_t)j * SEAC_BLOCKS + blockIdx.x) * 2] = b1;
    part[((int64_t)j * SEAC_BLOCKS + blockIdx.x) * 2 + 1] = b2;
  }
}

__global__ void __launch_bounds__(256) k_seac_finish(const double* __restrict__ part, int nb, double count_all,
                                                     double count_ent, float ent, float* __restrict__ loss) {
  __shared__ double sh[4];
  const int j = blockIdx.x;
  double s1 = 0.0, s2 = 0.0;
  for (int b = threadIdx.x; b < nb; b += 256) {
    s1 += part[((int64_t)j * SEAC_BLOCKS + b) * 2];
    s2 += part[((int64_t)j * SEAC_BLOCKS + b) * 2 + 1];
  }
  const double t1 = block_sum(s1, sh);
  const double t2 = block_sum(s2, sh);
  if (threadIdx.x == 0) loss[j] = (float)(t1 / count_all - (double)ent * (t2 / count_ent));
}

}  // namespace

extern "C" int mfg_packed_project_grouped(const uint16_t* idx, const float* val, int64_t m, int cap, int g,
                                          const float* wt, const float* bias, int e_dim, int k, int all, float* out,
                                          int64_t out_row, void* stream) {
  if (m <= 0 || cap <= 0 || cap > PROJ_MAX_CAP || g <= 0 || m % g != 0 || e_dim <= 0 || e_dim > 128 || k <= 0 ||
      k > 4096 || out_row < e_dim || (m + 3) / 4 > (int64_t)INT32_MAX)
    return -1;
  hipLaunchKernelGGL(k_project_grouped, dim3((unsigned)((m + 3) / 4)), dim3(256), (size_t)cap * 4 * 2 * sizeof(uint32_t),
                     (hipStream_t)stream, idx, val, m, cap, g, wt, bias, e_dim, k, all ? 1 : 0, out, out_row);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

extern "C" int mfg_seac_head(const float* logits, const float* critic, int n_agents, int64_t n_envs, int t, int n_max,
                             const int32_t* action, int64_t act_step, int64_t act_env, int64_t act_agent,
                             const float* reward, int64_t rew_step, int64_t rew_env, int64_t rew_agent,
                             const float* done, int64_t done_step, int64_t done_env, int64_t done_agent,
                             const int32_t* n_act, float gamma, float gae_coef, float vf_coef, float entropy_coef,
                             int cross, float* loss, float* dlogits, float* dcritic, void* ws, void* stream) {
  if (n_agents <= 0 || n_agents > 65535 || n_envs <= 0 || t <= 0 || t > 255 || n_max <= 0 || !ws) return -1;
  const int64_t rows = cross ? (int64_t)n_agents * n_envs : n_envs;
  const int64_t per = 256 / (t + 1), groups = (rows + per - 1) / per;  // pairs per block and pass
  const int nb = (int)(groups < SEAC_BLOCKS ? groups : SEAC_BLOCKS);
  double* part = (double*)ws;
  const Strides sa{act_step, act_env, act_agent}, sr{rew_step, rew_env, rew_agent}, sd{done_step, done_env, done_agent};
  hipLaunchKernelGGL(k_seac_head, dim3(nb, n_agents), dim3(256), 0, (hipStream_t)stream, logits, critic, n_agents,
                     n_envs, t, n_max, action, sa, reward, sr, done, sd, n_act, gamma, gae_coef > 0.0f ? gae_coef : 0.0f,
                     vf_coef, entropy_coef, cross ? 1 : 0, dlogits, dcritic, part);
  hipLaunchKernelGGL(k_seac_finish, dim3(n_agents), dim3(256), 0, (hipStream_t)stream, (const double*)part, nb,
                     (double)rows * (double)t, (double)n_envs * (double)t, entropy_coef, loss);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
