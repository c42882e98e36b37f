// Evaluation-side kernels (mfg_amd/evaluate.py BatchedEvaluator; include/mfg_learn.h, include/mfg_act.h):
//   mfg_policy_act: one acting step of RecurrentAC's actor (networks.py:50-69 without the critic) as ONE kernel,
//                   and with an action mask mfg_policy_act_masked (mfg_policy_act is its NULL-mask case),
//   mfg_eval_fold:  the per-step episode bookkeeping of eval_loop (base_ac.py:152-183) as ONE kernel.
//
// mfg_policy_act. A block of 256 threads owns a tile of 32 rows (env, agent) of one network; wave w owns rows
// 8w .. 8w+7 through every layer, lane l owns output columns l and l + 64. A layer's input rows sit in LDS (row
// stride a multiple of 4 floats, read as float4: every lane of a wave reads the same address, a broadcast), its
// weights are read from global memory K-major (wt[k][o]: the 64 lanes read 64 consecutive floats; the ~220 KB of
// weights do not fit a CU's LDS, every block walks them once and they stay in L2), and every output element is one
// k-ordered fmaf chain in a register: no split sums, no atomics, so the result does not depend on the launch shape
// and is bit-identical on every run. Intermediates never leave registers / LDS; per row the kernel reads the obs
// embedding, the last action, the done flag, the recurrent state and one uniform, and writes the new state, the
// action and (optionally) the logits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/mfg_learn.h"
#include "../../include/mfg_act.h"
#include "mfg_learn_device.h"

namespace {

constexpr int TILE = 32;      // rows per block
constexpr int WROWS = 8;      // rows per wave
constexpr int MAX_E = 128, MAX_AE = 32, MAX_H = 128, MAX_ACT = 32;

__host__ __device__ constexpr int pad4(int x) { return (x + 3) & ~3; }

// acc[c][r] += sum_k in[r][k] wt[k][col[c]] for the wave's WROWS rows (in: LDS rows of stride `ls`, zero padded to a
// multiple of 4 columns; wt: global, row stride ldw). col[c] must be a valid column (callers clamp and mask the store).
template <int NC>
__device__ __forceinline__ void dense(const float* __restrict__ in, int ls, int K, const float* __restrict__ wt, int ldw,
                                      const int (&col)[NC], float (&acc)[NC][WROWS]) {
  const int k4 = K & ~3;
#pragma unroll 2  // two k-quads of weight loads in flight per wave
  for (int k = 0; k < k4; k += 4) {
    float w[NC][4];
#pragma unroll
    for (int c = 0; c < NC; c++)
#pragma unroll
      for (int i = 0; i < 4; i++) w[c][i] = wt[(int64_t)(k + i) * ldw + col[c]];
#pragma unroll
    for (int r = 0; r < WROWS; r++) {
      const float4 a = *reinterpret_cast<const float4*>(in + r * ls + k);
#pragma unroll
      for (int c = 0; c < NC; c++) {
        acc[c][r] = fmaf(a.x, w[c][0], acc[c][r]);
        acc[c][r] = fmaf(a.y, w[c][1], acc[c][r]);
        acc[c][r] = fmaf(a.z, w[c][2], acc[c][r]);
        acc[c][r] = fmaf(a.w, w[c][3], acc[c][r]);
      }
    }
  }
  for (int k = k4; k < K; k++) {
#pragma unroll
    for (int c = 0; c < NC; c++) {
      const float w = wt[(int64_t)k * ldw + col[c]];
#pragma unroll
      for (int r = 0; r < WROWS; r++) acc[c][r] = fmaf(in[r * ls + k], w, acc[c][r]);
    }
  }
}

// out[r][o] = f(bias[o] + in[r] . wt[:, o]) for o < O <= 128 (lane's columns o = lane, lane + 64), into LDS rows
template <bool TANH>
__device__ __forceinline__ void layer(const float* __restrict__ in, int ls_in, int K, const float* __restrict__ wt,
                                      const float* __restrict__ bias, int O, float* __restrict__ out, int ls_out,
                                      int lane) {
  if (O > 64) {
    const int col[2] = {lane, min(lane + 64, O - 1)};
    float acc[2][WROWS] = {};
    dense<2>(in, ls_in, K, wt, O, col, acc);
#pragma unroll
    for (int r = 0; r < WROWS; r++) {
      const float v0 = acc[0][r] + bias[col[0]], v1 = acc[1][r] + bias[col[1]];
      out[r * ls_out + lane] = TANH ? tanhf(v0) : v0;
      if (lane + 64 < O) out[r * ls_out + lane + 64] = TANH ? tanhf(v1) : v1;
    }
  } else {
    const int col[1] = {min(lane, O - 1)};
    float acc[1][WROWS] = {};
    dense<1>(in, ls_in, K, wt, O, col, acc);
    if (lane < O) {
#pragma unroll
      for (int r = 0; r < WROWS; r++) {
        const float v = acc[0][r] + bias[lane];
        out[r * ls_out + lane] = TANH ? tanhf(v) : v;
      }
    }
  }
}

struct ActArgs {
  const float* emb; int64_t emb_env, emb_agent;
  int64_t n_envs; int n_agents, g, E, AE, H, n_max;
  mfg_actor_weights w;
  const int32_t* n_act; const int32_t* prev_action; const uint8_t* prev_done;
  float* h; int64_t h_env, h_agent;
  const float* u; int greedy; const uint32_t* mask; int32_t* act_out; float* logits_out;
  int64_t rows_per_group;
};

// row q of a group as (env b, agent i): per-agent networks (g > 1) put the agent on blockIdx.y and q is the env; the
// shared network walks the engine's [B][A] rows
__device__ __forceinline__ void row_env_agent(int g, int A, int64_t q, int64_t& b, int& i) {
  if (g > 1) { b = q; i = (int)blockIdx.y; }
  else { b = q / A; i = (int)(q - b * A); }
}

__global__ void __launch_bounds__(256) k_policy_act(const ActArgs p) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int E = p.E, AE = p.AE, H = p.H, NM = p.n_max, A = p.n_agents;
  const int lsA = pad4(max(E + AE, H)), lsB = pad4(max(max(E, H), NM)), lsC = pad4(H);
  float* bufA = lds;                    // [TILE][lsA]: ax, then x, then the head's hidden tanh (lsA >= E + AE, H)
  float* bufB = bufA + TILE * lsA;      // [TILE][lsB]: h1, then h', then the logits (lsB >= E, H, n_max)
  float* bufC = bufB + TILE * lsB;      // [TILE][lsC]: h_in
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int net = p.g > 1 ? (int)blockIdx.y % p.g : 0;
  const int64_t row0 = (int64_t)blockIdx.x * TILE;

  // weights of this block's network
  const float* aemb = p.w.action_emb + (int64_t)net * (NM + 1) * AE;
  const float* w1t = p.w.w1t + (int64_t)net * (E + AE) * E;
  const float* b1 = p.w.b1 + (int64_t)net * E;
  const float* w3t = p.w.w3t + (int64_t)net * E * E;
  const float* b3 = p.w.b3 + (int64_t)net * E;
  const float* wiht = p.w.wiht + (int64_t)net * E * 3 * H;
  const float* bih = p.w.bih + (int64_t)net * 3 * H;
  const float* whht = p.w.whht + (int64_t)net * H * 3 * H;
  const float* bhh = p.w.bhh + (int64_t)net * 3 * H;
  const float* wat = p.w.wat + (int64_t)net * H * H;
  const float* ba = p.w.ba + (int64_t)net * H;
  const float* wbt = p.w.wbt + (int64_t)net * H * NM;
  const float* bb = p.w.bb + (int64_t)net * NM;

  // ---- stage the tile's inputs: ax = tanh(cat(emb, action_emb[a_in + 1])) and h_in (zero padded rows / columns)
  for (int r = wv; r < TILE; r += 4) {
    const int64_t q = row0 + r;  // row inside the group
    const bool on = q < p.rows_per_group;
    int64_t b = 0; int i = 0;
    if (on) row_env_agent(p.g, A, q, b, i);
    const bool fresh = !p.prev_action || !p.prev_done || p.prev_done[b] != 0;  // episode start
    int a_in = (on && !fresh) ? p.prev_action[b * A + i] : -1;
    if (a_in < -1 || a_in >= NM) a_in = -1;
    const float* e = p.emb + b * p.emb_env + i * p.emb_agent;
    for (int c = lane; c < lsA; c += 64) {
      float v = 0.0f;
      if (on && c < E) v = tanhf(e[c]);
      else if (on && c < E + AE) v = tanhf(aemb[(a_in + 1) * AE + (c - E)]);
      bufA[r * lsA + c] = v;
    }
    const float* hr = p.h + b * p.h_env + i * p.h_agent;
    for (int c = lane; c < lsC; c += 64) bufC[r * lsC + c] = (on && !fresh && c < H) ? hr[c] : 0.0f;
  }
  __syncthreads();

  float* inA = bufA + wv * WROWS * lsA;
  float* inB = bufB + wv * WROWS * lsB;
  float* inC = bufC + wv * WROWS * lsC;

  // ---- mix: h1 = tanh(W1 ax + b1) -> bufB;  x = W3 h1 + b3 -> bufA
  for (int c = lane; c < lsB; c += 64)
    if (c >= E)
      for (int r = 0; r < WROWS; r++) inB[r * lsB + c] = 0.0f;  // the padding columns read by the next layer
  layer<true>(inA, lsA, E + AE, w1t, b1, E, inB, lsB, lane);
  __syncthreads();
  layer<false>(inB, lsB, E, w3t, b3, E, inA, lsA, lane);  // columns E .. pad4(E) of bufA: still tanh(action_emb) or 0,
  __syncthreads();                                        // never read below (K = E, tail loop stops at E)

  // ---- the GRU cell (gate order r, z, n; mfg_gru_fwd_step's arithmetic) on x (bufA) and h_in (bufC) -> h' (global, bufB)
  for (int j0 = 0; j0 < H; j0 += 64) {
    const int j = j0 + lane, jc = min(j, H - 1);
    const int col[3] = {jc, H + jc, 2 * H + jc};
    float gi[3][WROWS] = {}, gh[3][WROWS] = {};
    dense<3>(inA, lsA, E, wiht, 3 * H, col, gi);
    dense<3>(inC, lsC, H, whht, 3 * H, col, gh);
    const float bir = bih[jc], biz = bih[H + jc], bin = bih[2 * H + jc];
    const float bhr = bhh[jc], bhz = bhh[H + jc], bhn = bhh[2 * H + jc];
    float hn[WROWS];
#pragma unroll
    for (int r = 0; r < WROWS; r++) {
      const float hp = inC[r * lsC + jc];
      const float rg = sigm((gi[0][r] + bir) + (gh[0][r] + bhr));
      const float zg = sigm((gi[1][r] + biz) + (gh[1][r] + bhz));
      const float ng = tanhf((gi[2][r] + bin) + rg * (gh[2][r] + bhn));
      hn[r] = ng + zg * (hp - ng);
    }
    __syncthreads();  // every wave is done with bufB (h1) only after the x layer above; h' columns go in now
    if (j < H) {
#pragma unroll
      for (int r = 0; r < WROWS; r++) {
        inB[r * lsB + j] = hn[r];
        const int64_t q = row0 + wv * WROWS + r;
        if (q < p.rows_per_group) {
          int64_t b; int i;
          row_env_agent(p.g, A, q, b, i);
          p.h[b * p.h_env + i * p.h_agent + j] = hn[r];
        }
      }
    }
  }
  for (int c = H + lane; c < lsB; c += 64)
    if (c < pad4(H))
      for (int r = 0; r < WROWS; r++) inB[r * lsB + c] = 0.0f;
  __syncthreads();

  // ---- action head: t = tanh(Wa h' + ba) -> bufA;  lg = Wb t + bb -> bufB
  layer<true>(inB, lsB, H, wat, ba, H, inA, lsA, lane);
  __syncthreads();
  layer<false>(inA, lsA, H, wbt, bb, NM, inB, lsB, lane);
  __syncthreads();

  // ---- sample / argmax: one thread per row, mfg_sample_categorical's arithmetic on the row's logits
  if (tid < TILE) {
    const int64_t q = row0 + tid;
    if (q < p.rows_per_group) {
      int64_t b; int i;
      row_env_agent(p.g, A, q, b, i);
      const int64_t row = b * A + i;
      float* l = bufB + tid * lsB;
      const int n_act = p.n_act[net];
      if (p.logits_out)  // the raw logits, before the mask touches the row
        for (int a = 0; a < NM; a++) p.logits_out[row * NM + a] = l[a];
      int pick = -1;
      if (n_act >= 1 && n_act <= NM) {
        // masked acting: the cleared bits' logits become -inf in this row's LDS copy (only this thread reads it from
        // here on), unless the word has no bit set among the row's n_act
        if (p.mask) {
          const uint32_t m = p.mask[row] & (n_act >= 32 ? 0xFFFFFFFFu : (1u << n_act) - 1u);
          if (m)
            for (int a = 0; a < n_act; a++)
              if (!((m >> a) & 1)) l[a] = -INFINITY;
        }
        float mx, s;
        row_max_expsum(l, n_act, mx, s);
        if (s > 0.0f && !isinf(s)) pick = row_pick(l, n_act, mx, s, p.greedy != 0, p.greedy ? 0.0f : p.u[row]);
      }
      p.act_out[row] = pick;
    }
  }
}

// ---- the episode fold: one thread per env
__global__ void __launch_bounds__(256) k_eval_fold(const double* __restrict__ reward, const uint8_t* __restrict__ done,
                                                   int64_t n_envs, int A, int n_episodes, float* __restrict__ eps_rew,
                                                   int32_t* __restrict__ len, int32_t* __restrict__ count,
                                                   float* __restrict__ rows, int32_t* __restrict__ lengths,
                                                   int32_t* __restrict__ finished) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= n_envs) return;
  float* e = eps_rew + b * A;
  const double* rw = reward + b * A;
  const bool d = done[b] != 0;
  const int k = count[b];
  const bool store = d && k >= 0 && k < n_episodes;
  float* out = rows + (b * n_episodes + (store ? k : 0)) * (int64_t)(A + 1);
  float sum = 0.0f;
  for (int i = 0; i < A; i++) {
    const float v = e[i] + (float)rw[i];
    sum = sum + v;
    if (store) out[i] = v;
    e[i] = d ? 0.0f : v;
  }
  const int n = len[b] + 1;
  len[b] = d ? 0 : n;
  if (store) {
    out[A] = sum;
    lengths[b * n_episodes + k] = n;
    count[b] = k + 1;
    if (k + 1 == n_episodes) atomicAdd(finished, 1);
  }
}

}  // namespace

extern "C" int mfg_policy_act_masked(const float* emb, int64_t emb_env, int64_t emb_agent, int64_t n_envs, int n_agents,
                                     int g, int e_dim, int ae_dim, int hd, int n_max, const mfg_actor_weights* w,
                                     const int32_t* n_act, const int32_t* prev_action, const uint8_t* prev_done,
                                     float* h, int64_t h_env, int64_t h_agent, const float* u, int greedy,
                                     const uint32_t* mask, int32_t* act_out, float* logits_out, void* stream) {
  if (!emb || !w || !n_act || !h || !act_out || (!greedy && !u)) return -1;
  if (n_envs <= 0 || n_agents <= 0 || (g != 1 && g != n_agents)) return -1;
  if (e_dim < 1 || e_dim > MAX_E || ae_dim < 1 || ae_dim > MAX_AE || hd < 1 || hd > MAX_H || n_max < 1 ||
      n_max > MAX_ACT)
    return -1;
  if (n_envs > (INT64_MAX / 4) / n_agents) return -1;
  ActArgs a;
  a.emb = emb; a.emb_env = emb_env; a.emb_agent = emb_agent;
  a.n_envs = n_envs; a.n_agents = n_agents; a.g = g; a.E = e_dim; a.AE = ae_dim; a.H = hd; a.n_max = n_max;
  a.w = *w;
  a.n_act = n_act; a.prev_action = prev_action; a.prev_done = prev_done;
  a.h = h; a.h_env = h_env; a.h_agent = h_agent;
  a.u = u; a.greedy = greedy; a.mask = mask; a.act_out = act_out; a.logits_out = logits_out;
  a.rows_per_group = g > 1 ? n_envs : n_envs * n_agents;
  const int64_t nbx = (a.rows_per_group + TILE - 1) / TILE;
  const int nby = g > 1 ? n_agents : 1;
  if (nbx > INT32_MAX || nby > 65535) return -1;
  const int wide = e_dim > hd ? (e_dim > n_max ? e_dim : n_max) : (hd > n_max ? hd : n_max);
  const int first = e_dim + ae_dim > hd ? e_dim + ae_dim : hd;
  const size_t lds = (size_t)TILE * (pad4(first) + pad4(wide) + pad4(hd)) * sizeof(float);
  hipLaunchKernelGGL(k_policy_act, dim3((unsigned)nbx, (unsigned)nby), dim3(256), lds, (hipStream_t)stream, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

// the NULL-mask case of the same kernel
extern "C" int mfg_policy_act(const float* emb, int64_t emb_env, int64_t emb_agent, int64_t n_envs, int n_agents, int g,
                              int e_dim, int ae_dim, int hd, int n_max, const mfg_actor_weights* w,
                              const int32_t* n_act, const int32_t* prev_action, const uint8_t* prev_done, float* h,
                              int64_t h_env, int64_t h_agent, const float* u, int greedy, int32_t* act_out,
                              float* logits_out, void* stream) {
  return mfg_policy_act_masked(emb, emb_env, emb_agent, n_envs, n_agents, g, e_dim, ae_dim, hd, n_max, w, n_act,
                               prev_action, prev_done, h, h_env, h_agent, u, greedy, nullptr, act_out, logits_out,
                               stream);
}

extern "C" int mfg_eval_fold(const double* reward, const uint8_t* done, int64_t n_envs, int n_agents, int n_episodes,
                             float* eps_rew, int32_t* len, int32_t* count, float* rows, int32_t* lengths,
                             int32_t* finished, void* stream) {
  if (!reward || !done || !eps_rew || !len || !count || !rows || !lengths || !finished) return -1;
  if (n_envs <= 0 || n_agents <= 0 || n_episodes <= 0) return -1;
  hipLaunchKernelGGL(k_eval_fold, dim3((unsigned)((n_envs + 255) / 256)), dim3(256), 0, (hipStream_t)stream, reward,
                     done, n_envs, n_agents, n_episodes, eps_rew, len, count, rows, lengths, finished);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}
