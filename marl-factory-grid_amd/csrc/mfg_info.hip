// mfg_info.hip — the batched episode monitor (C-ABI of include/mfg_info.h): the info program evaluated per env-step
// and folded per episode on the device, from the buffers an mfg_step call wrote.
//
// Execution model (as the engine's, mfg_device.h): one wavefront per env, MFG_INFO_WPB waves per workgroup, no
// workgroup barrier (B need not be a multiple of the waves per workgroup). Lanes stride over the columns
// (key = lane, lane + 64, ...); each lane walks its key's CSR op list with the shared evaluation function
// (mfg_info_eval.h). A step's event rows, actions and rewards are loaded once per wave (two 64-lane passes for more
// than 64 agents) and read back from LDS. The K loop of a fused call runs inside the kernel: the env's accumulators
// are read before k = 0 and written after k = K - 1, in registers for up to MFG_INFO_KPL_MAX keys per lane, else in
// the wave's LDS slice. The program (ops, CSR, action table) stays in HBM: every wave reads the same few KiB, so it
// lives in L2 / the vector L1 (cap_dest81's action table alone is 101 KiB, past any LDS staging).
#define MFG_OBS_UNIT  // mfg_kernels.h for philox_u32 and the wave primitives only: none of its kernels
#include "mfg_kernels.h"
#include "mfg_info_eval.h"

#define MFG_INFO_WPB 4      // waves (envs) per workgroup
#define MFG_INFO_KPL_MAX 4  // keys per lane held in registers; more columns than 64 * this: LDS accumulators
#define MFG_INFO_LDS_BUDGET (56 * 1024)  // dynamic LDS per workgroup of the LDS-accumulator kernel

int mfg_internal_fail(const char* msg);  // mfg_engine.hip: sets the last-error string, returns -1

namespace {

int ifail(const std::string& m) { return mfg_internal_fail(m.c_str()); }
#define INFO_HIPCHK(x)                                                                   \
  do {                                                                                   \
    hipError_t _e = (x);                                                                 \
    if (_e != hipSuccess) return ifail(std::string(#x) + ": " + hipGetErrorString(_e));   \
  } while (0)

struct DevScope {
  int prev = -1;
  explicit DevScope(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
  }
  ~DevScope() {
    int cur = -1;
    if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) (void)hipSetDevice(prev);
  }
};

// what the kernels need, by value
struct InfoDev {
  MfgInfoProg P;            // device pointers
  const int32_t* n_actions; // [A]
  long long B, cap;
  int Kc;
  double* acc;              // [B][Kc]
  uint32_t* cnt;            // [B][Kc]
  int32_t* len;             // [B]
  int32_t* ep_index;        // [B]
  uint32_t* counter;        // finished-episode rows claimed
  int32_t* ep_hdr;          // [cap][MFG_INFO_HDR_N]
  double* ep_sum;           // [cap][Kc]
  uint32_t* ep_cnt;         // [cap][Kc]
};

// one wave's staged step
struct InfoRows {
  double rew[MFG_MAX_AGENTS];
  int32_t misc[MFG_EV_MISC_N];
  uint8_t act[MFG_MAX_AGENTS], watch[MFG_MAX_AGENTS], slot[MFG_MAX_AGENTS];
};

template <int KPL, typename F>
__device__ __forceinline__ void for_keys(int lane, int Kc, F f) {
  if constexpr (KPL > 0) {
#pragma unroll
    for (int j = 0; j < KPL; j++) {
      const int key = j * MFG_WAVE + lane;
      if (key < Kc) f(j, key);
    }
  } else {
    for (int key = lane; key < Kc; key += MFG_WAVE) f(0, key);
  }
}

// KPL > 0: Kc <= 64 * KPL, accumulators in registers; KPL == 0: in the wave's dynamic LDS slice (lds_stride bytes:
// acc f64 [Kc] then cnt u32 [Kc])
template <int KPL>
__global__ void __launch_bounds__(MFG_INFO_WPB * MFG_WAVE)
k_info_step(InfoDev D, int K, const int32_t* __restrict__ actions, uint32_t philox_seed, uint32_t env_base,
            long long step_base, const uint8_t* __restrict__ ev_act, const uint8_t* __restrict__ ev_watch,
            const int32_t* __restrict__ ev_misc, const double* __restrict__ reward, const uint8_t* __restrict__ done,
            double* __restrict__ vals, uint8_t* __restrict__ pres, int lds_stride) {
  __shared__ InfoRows rows_all[MFG_INFO_WPB];
  extern __shared__ double dyn_lds[];
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
  const long long env = (long long)blockIdx.x * (long long)(blockDim.x >> 6) + wave;
  if (env >= D.B) return;  // whole waves leave: nothing below synchronises across waves
  InfoRows& R = rows_all[wave];
  const int Kc = D.Kc, A = D.P.n_agents;
  const size_t erow = (size_t)env * (size_t)Kc;

  constexpr int NR = KPL > 0 ? KPL : 1;
  double acc_r[NR];
  uint32_t cnt_r[NR];
  double* lacc = nullptr;
  uint32_t* lcnt = nullptr;
  if constexpr (KPL == 0) {
    lacc = (double*)((uint8_t*)dyn_lds + (size_t)wave * (size_t)lds_stride);
    lcnt = (uint32_t*)(lacc + Kc);
  }
#pragma unroll
  for (int j = 0; j < NR; j++) { acc_r[j] = 0.0; cnt_r[j] = 0u; }
  for_keys<KPL>(lane, Kc, [&](int j, int key) {
    const double a = D.acc[erow + key];
    const uint32_t c = D.cnt[erow + key];
    if constexpr (KPL > 0) { acc_r[j] = a; cnt_r[j] = c; } else { lacc[key] = a; lcnt[key] = c; }
  });
  int len = uni(D.len[env]);
  int epi = uni(D.ep_index[env]);

  for (int k = 0; k < K; k++) {
    const size_t kb = (size_t)k * (size_t)D.B + (size_t)env;
    wave_sync();  // the previous step's reads of the staged rows are done
#pragma unroll
    for (int h = 0; h < MFG_MAX_AGENTS / MFG_WAVE; h++) {
      const int a = h * MFG_WAVE + lane;
      if (a < A) {
        const int na = D.n_actions[a];
        int s;
        if (actions) {
          s = actions[kb * A + a];
        } else {
          const uint32_t u = philox_u32(philox_seed, env_base + (uint32_t)env, (uint32_t)(step_base + k), (uint32_t)a);
          s = (int)(((uint64_t)u * (uint64_t)na) >> 32);
        }
        s = s < 0 ? 0 : (s > na - 1 ? na - 1 : s);
        R.slot[a] = (uint8_t)s;
        R.act[a] = ev_act[kb * A + a];
        R.watch[a] = ev_watch[kb * A + a];
        R.rew[a] = reward[kb * A + a];
      }
    }
    if (lane < MFG_EV_MISC_N) R.misc[lane] = ev_misc[kb * MFG_EV_MISC_N + lane];
    wave_sync();
    const bool crashed = (uni(R.misc[MFG_EVM_FLAGS]) & 2) != 0;
    const bool fin = crashed || uni((int)done[kb]) != 0;
    for_keys<KPL>(lane, Kc, [&](int j, int key) {
      double v = 0.0;
      bool p = false;
      if (!crashed) p = mfg_info_eval_key(D.P, key, R.slot, R.act, R.watch, R.misc, R.rew, &v);
      if (vals) vals[kb * Kc + key] = p ? v : 0.0;
      if (pres) pres[kb * Kc + key] = p ? 1 : 0;
      if (p) {
        if constexpr (KPL > 0) { acc_r[j] = acc_r[j] + v; cnt_r[j] += 1u; } else { lacc[key] = lacc[key] + v; lcnt[key] += 1u; }
      }
    });
    len += 1;
    if (fin) {
      // one row of the finished-episode buffer, claimed with one atomic add per episode; past the capacity only the
      // counter moves
      uint32_t idx = 0;
      if (lane == 0) idx = atomicAdd(D.counter, 1u);
      idx = (uint32_t)uni((int)idx);
      const bool keep = (long long)idx < D.cap;
      if (keep && lane < MFG_INFO_HDR_N) {
        int h = 0;
        if (lane == MFG_INFO_HDR_ENV) h = (int)env;
        if (lane == MFG_INFO_HDR_EP_INDEX) h = epi;
        if (lane == MFG_INFO_HDR_LENGTH) h = len;
        if (lane == MFG_INFO_HDR_CRASHED) h = crashed ? 1 : 0;
        if (lane == MFG_INFO_HDR_MAINT_BASE) h = R.misc[MFG_EVM_MAINT_BASE];
        D.ep_hdr[(size_t)idx * MFG_INFO_HDR_N + lane] = h;
      }
      const size_t rrow = (size_t)idx * (size_t)Kc;
      for_keys<KPL>(lane, Kc, [&](int j, int key) {
        if constexpr (KPL > 0) {
          if (keep) { D.ep_sum[rrow + key] = acc_r[j]; D.ep_cnt[rrow + key] = cnt_r[j]; }
          acc_r[j] = 0.0;
          cnt_r[j] = 0u;
        } else {
          if (keep) { D.ep_sum[rrow + key] = lacc[key]; D.ep_cnt[rrow + key] = lcnt[key]; }
          lacc[key] = 0.0;
          lcnt[key] = 0u;
        }
      });
      len = 0;
      epi += 1;
    }
  }
  for_keys<KPL>(lane, Kc, [&](int j, int key) {
    if constexpr (KPL > 0) {
      D.acc[erow + key] = acc_r[j];
      D.cnt[erow + key] = cnt_r[j];
    } else {
      D.acc[erow + key] = lacc[key];
      D.cnt[erow + key] = lcnt[key];
    }
  });
  if (lane == 0) {
    D.len[env] = len;
    D.ep_index[env] = epi;
  }
}

// acc / cnt / len of the masked envs to 0: one thread per (env, column)
__global__ void __launch_bounds__(256) k_info_reset(InfoDev D, const uint8_t* __restrict__ mask) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= D.B * D.Kc) return;
  const long long env = i / D.Kc;
  if (mask && !mask[env]) return;
  D.acc[i] = 0.0;
  D.cnt[i] = 0u;
  if (i - env * D.Kc == 0) D.len[env] = 0;
}

}  // namespace

struct mfg_info {
  int device = 0;
  int kpl = 0, wpb = MFG_INFO_WPB, lds_stride = 0;
  InfoDev d{};
  std::vector<void*> bufs;
};

namespace {

template <typename T>
int dev_alloc(mfg_info* h, size_t n, T** out, const T* src = nullptr) {
  void* p = nullptr;
  const size_t bytes = sizeof(T) * (n ? n : 1);
  INFO_HIPCHK(hipMalloc(&p, bytes));
  h->bufs.push_back(p);
  if (src && n) {
    INFO_HIPCHK(hipMemcpy(p, src, sizeof(T) * n, hipMemcpyHostToDevice));
  } else {
    INFO_HIPCHK(hipMemset(p, 0, bytes));
  }
  *out = (T*)p;
  return 0;
}

int create_impl(mfg_info* h, const mfg_info_op* ops, int n_ops, const int32_t* key_off, int n_keys,
                const double* action_table, int n_agents, const int32_t* n_actions, double noop_cost, int dest_max) {
  InfoDev& d = h->d;
  const size_t B = (size_t)d.B, cap = (size_t)d.cap, Kc = (size_t)d.Kc;
  mfg_info_op* d_ops = nullptr;
  int32_t *d_off = nullptr, *d_na = nullptr;
  double* d_tab = nullptr;
  if (dev_alloc(h, (size_t)n_ops, &d_ops, ops) || dev_alloc(h, (size_t)n_keys + 1, &d_off, key_off) ||
      dev_alloc(h, (size_t)n_agents * MFG_MAX_ACTIONS * MFG_INFO_ATAB_N, &d_tab, action_table) ||
      dev_alloc(h, (size_t)n_agents, &d_na, n_actions))
    return -1;
  d.P = MfgInfoProg{d_ops, d_off, d_tab, n_keys, n_agents, noop_cost, dest_max};
  d.n_actions = d_na;
  if (dev_alloc(h, B * Kc, &d.acc) || dev_alloc(h, B * Kc, &d.cnt) || dev_alloc(h, B, &d.len) ||
      dev_alloc(h, B, &d.ep_index) || dev_alloc(h, 1, &d.counter) || dev_alloc(h, cap * MFG_INFO_HDR_N, &d.ep_hdr) ||
      dev_alloc(h, cap * Kc, &d.ep_sum) || dev_alloc(h, cap * Kc, &d.ep_cnt))
    return -1;
  return 0;
}

}  // namespace

extern "C" int mfg_info_create(const mfg_info_op* ops, int n_ops, const int32_t* key_off, int n_keys,
                               const double* action_table, int n_agents, const int32_t* n_actions, double noop_cost,
                               int dest_max, int device, int64_t n_envs, int64_t ep_capacity, mfg_info** out) {
  if (!out) return ifail("null argument");
  *out = nullptr;
  const std::string bad = mfg_info_check_program(ops, n_ops, key_off, n_keys, action_table, n_agents, n_actions, dest_max);
  if (!bad.empty()) return ifail("mfg_info_create: " + bad);
  if (n_envs < 1 || n_envs > (int64_t)1 << 30) return ifail("mfg_info_create: n_envs out of range");
  if (ep_capacity < 1 || ep_capacity > (int64_t)1 << 30) return ifail("mfg_info_create: ep_capacity out of range");
  int n_dev = 0;
  if (hipGetDeviceCount(&n_dev) != hipSuccess || device < 0 || device >= n_dev)
    return ifail("mfg_info_create: no such HIP device");
  mfg_info* h = new mfg_info();
  h->device = device;
  h->d.B = n_envs;
  h->d.cap = ep_capacity;
  const int Kc = n_keys + 2;
  h->d.Kc = Kc;
  h->kpl = Kc <= MFG_WAVE ? 1 : Kc <= 2 * MFG_WAVE ? 2 : Kc <= MFG_INFO_KPL_MAX * MFG_WAVE ? 4 : 0;
  if (h->kpl == 0) {
    h->lds_stride = (Kc * 12 + 7) & ~7;
    h->wpb = std::max(1, std::min(MFG_INFO_WPB, MFG_INFO_LDS_BUDGET / h->lds_stride));
  }
  DevScope g(device);
  if (create_impl(h, ops, n_ops, key_off, n_keys, action_table, n_agents, n_actions, noop_cost, dest_max)) {
    for (void* p : h->bufs) (void)hipFree(p);
    delete h;
    return -1;
  }
  *out = h;
  return 0;
}

extern "C" int mfg_info_destroy(mfg_info* h) {
  if (!h) return 0;
  DevScope g(h->device);
  for (void* p : h->bufs) (void)hipFree(p);
  delete h;
  return 0;
}

extern "C" int mfg_info_config(const mfg_info* h, int32_t* out) {
  if (!h || !out) return ifail("null argument");
  out[0] = h->d.Kc;
  out[1] = h->kpl;
  out[2] = h->wpb;
  out[3] = (int32_t)(MFG_INFO_WPB * sizeof(InfoRows)) + (h->kpl ? 0 : h->wpb * h->lds_stride);
  return 0;
}

extern "C" int mfg_info_step(mfg_info* h, int K, const int32_t* actions, uint32_t philox_seed, uint32_t env_base,
                             int64_t step_base, const uint8_t* ev_act, const uint8_t* ev_watch,
                             const int32_t* ev_misc, const double* reward, const uint8_t* done, double* vals,
                             uint8_t* pres, void* stream) {
  if (!h) return ifail("null info handle");
  if (K < 1) return ifail("mfg_info_step: K must be >= 1");
  if (!ev_act || !ev_watch || !ev_misc || !reward || !done)
    return ifail("mfg_info_step: ev_act, ev_watch, ev_misc, reward and done are required");
  DevScope g(h->device);
  hipStream_t st = (hipStream_t)stream;
  const unsigned blocks = (unsigned)((h->d.B + h->wpb - 1) / h->wpb);
  const dim3 grid(blocks), block((unsigned)(h->wpb * MFG_WAVE));
#define INFO_LAUNCH(KPL, LDS)                                                                                       \
  hipLaunchKernelGGL((k_info_step<KPL>), grid, block, (size_t)(LDS), st, h->d, K, actions, philox_seed, env_base,    \
                     (long long)step_base, ev_act, ev_watch, ev_misc, reward, done, vals, pres, h->lds_stride)
  switch (h->kpl) {
    case 1: INFO_LAUNCH(1, 0); break;
    case 2: INFO_LAUNCH(2, 0); break;
    case 4: INFO_LAUNCH(4, 0); break;
    default: INFO_LAUNCH(0, (size_t)h->wpb * (size_t)h->lds_stride); break;
  }
#undef INFO_LAUNCH
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return ifail(std::string("k_info_step launch: ") + hipGetErrorString(err));
  return 0;
}

extern "C" int mfg_info_episodes(mfg_info* h, uint32_t* out_count, void* stream) {
  if (!h || !out_count) return ifail("null argument");
  DevScope g(h->device);
  hipStream_t st = (hipStream_t)stream;
  INFO_HIPCHK(hipMemcpyAsync(out_count, h->d.counter, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  INFO_HIPCHK(hipStreamSynchronize(st));
  return 0;
}

extern "C" int mfg_info_rows(const mfg_info* h, const int32_t** hdr, const double** sum, const uint32_t** count) {
  if (!h) return ifail("null info handle");
  if (hdr) *hdr = h->d.ep_hdr;
  if (sum) *sum = h->d.ep_sum;
  if (count) *count = h->d.ep_cnt;
  return 0;
}

extern "C" int mfg_info_drain(mfg_info* h, int64_t max_rows, int32_t* hdr_out, double* sum_out, uint32_t* count_out,
                              uint32_t* out_count, void* stream) {
  if (!h || !out_count) return ifail("null argument");
  if (max_rows < 0) return ifail("mfg_info_drain: max_rows must be >= 0");
  DevScope g(h->device);
  hipStream_t st = (hipStream_t)stream;
  INFO_HIPCHK(hipMemcpyAsync(out_count, h->d.counter, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  INFO_HIPCHK(hipStreamSynchronize(st));
  const size_t n = (size_t)std::min<long long>(std::min<long long>((long long)*out_count, h->d.cap), (long long)max_rows);
  const size_t Kc = (size_t)h->d.Kc;
  if (n && hdr_out)
    INFO_HIPCHK(hipMemcpyAsync(hdr_out, h->d.ep_hdr, n * MFG_INFO_HDR_N * sizeof(int32_t), hipMemcpyDeviceToHost, st));
  if (n && sum_out) INFO_HIPCHK(hipMemcpyAsync(sum_out, h->d.ep_sum, n * Kc * sizeof(double), hipMemcpyDeviceToHost, st));
  if (n && count_out)
    INFO_HIPCHK(hipMemcpyAsync(count_out, h->d.ep_cnt, n * Kc * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  INFO_HIPCHK(hipMemsetAsync(h->d.counter, 0, sizeof(uint32_t), st));
  INFO_HIPCHK(hipStreamSynchronize(st));
  return 0;
}

extern "C" int mfg_info_reset(mfg_info* h, const uint8_t* mask, void* stream) {
  if (!h) return ifail("null info handle");
  DevScope g(h->device);
  const long long n = h->d.B * h->d.Kc;
  hipLaunchKernelGGL(k_info_reset, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, h->d, mask);
  const hipError_t err = hipGetLastError();
  if (err != hipSuccess) return ifail(std::string("k_info_reset launch: ") + hipGetErrorString(err));
  return 0;
}

extern "C" int mfg_info_eval_host(const mfg_info_op* ops, int n_ops, const int32_t* key_off, int n_keys,
                                  const double* action_table, int n_agents, const int32_t* n_actions,
                                  double noop_cost, int dest_max, const int32_t* actions, const uint8_t* ev_act,
                                  const uint8_t* ev_watch, const int32_t* ev_misc, const double* reward, double* vals,
                                  uint8_t* pres) {
  const std::string bad = mfg_info_check_program(ops, n_ops, key_off, n_keys, action_table, n_agents, n_actions, dest_max);
  if (!bad.empty()) return ifail("mfg_info_eval_host: " + bad);
  if (!actions || !ev_act || !ev_watch || !ev_misc || !reward || !vals || !pres) return ifail("null argument");
  const MfgInfoProg P{ops, key_off, action_table, n_keys, n_agents, noop_cost, dest_max};
  uint8_t slot[MFG_MAX_AGENTS];
  mfg_info_clamp_slots(actions, n_actions, n_agents, slot);
  const bool crashed = (ev_misc[MFG_EVM_FLAGS] & 2) != 0;
  for (int key = 0; key < n_keys + 2; key++) {
    double v = 0.0;
    bool p = false;
    if (!crashed) p = mfg_info_eval_key(P, key, slot, ev_act, ev_watch, ev_misc, reward, &v);
    vals[key] = p ? v : 0.0;
    pres[key] = p ? 1 : 0;
  }
  return 0;
}
