// mfg_record.hip — the batched state recorder (C-ABI of include/mfg_record.h): per-step state rows of the selected
// envs and the agents' cell-visit counts of the whole batch, from the env records and the buffers of one K = 1
// mfg_step call made without auto-reset.
//
// The unit knows the engine only through mfg_layout / mfg_state_ptr / mfg_state_bytes (include/mfg.h); mfg_device.h
// gives the header slots and the entity-word bits. Two kernels per step:
//  * k_record_rows: one wavefront per SELECTED env, MFG_REC_WPB waves per workgroup, no workgroup barrier. The wave
//    reads its env's episode number, tests it against the episode filter, takes the next index of the env's row
//    counter (one wave owns one counter: a plain read-modify-write by lane 0) and, below capacity, writes the row.
//    Lanes stride over the agents, doors and item slots (i = lane, lane + 64, ...), so specs with more than 64 of
//    any of them take further passes of the same loops.
//  * k_record_occ: a workgroup of MFG_REC_OCC_THREADS threads covers a chunk of consecutive envs; its threads stride
//    over the chunk's (env, agent) pairs. LDS: the cells are counted into a u32 histogram of H * W bins with LDS
//    atomics, and only the nonzero bins are flushed with one 64-bit global atomic add each. GLOBAL (levels whose
//    histogram does not fit the LDS budget): every pair adds straight to the u64 map. Integer adds commute, so the
//    map does not depend on arrival order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "mfg_device.h"
#include "../../include/mfg_record.h"

#define MFG_REC_WPB 4               // row kernel: waves (selected envs) per workgroup
#define MFG_REC_OCC_THREADS 256     // occupancy kernel: threads per workgroup
#define MFG_REC_OCC_MIN_ENVS 32     // ... envs per workgroup at least (small batches still take several workgroups)
#define MFG_REC_OCC_GRID 512        // ... workgroups aimed at for large batches (two per CU)
#define MFG_REC_OCC_LDS_CELLS 8192  // LDS histogram budget: 32 KiB of u32 bins, several workgroups per CU
#define MFG_REC_LAYOUT_MIN 27       // mfg_layout ints this unit reads (through o_machines)

int mfg_internal_fail(const char* msg);  // mfg_engine.hip: sets the last-error string, returns -1

namespace {

int rfail(const std::string& m) { return mfg_internal_fail(m.c_str()); }
#define REC_HIPCHK(x)                                                                    \
  do {                                                                                   \
    hipError_t _e = (x);                                                                 \
    if (_e != hipSuccess) return rfail(std::string(#x) + ": " + hipGetErrorString(_e));   \
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
struct RecDev {
  const uint8_t* state;      // [B][rec_size] env records
  long long B, n_sel, cap;
  int rec_size, o_hdr, o_agent_pos, o_battery, o_door, o_items;  // record offsets (bytes)
  int A, nd, imax, HW, has_bat;
  int row_words, o_cell, o_act, o_bat, o_rdoor, o_ritems;        // row offsets (words)
  const int32_t* envs;       // [n_sel]
  const int32_t* episodes;   // [n_ep]
  int n_ep;
  uint32_t* rows;            // [n_sel][cap][row_words]
  uint32_t* counters;        // [n_sel]
  unsigned long long* occ;   // [HW]
  int occ_envs;              // envs per workgroup of k_record_occ
};

__global__ void __launch_bounds__(MFG_REC_WPB * MFG_WAVE)
k_record_rows(RecDev D, const int32_t* __restrict__ actions, const uint8_t* __restrict__ ev_act,
              const uint8_t* __restrict__ ev_watch, const int32_t* __restrict__ ev_misc,
              const uint8_t* __restrict__ done) {
  const int wave = (int)(threadIdx.x >> 6), lane = (int)(threadIdx.x & 63);
  const long long sel = (long long)blockIdx.x * MFG_REC_WPB + wave;
  if (sel >= D.n_sel) return;  // whole waves leave: nothing below synchronises across waves
  const long long env = D.envs[sel];
  if (env < 0 || env >= D.B) return;  // (checked at create)
  const uint8_t* rec = D.state + (size_t)env * (size_t)D.rec_size;
  const int32_t* hdr = (const int32_t*)(rec + D.o_hdr);
  const int episode = hdr[H_EPISODE] + 1;  // 1-based (the slot is 0 in the first episode); every lane reads the same word
  if (D.n_ep > 0) {
    bool hit = false;
    for (int i = lane; i < D.n_ep; i += MFG_WAVE) hit |= D.episodes[i] == episode;
    if (!__any(hit)) return;
  }
  // the env's next row index; the counter keeps counting past the capacity, the row is then dropped
  uint32_t idx = 0;
  if (lane == 0) {
    idx = D.counters[sel];
    D.counters[sel] = idx + 1u;
  }
  idx = (uint32_t)__shfl((int)idx, 0);
  if ((long long)idx >= D.cap) return;
  uint32_t* row = D.rows + ((size_t)sel * (size_t)D.cap + (size_t)idx) * (size_t)D.row_words;
  const int A = D.A;
  if (lane == 0) row[0] = (uint32_t)env;
  if (lane == 1) row[1] = (uint32_t)episode;
  if (lane == 2) row[2] = (uint32_t)hdr[H_STEP];
  if (lane == 3) {
    const uint32_t crashed = ((uint32_t)ev_misc[(size_t)env * MFG_EV_MISC_N + MFG_EVM_FLAGS] >> 1) & 1u;
    row[3] = (done[env] ? 1u : 0u) | (crashed << 1);
  }
  const int32_t* apos = (const int32_t*)(rec + D.o_agent_pos);
  for (int a = lane; a < A; a += MFG_WAVE) {
    const size_t ea = (size_t)env * (size_t)A + (size_t)a;
    row[D.o_cell + a] = (uint32_t)apos[a];
    row[D.o_act + a] = ((uint32_t)actions[ea] & 0xFFu) | ((uint32_t)ev_act[ea] << 8) | ((uint32_t)ev_watch[ea] << 16);
  }
  if (D.has_bat) {
    const uint32_t* bat = (const uint32_t*)(rec + D.o_battery);  // f64 [A] as word pairs
    for (int i = lane; i < 2 * A; i += MFG_WAVE) row[D.o_bat + i] = bat[i];
  }
  const uint32_t* door = (const uint32_t*)(rec + D.o_door);
  for (int d = lane; d < D.nd; d += MFG_WAVE) row[D.o_rdoor + d] = door[d];
  if (lane == 0) row[D.o_ritems] = (uint32_t)hdr[H_N_ITEMS];
  if (lane == 1) row[D.o_ritems + 1] = (uint32_t)hdr[H_ITEM_BASE];
  const uint32_t* items = (const uint32_t*)(rec + D.o_items);
  for (int k = lane; k < D.imax; k += MFG_WAVE) row[D.o_ritems + 2 + k] = items[k];
}

// LDS: the workgroup's u32 histogram in dynamic LDS (4 * HW bytes); else straight to global memory
template <bool LDS>
__global__ void __launch_bounds__(MFG_REC_OCC_THREADS) k_record_occ(RecDev D) {
  extern __shared__ __attribute__((aligned(16))) uint32_t hist[];
  const int HW = D.HW, A = D.A;
  if constexpr (LDS) {
    for (int c = (int)threadIdx.x; c < HW; c += MFG_REC_OCC_THREADS) hist[c] = 0u;
    __syncthreads();
  }
  const long long e0 = (long long)blockIdx.x * D.occ_envs;
  const long long ne = min((long long)D.occ_envs, D.B - e0);  // > 0: the grid is ceil(B / occ_envs)
  const long long n = ne * A;
  for (long long i = threadIdx.x; i < n; i += MFG_REC_OCC_THREADS) {
    const long long env = e0 + i / A;
    const int a = (int)(i % A);
    const int32_t cell = ((const int32_t*)(D.state + (size_t)env * (size_t)D.rec_size + D.o_agent_pos))[a];
    if (cell < 0 || cell >= HW) continue;  // never outside the map
    if constexpr (LDS) {
      atomicAdd(&hist[cell], 1u);
    } else {
      atomicAdd(&D.occ[cell], 1ull);
    }
  }
  if constexpr (LDS) {
    __syncthreads();
    for (int c = (int)threadIdx.x; c < HW; c += MFG_REC_OCC_THREADS) {
      const uint32_t v = hist[c];
      if (v) atomicAdd(&D.occ[c], (unsigned long long)v);
    }
  }
}

}  // namespace

struct mfg_record {
  int device = 0;
  RecDev d{};
  int occ_path = MFG_RECORD_OCC_OFF;
  unsigned row_grid = 0, occ_grid = 0;
  std::vector<void*> bufs;
  std::vector<uint32_t> h_counts;  // drain scratch
};

namespace {

template <typename T>
int dev_alloc(mfg_record* h, size_t n, T** out, const T* src = nullptr) {
  void* p = nullptr;
  const size_t bytes = sizeof(T) * (n ? n : 1);
  REC_HIPCHK(hipMalloc(&p, bytes));
  h->bufs.push_back(p);
  REC_HIPCHK(hipMemset(p, 0, bytes));
  if (src && n) REC_HIPCHK(hipMemcpy(p, src, sizeof(T) * n, hipMemcpyHostToDevice));
  *out = (T*)p;
  return 0;
}

int create_impl(mfg_record* h, const int32_t* envs, const int32_t* episodes, int occupancy) {
  RecDev& d = h->d;
  int32_t *d_envs = nullptr, *d_eps = nullptr;
  if (dev_alloc(h, (size_t)d.n_sel, &d_envs, envs) || dev_alloc(h, (size_t)d.n_ep, &d_eps, episodes)) return -1;
  d.envs = d_envs;
  d.episodes = d_eps;
  if (dev_alloc(h, (size_t)d.n_sel * (size_t)d.cap * (size_t)d.row_words, &d.rows) ||
      dev_alloc(h, (size_t)d.n_sel, &d.counters) || dev_alloc(h, occupancy ? (size_t)d.HW : 0, &d.occ))
    return -1;
  return 0;
}

}  // namespace

extern "C" int mfg_record_create(mfg_engine* e, const mfg_spec* spec, const int32_t* envs, int64_t n_sel,
                                 int64_t capacity, const int32_t* episodes, int n_ep, int occupancy,
                                 int occ_lds_cells, mfg_record** out) {
  if (!out) return rfail("null argument");
  *out = nullptr;
  if (!e || !spec) return rfail("mfg_record_create: the engine and its spec are required");
  int32_t lay[64] = {0};
  const int n_lay = mfg_layout(e, lay);
  if (n_lay < MFG_REC_LAYOUT_MIN) return rfail("mfg_record_create: mfg_layout reports too few entries");
  // mfg_layout: [size, o_hdr, o_rule_ctr, o_agent_pos, o_agent_arr, o_agent_par, o_frozen_org, o_frozen_gp, o_door,
  //              o_items, o_pods, ..., o_battery (15), o_frozen_bat (16), ...]
  const int size = lay[0], o_hdr = lay[1], o_agent_pos = lay[3], o_agent_arr = lay[4], o_door = lay[8],
            o_items = lay[9], o_pods = lay[10], o_battery = lay[15];
  uint8_t* state = (uint8_t*)mfg_state_ptr(e);
  const int64_t bytes = mfg_state_bytes(e);
  if (!state || size < 16 || bytes < size || bytes % size) return rfail("mfg_record_create: the engine has no state records");
  const int64_t B = bytes / size;
  const int A = spec->n_agents, nd = spec->n_doors;
  if (A < 1 || A > MFG_MAX_AGENTS || o_agent_arr - o_agent_pos != 4 * A)
    return rfail("mfg_record_create: spec.n_agents does not match the engine's record layout");
  if (nd < 0 || nd > MFG_MAX_DOORS || o_items - o_door != 4 * nd)
    return rfail("mfg_record_create: spec.n_doors does not match the engine's record layout");
  const int imax = (o_pods - o_items) / 4;
  if (o_pods < o_items || (o_pods - o_items) % 4 || imax > MFG_MAX_GROUP)
    return rfail("mfg_record_create: item slots of the record layout out of range");
  if (spec->H < 1 || spec->W < 1 || (int64_t)spec->H * spec->W >= EW_NOPOS)
    return rfail("mfg_record_create: level shape out of range");
  if (o_hdr < 0 || o_hdr + 4 * MFG_HDR_N > size || o_agent_pos < 0 || o_pods > size || o_battery < 0 ||
      o_battery + 8 * A > size || o_battery % 8)
    return rfail("mfg_record_create: record layout out of range");
  if (n_sel < 0 || n_sel > B) return rfail("mfg_record_create: n_sel must be 0 .. the engine's env count");
  if (n_sel > 0 && !envs) return rfail("mfg_record_create: envs is required when n_sel > 0");
  if (capacity < 1 || capacity > MFG_RECORD_MAX_CAPACITY)
    return rfail("mfg_record_create: capacity must be 1 .. MFG_RECORD_MAX_CAPACITY");
  if (n_ep < 0 || n_ep > MFG_RECORD_MAX_EPISODES || (n_ep > 0 && !episodes))
    return rfail("mfg_record_create: n_ep must be 0 .. MFG_RECORD_MAX_EPISODES, with episodes given when > 0");
  for (int i = 0; i < n_ep; i++)
    if (episodes[i] < 1) return rfail("mfg_record_create: episode numbers are 1-based");
  if (occupancy != 0 && occupancy != 1) return rfail("mfg_record_create: occupancy must be 0 or 1");
  if (occ_lds_cells < 0) return rfail("mfg_record_create: occ_lds_cells must be >= 0");
  if (n_sel == 0 && !occupancy) return rfail("mfg_record_create: no env selected and occupancy off: nothing to record");
  {
    std::vector<bool> seen((size_t)B, false);
    for (int64_t i = 0; i < n_sel; i++) {
      const int64_t b = envs[i];
      if (b < 0 || b >= B) return rfail("mfg_record_create: env id " + std::to_string(b) + " out of range");
      if (seen[(size_t)b]) return rfail("mfg_record_create: env id " + std::to_string(b) + " is selected twice");
      seen[(size_t)b] = true;
    }
  }
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, state) != hipSuccess)
    return rfail("mfg_record_create: the engine's state records are not device memory");
  mfg_record* h = new mfg_record();
  h->device = attr.device;
  RecDev& d = h->d;
  d.state = state;
  d.B = B; d.n_sel = n_sel; d.cap = capacity;
  d.rec_size = size; d.o_hdr = o_hdr; d.o_agent_pos = o_agent_pos; d.o_battery = o_battery; d.o_door = o_door;
  d.o_items = o_items;
  d.A = A; d.nd = nd; d.imax = imax; d.HW = spec->H * spec->W; d.has_bat = spec->has_batteries ? 1 : 0;
  d.o_cell = 4;
  d.o_act = 4 + A;
  d.o_bat = d.has_bat ? 4 + 2 * A : -1;
  d.o_rdoor = 4 + 2 * A + (d.has_bat ? 2 * A : 0);
  d.o_ritems = d.o_rdoor + nd;
  d.row_words = d.o_ritems + 2 + imax;
  d.n_ep = n_ep;
  if ((double)n_sel * (double)capacity * (double)d.row_words * 4.0 > 64.0 * 1024 * 1024 * 1024) {
    delete h;
    return rfail("mfg_record_create: n_sel * capacity rows exceed 64 GiB");
  }
  h->row_grid = (unsigned)((n_sel + MFG_REC_WPB - 1) / MFG_REC_WPB);
  if (occupancy) {
    const int bound = occ_lds_cells > 0 ? std::min(occ_lds_cells, MFG_REC_OCC_LDS_CELLS) : MFG_REC_OCC_LDS_CELLS;
    h->occ_path = d.HW <= bound ? MFG_RECORD_OCC_LDS : MFG_RECORD_OCC_GLOBAL;
    d.occ_envs = (int)std::max<int64_t>(MFG_REC_OCC_MIN_ENVS, (B + MFG_REC_OCC_GRID - 1) / MFG_REC_OCC_GRID);
    h->occ_grid = (unsigned)((B + d.occ_envs - 1) / d.occ_envs);
  }
  DevScope g(h->device);
  if (create_impl(h, envs, episodes, occupancy)) {
    for (void* p : h->bufs) (void)hipFree(p);
    delete h;
    return -1;
  }
  h->h_counts.resize((size_t)std::max<int64_t>(n_sel, 1));
  *out = h;
  return 0;
}

extern "C" int mfg_record_destroy(mfg_record* h) {
  if (!h) return 0;
  DevScope g(h->device);
  for (void* p : h->bufs) (void)hipFree(p);
  delete h;
  return 0;
}

extern "C" int mfg_record_config(const mfg_record* h, int32_t* out) {
  if (!h || !out) return rfail("null argument");
  const RecDev& d = h->d;
  out[MFG_RECORD_CFG_ROW_WORDS] = d.row_words;
  out[MFG_RECORD_CFG_N_SEL] = (int32_t)d.n_sel;
  out[MFG_RECORD_CFG_CAPACITY] = (int32_t)d.cap;
  out[MFG_RECORD_CFG_ROW_WAVES] = MFG_REC_WPB;
  out[MFG_RECORD_CFG_ROW_GRID] = (int32_t)h->row_grid;
  out[MFG_RECORD_CFG_OCC_THREADS] = MFG_REC_OCC_THREADS;
  out[MFG_RECORD_CFG_OCC_ENVS] = d.occ_envs;
  out[MFG_RECORD_CFG_OCC_GRID] = (int32_t)h->occ_grid;
  out[MFG_RECORD_CFG_OCC_PATH] = h->occ_path;
  out[MFG_RECORD_CFG_OCC_LDS] = h->occ_path == MFG_RECORD_OCC_LDS ? 4 * d.HW : 0;
  out[MFG_RECORD_CFG_O_CELL] = d.o_cell;
  out[MFG_RECORD_CFG_O_ACT] = d.o_act;
  out[MFG_RECORD_CFG_O_BAT] = d.o_bat;
  out[MFG_RECORD_CFG_O_DOOR] = d.o_rdoor;
  out[MFG_RECORD_CFG_O_ITEMS] = d.o_ritems;
  out[MFG_RECORD_CFG_ITEM_CAP] = d.imax;
  return 0;
}

extern "C" int mfg_record_step(mfg_record* h, const int32_t* actions, const uint8_t* ev_act, const uint8_t* ev_watch,
                               const int32_t* ev_misc, const uint8_t* done, void* stream) {
  if (!h) return rfail("null record handle");
  if (h->d.n_sel > 0 && (!actions || !ev_act || !ev_watch || !ev_misc || !done))
    return rfail("mfg_record_step: actions, ev_act, ev_watch, ev_misc and done are required when envs are selected");
  DevScope g(h->device);
  hipStream_t st = (hipStream_t)stream;
  if (h->row_grid) {
    hipLaunchKernelGGL(k_record_rows, dim3(h->row_grid), dim3(MFG_REC_WPB * MFG_WAVE), 0, st, h->d, actions, ev_act,
                       ev_watch, ev_misc, done);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return rfail(std::string("k_record_rows launch: ") + hipGetErrorString(err));
  }
  if (h->occ_grid) {
    if (h->occ_path == MFG_RECORD_OCC_LDS)
      hipLaunchKernelGGL(k_record_occ<true>, dim3(h->occ_grid), dim3(MFG_REC_OCC_THREADS), (size_t)4 * h->d.HW, st, h->d);
    else
      hipLaunchKernelGGL(k_record_occ<false>, dim3(h->occ_grid), dim3(MFG_REC_OCC_THREADS), 0, st, h->d);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return rfail(std::string("k_record_occ launch: ") + hipGetErrorString(err));
  }
  return 0;
}

extern "C" int mfg_record_drain(mfg_record* h, uint32_t* rows_out, uint32_t* counts_out, void* stream) {
  if (!h) return rfail("null record handle");
  DevScope g(h->device);
  hipStream_t st = (hipStream_t)stream;
  const RecDev& d = h->d;
  const size_t n_sel = (size_t)d.n_sel;
  if (n_sel) {
    REC_HIPCHK(hipMemcpyAsync(h->h_counts.data(), d.counters, n_sel * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    REC_HIPCHK(hipStreamSynchronize(st));
    const size_t env_words = (size_t)d.cap * (size_t)d.row_words;
    for (size_t s = 0; s < n_sel; s++) {
      if (counts_out) counts_out[s] = h->h_counts[s];
      const size_t n = (size_t)std::min<long long>((long long)h->h_counts[s], d.cap);
      if (n && rows_out)
        REC_HIPCHK(hipMemcpyAsync(rows_out + s * env_words, d.rows + s * env_words,
                                  n * (size_t)d.row_words * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    }
    REC_HIPCHK(hipMemsetAsync(d.counters, 0, n_sel * sizeof(uint32_t), st));
  }
  REC_HIPCHK(hipStreamSynchronize(st));
  return 0;
}

extern "C" int mfg_record_occupancy(mfg_record* h, uint64_t* out, void* stream) {
  if (!h || !out) return rfail("null argument");
  if (h->occ_path == MFG_RECORD_OCC_OFF) return rfail("mfg_record_occupancy: the recorder was created with occupancy off");
  DevScope g(h->device);
  hipStream_t st = (hipStream_t)stream;
  REC_HIPCHK(hipMemcpyAsync(out, h->d.occ, (size_t)h->d.HW * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  REC_HIPCHK(hipStreamSynchronize(st));
  return 0;
}

extern "C" int mfg_record_clear_occupancy(mfg_record* h, void* stream) {
  if (!h) return rfail("null record handle");
  if (h->occ_path == MFG_RECORD_OCC_OFF) return rfail("mfg_record_clear_occupancy: the recorder was created with occupancy off");
  DevScope g(h->device);
  REC_HIPCHK(hipMemsetAsync(h->d.occ, 0, (size_t)h->d.HW * sizeof(uint64_t), (hipStream_t)stream));
  return 0;
}

extern "C" int mfg_record_env_state(mfg_record* h, int64_t env, void* out, void* stream) {
  if (!h || !out) return rfail("null argument");
  if (env < 0 || env >= h->d.B) return rfail("mfg_record_env_state: env id out of range");
  DevScope g(h->device);
  hipStream_t st = (hipStream_t)stream;
  REC_HIPCHK(hipMemcpyAsync(out, h->d.state + (size_t)env * (size_t)h->d.rec_size, (size_t)h->d.rec_size,
                            hipMemcpyDeviceToHost, st));
  REC_HIPCHK(hipStreamSynchronize(st));
  return 0;
}
