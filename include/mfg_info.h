/* mfg_info.h — the batched episode monitor: the reference's per-step info dict (environment/factory.py:222-259)
 * evaluated for all B envs on the device and folded per episode, the batched form of utils/logging/envmonitor.py.
 *
 * Not part of the Factory.step boundary (include/mfg.h): it reads the buffers an mfg_step call wrote (the event rows,
 * rewards and done flags) and touches no engine state. The key set and the accumulation order of one config are
 * compiled on the host (mfg_amd/info_program.py) into an "info program":
 *
 *   ops      one record per accumulation, sorted by key (stable: the ops of one key keep the reference's order)
 *   key_off  CSR [n_keys + 1]: key k owns ops[key_off[k] .. key_off[k + 1])
 *   action_table  f64 [n_agents][MFG_MAX_ACTIONS][MFG_INFO_ATAB_N]: valid, fail, aux0, aux1 reward and the battery
 *            cost of every action slot (NaN: the per-action cost dict has no entry for the slot's class)
 *
 * A key's value starts at 0.0 and adds its ops' values in op order, all in f64; a key is present when at least one
 * of its ops fired. Column n_keys is 'step_reward' (the left-to-right f64 sum of the reward row from 0.0), column
 * n_keys + 1 is 'step' (MFG_EVM_STEP); both are always present. Kc = n_keys + 2 columns in all.
 *
 * Plain C, device pointers unless stated, launched on `stream` (a hipStream_t); every function returns 0, or a
 * negative value with a message in the last-error string of include/mfg.h (queried with a NULL engine). */
#ifndef MFG_INFO_H
#define MFG_INFO_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MFG_INFO_MAX_KEYS 4096   /* n_keys bound */
#define MFG_INFO_MAX_OPS 65536   /* n_ops bound */
#define MFG_INFO_ATAB_N 5        /* action table columns: valid, fail, aux0, aux1, battery_cost */
#define MFG_INFO_HDR_N 8         /* ints per finished-episode header row */

/* op kinds; "agent", "i0", "i1", "r" name the fields of the op record below */
enum {
  MFG_INFO_ACTION = 0,         /* agent acted (ev_act bit7) with a slot in the bitmask i0: + the slot's valid / fail
                                  (drop-off branch, ev_act bit2: aux0 / aux1) reward by ev_act bit0 */
  MFG_INFO_ACT_COLL = 1,       /* agent acted and ev_act bit1: + 1.0 */
  MFG_INFO_DOOR_AUTOCLOSE = 2, /* MFG_EVM_FLAGS bit0: + 1.0 */
  MFG_INFO_BATTERY_COST = 3,   /* every step: i0 == 0: + r; i0 == 1: + the acted slot's battery cost, else noop_cost */
  MFG_INFO_DIRT_SPAWN = 4,     /* MFG_EVM_DIRT_SPAWN >= 0: + it */
  MFG_INFO_DEST_REACH = 5,     /* + r once per destination credited to agent (ev_watch bits 3..7, at most dest_max) */
  MFG_INFO_RESPAWN_ITEMS = 6,  /* MFG_EVM_RESPAWN_ITEMS >= 0: + it */
  MFG_INFO_WATCH_BIT = 7,      /* ev_watch[agent] & i0: + r */
  MFG_INFO_DOOR_COLL = 8,      /* door i0's WatchCollisions bit: + r */
  MFG_INFO_MAINT_COLL = 9,     /* maintainer slot i0's WatchCollisions bit: + r */
  MFG_INFO_DONE_BIT = 10,      /* MFG_EVM_DONE_MASK bit i0: + r */
  MFG_INFO_MAINT_DONE = 11,    /* MFG_EVM_DONE_MASK bit i0 and ev_watch[agent] bit2: + r */
  MFG_INFO_KIND_N = 12
};

#pragma pack(push, 4)
typedef struct mfg_info_op {
  int32_t key;    /* column, 0 .. n_keys - 1 */
  int32_t kind;   /* MFG_INFO_* */
  int32_t agent;  /* agent index of the kinds that read an agent's row bytes, else 0 */
  int32_t i0;
  int32_t i1;     /* reserved, 0 */
  double r;
} mfg_info_op;    /* 28 bytes, 4-byte aligned */
#pragma pack(pop)

/* header row of a finished episode */
enum { MFG_INFO_HDR_ENV = 0, MFG_INFO_HDR_EP_INDEX = 1, MFG_INFO_HDR_LENGTH = 2, MFG_INFO_HDR_CRASHED = 3,
       MFG_INFO_HDR_MAINT_BASE = 4 };

typedef struct mfg_info mfg_info;

/* Check the program (host memory; every count and every index, see the top of this file), copy it to `device` and
 * allocate, zeroed: the per-env accumulators acc f64 [n_envs][Kc], cnt u32 [n_envs][Kc], len i32 [n_envs],
 * ep_index i32 [n_envs], and a finished-episode buffer of ep_capacity rows (header i32 [MFG_INFO_HDR_N],
 * sum f64 [Kc], count u32 [Kc]) with its claim counter. n_agents 1..MFG_MAX_AGENTS, n_actions[a] 1..MFG_MAX_ACTIONS,
 * n_keys 0..MFG_INFO_MAX_KEYS, n_ops 0..MFG_INFO_MAX_OPS, dest_max 0..31, n_envs >= 1, ep_capacity >= 1. */
int mfg_info_create(const mfg_info_op* ops, int n_ops, const int32_t* key_off, int n_keys,
                    const double* action_table, int n_agents, const int32_t* n_actions, double noop_cost,
                    int dest_max, int device, int64_t n_envs, int64_t ep_capacity, mfg_info** out);
int mfg_info_destroy(mfg_info* h);

/* out[0] = Kc, out[1] = keys per lane held in registers (0: the accumulators live in LDS), out[2] = waves per
 * workgroup, out[3] = LDS bytes per workgroup: the launch shape the builder chose. */
int mfg_info_config(const mfg_info* h, int32_t* out);

/* The K steps of one mfg_step call, in order, from that call's buffers: actions i32 [K][B][A] (NULL: the Philox
 * action index of mfg_step with the same philox_seed / env_base / step_base), ev_act / ev_watch u8 [K][B][A],
 * ev_misc i32 [K][B][MFG_EV_MISC_N], reward f64 [K][B][A], done u8 [K][B]. Per env and step: every column's value
 * and presence, written to vals f64 [K][B][Kc] / pres u8 [K][B][Kc] (either may be NULL), and folded into the env's
 * accumulators (acc += value, cnt += 1 where present; len += 1). A crashed step (MFG_EVM_FLAGS bit1) contributes no
 * value (its vals / pres rows are 0), counts in len and ends the episode with crashed = 1. When done (or crashed)
 * the env claims a row index with one atomic add on the counter, writes its row if the index is below ep_capacity,
 * clears its accumulators and increments its ep_index. The counter keeps counting past ep_capacity. */
int mfg_info_step(mfg_info* h, int K, const int32_t* actions, uint32_t philox_seed, uint32_t env_base,
                  int64_t step_base, const uint8_t* ev_act, const uint8_t* ev_watch, const int32_t* ev_misc,
                  const double* reward, const uint8_t* done, double* vals, uint8_t* pres, void* stream);

/* Episodes finished since the last drain (may exceed ep_capacity: the excess was dropped). Waits for `stream`. */
int mfg_info_episodes(mfg_info* h, uint32_t* out_count, void* stream);

/* The device buffers of the finished rows (fixed for the handle's lifetime): header i32 [cap][MFG_INFO_HDR_N],
 * sum f64 [cap][Kc], count u32 [cap][Kc]. Row order is unspecified; rows 0 .. min(count, cap) - 1 are valid. */
int mfg_info_rows(const mfg_info* h, const int32_t** hdr, const double** sum, const uint32_t** count);

/* Read the counter into *out_count, copy the first min(count, ep_capacity, max_rows) rows into the HOST buffers
 * hdr_out / sum_out / count_out (any may be NULL; max_rows rows each), then reset the counter to 0. Waits for
 * `stream`. Rows beyond max_rows are discarded with the reset. */
int mfg_info_drain(mfg_info* h, int64_t max_rows, int32_t* hdr_out, double* sum_out, uint32_t* count_out,
                   uint32_t* out_count, void* stream);

/* Clear the accumulators (acc, cnt, len) of the envs with mask[b] != 0 (mask u8 [B]; NULL: every env). The
 * per-env ep_index and the finished rows stay. */
int mfg_info_reset(mfg_info* h, const uint8_t* mask, void* stream);

/* One env-step on HOST memory with the kernel's own evaluation function: the program as for the create call,
 * actions i32 [A], ev_act / ev_watch u8 [A], ev_misc i32 [MFG_EV_MISC_N], reward f64 [A] -> vals f64 [Kc],
 * pres u8 [Kc] (zeros for a crashed step). No GPU is touched. */
int mfg_info_eval_host(const mfg_info_op* ops, int n_ops, const int32_t* key_off, int n_keys,
                       const double* action_table, int n_agents, const int32_t* n_actions, double noop_cost,
                       int dest_max, const int32_t* actions, const uint8_t* ev_act, const uint8_t* ev_watch,
                       const int32_t* ev_misc, const double* reward, double* vals, uint8_t* pres);

#ifdef __cplusplus
}
#endif
#endif
