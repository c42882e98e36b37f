// mfg_info_eval.h — the info program's per-key evaluation, ONE function for the kernel (k_info_step, mfg_info.hip),
// the host entry point (mfg_info_eval_host) and the stand-alone host check (tools/info_eval_check.cpp), and the
// program validator every entry point runs before a program is used. Plain C++: no HIP header is needed on the host.
#pragma once
#include <stdint.h>
#include <string>

#include "../../include/mfg.h"
#include "../../include/mfg_info.h"

#if defined(__HIPCC__)
#define MFG_HD __host__ __device__
#else
#define MFG_HD
#endif

// A validated program (host or device pointers, as the caller's side needs).
struct MfgInfoProg {
  const mfg_info_op* ops;
  const int32_t* key_off;  // [n_keys + 1]
  const double* atab;      // [A][MFG_MAX_ACTIONS][MFG_INFO_ATAB_N]
  int n_keys, n_agents;
  double noop_cost;
  int dest_max;
};

// Value and presence of column `key` (< n_keys + 2) for one env-step. slot: the agents' action indices clamped to
// their action counts (u8 [A]); eact / ewatch: the ev_act / ev_watch rows; misc: the ev_misc row; reward: f64 [A].
// Additions only, in op order from 0.0 (InfoColumns.__call__): the host and the device give the same bits.
MFG_HD inline bool mfg_info_eval_key(const MfgInfoProg& P, int key, const uint8_t* slot, const uint8_t* eact,
                                     const uint8_t* ewatch, const int32_t* misc, const double* reward, double* out) {
  double v = 0.0;
  if (key >= P.n_keys) {
    if (key == P.n_keys) {
      for (int a = 0; a < P.n_agents; a++) v = v + reward[a];  // sum(reward): left to right from 0
    } else {
      v = (double)misc[MFG_EVM_STEP];
    }
    *out = v;
    return true;
  }
  bool p = false;
  const int o1 = P.key_off[key + 1];
  for (int o = P.key_off[key]; o < o1; o++) {
    const mfg_info_op& op = P.ops[o];
    const int a = op.agent, i0 = op.i0;
    bool m = false;
    double x = op.r;
    switch (op.kind) {
      case MFG_INFO_ACTION: {
        const int s = slot[a], b = eact[a];
        m = (b & 0x80) && ((((uint32_t)i0) >> s) & 1u);
        // columns 0 valid, 1 fail, 2 aux0, 3 aux1: the drop-off branch (bit2) takes the aux pair
        x = P.atab[((size_t)a * MFG_MAX_ACTIONS + s) * MFG_INFO_ATAB_N + ((b & 4) ? 2 : 0) + ((b & 1) ? 0 : 1)];
        break;
      }
      case MFG_INFO_ACT_COLL:
        m = (eact[a] & 0x82) == 0x82;
        x = 1.0;
        break;
      case MFG_INFO_DOOR_AUTOCLOSE:
        m = (misc[MFG_EVM_FLAGS] & 1) != 0;
        x = 1.0;
        break;
      case MFG_INFO_BATTERY_COST:
        m = true;
        if (i0)
          x = (eact[a] & 0x80) ? P.atab[((size_t)a * MFG_MAX_ACTIONS + slot[a]) * MFG_INFO_ATAB_N + 4] : P.noop_cost;
        break;
      case MFG_INFO_DIRT_SPAWN:
        m = misc[MFG_EVM_DIRT_SPAWN] >= 0;
        x = (double)misc[MFG_EVM_DIRT_SPAWN];
        break;
      case MFG_INFO_DEST_REACH: {
        int n = (ewatch[a] >> 3) & 31;
        if (n > P.dest_max) n = P.dest_max;
        for (int c = 1; c < n; c++) v = v + x;  // one addition per credited destination (the last one below)
        m = n > 0;
        break;
      }
      case MFG_INFO_RESPAWN_ITEMS:
        m = misc[MFG_EVM_RESPAWN_ITEMS] >= 0;
        x = (double)misc[MFG_EVM_RESPAWN_ITEMS];
        break;
      case MFG_INFO_WATCH_BIT:
        m = (ewatch[a] & i0) != 0;
        break;
      case MFG_INFO_DOOR_COLL: {
        const int col = i0 < 32 ? MFG_EVM_DOOR_COLL_LO
                                : i0 < 64 ? MFG_EVM_DOOR_COLL_HI : i0 < 96 ? MFG_EVM_DOOR_COLL_2 : MFG_EVM_DOOR_COLL_3;
        m = ((((uint32_t)misc[col]) >> (i0 & 31)) & 1u) != 0;
        break;
      }
      case MFG_INFO_MAINT_COLL:
        m = ((((uint32_t)misc[i0 < 32 ? MFG_EVM_MAINT_COLL : MFG_EVM_MAINT_COLL_HI]) >> (i0 & 31)) & 1u) != 0;
        break;
      case MFG_INFO_DONE_BIT:
        m = ((((uint32_t)misc[MFG_EVM_DONE_MASK]) >> i0) & 1u) != 0;
        break;
      case MFG_INFO_MAINT_DONE:
        m = ((((uint32_t)misc[MFG_EVM_DONE_MASK]) >> i0) & 1u) != 0 && (ewatch[a] & 4) != 0;
        break;
      default:
        break;
    }
    if (m) {
      v = v + x;
      p = true;
    }
  }
  *out = v;
  return p;
}

// Host: every count and index of a program. Returns an empty string, or what is wrong.
inline std::string mfg_info_check_program(const mfg_info_op* ops, int n_ops, const int32_t* key_off, int n_keys,
                                          const double* action_table, int n_agents, const int32_t* n_actions,
                                          int dest_max) {
  auto num = [](long long x) { return std::to_string(x); };
  if (n_agents < 1 || n_agents > MFG_MAX_AGENTS) return "n_agents out of range: " + num(n_agents);
  if (n_keys < 0 || n_keys > MFG_INFO_MAX_KEYS)
    return "n_keys out of range: " + num(n_keys) + " (at most " + num(MFG_INFO_MAX_KEYS) + ")";
  if (n_ops < 0 || n_ops > MFG_INFO_MAX_OPS)
    return "n_ops out of range: " + num(n_ops) + " (at most " + num(MFG_INFO_MAX_OPS) + ")";
  if (dest_max < 0 || dest_max > 31) return "dest_max out of range: " + num(dest_max);
  if (!key_off || !action_table || !n_actions || (n_ops && !ops)) return "null program pointer";
  for (int a = 0; a < n_agents; a++)
    if (n_actions[a] < 1 || n_actions[a] > MFG_MAX_ACTIONS)
      return "n_actions out of range for agent " + num(a) + ": " + num(n_actions[a]);
  if (key_off[0] != 0) return "key_off[0] must be 0";
  for (int k = 0; k < n_keys; k++)
    if (key_off[k + 1] < key_off[k] || key_off[k + 1] > n_ops)
      return "key_off is not monotone within n_ops at key " + num(k);
  if (key_off[n_keys] != n_ops) return "key_off[n_keys] must equal n_ops";
  for (int k = 0; k < n_keys; k++) {
    for (int o = key_off[k]; o < key_off[k + 1]; o++) {
      const mfg_info_op& op = ops[o];
      const std::string at = " (op " + num(o) + ")";
      if (op.key < 0 || op.key >= n_keys) return "op key out of range: " + num(op.key) + at;
      if (op.key != k) return "op key " + num(op.key) + " sits in the op list of key " + num(k) + at;
      if (op.kind < 0 || op.kind >= MFG_INFO_KIND_N) return "op kind out of range: " + num(op.kind) + at;
      if (op.agent < 0 || op.agent >= n_agents) return "op agent index out of range: " + num(op.agent) + at;
      int lo = 0, hi = 0;  // i0 in [lo, hi]
      switch (op.kind) {
        case MFG_INFO_ACTION: lo = INT32_MIN; hi = INT32_MAX; break;  // u32 bitmask
        case MFG_INFO_BATTERY_COST: hi = 1; break;
        case MFG_INFO_WATCH_BIT: lo = 1; hi = 255; break;
        case MFG_INFO_DOOR_COLL: hi = MFG_MAX_DOORS - 1; break;
        case MFG_INFO_MAINT_COLL: hi = 63; break;
        case MFG_INFO_DONE_BIT: case MFG_INFO_MAINT_DONE: hi = 31; break;
        default: break;
      }
      if (op.i0 < lo || op.i0 > hi) return "op i0 out of range: " + num(op.i0) + at;
    }
  }
  return std::string();
}

// Host: the agents' action indices clamped to [0, n_actions[a]) as the u8 slots the evaluation reads.
inline void mfg_info_clamp_slots(const int32_t* actions, const int32_t* n_actions, int n_agents, uint8_t* slot) {
  for (int a = 0; a < n_agents; a++) {
    int s = actions[a];
    if (s < 0) s = 0;
    if (s > n_actions[a] - 1) s = n_actions[a] - 1;
    slot[a] = (uint8_t)s;
  }
}
