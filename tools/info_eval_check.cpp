// info_eval_check.cpp — stand-alone host check of the info monitor's shared code (csrc/mfg_info_eval.h): the per-key
// evaluation function the kernel runs and the program validator, on a hand-written program with a few ops of every
// kind, 70 agents (the second 64-lane agent word) and door bits in all four door words. Meant for a sanitizer build,
// on the host only (no GPU code, no GPU call):
//
//   hipcc -x hip --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -o info_eval_check tools/info_eval_check.cpp && ./info_eval_check
//
// (or any host C++17 compiler with -fsanitize=address,undefined). Exit status 0 and "info_eval_check ok" = clean.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../marl-factory-grid_amd/csrc/mfg_info_eval.h"

static int g_bad = 0;
#define EXPECT(c)                                                        \
  do {                                                                   \
    if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); g_bad++; } \
  } while (0)

int main() {
  const int A = 70;
  enum { K_ACT0, K_ACT69, K_COLL69, K_AUTOCLOSE, K_BAT_FIXED, K_BAT_TABLE, K_DIRT, K_REACH, K_ITEMS, K_WATCH,
         K_DOOR0, K_DOOR40, K_DOOR70, K_DOOR127, K_MAINT33, K_DONE31, K_MDONE, K_EMPTY, N_KEYS };
  std::vector<mfg_info_op> ops;
  std::vector<int32_t> key_off(1, 0);
  auto op = [&](int key, int kind, int agent, int i0, double r) { ops.push_back(mfg_info_op{key, kind, agent, i0, 0, r}); };
  auto end_key = [&]() { key_off.push_back((int32_t)ops.size()); };
  op(K_ACT0, MFG_INFO_ACTION, 0, 0x6, 0.0); end_key();                 // slots 1, 2
  op(K_ACT69, MFG_INFO_ACTION, 69, (int32_t)0x80000001u, 0.0); end_key();  // slots 0, 31
  op(K_COLL69, MFG_INFO_ACT_COLL, 69, 0, 0.0);
  op(K_COLL69, MFG_INFO_WATCH_BIT, 69, 1, -0.25); end_key();           // two ops on one key, in order
  op(K_AUTOCLOSE, MFG_INFO_DOOR_AUTOCLOSE, 0, 0, 0.0); end_key();
  op(K_BAT_FIXED, MFG_INFO_BATTERY_COST, 64, 0, 0.125); end_key();
  op(K_BAT_TABLE, MFG_INFO_BATTERY_COST, 69, 1, 0.0);
  op(K_BAT_TABLE, MFG_INFO_WATCH_BIT, 69, 2, -1.0); end_key();
  op(K_DIRT, MFG_INFO_DIRT_SPAWN, 0, 0, 0.0); end_key();
  op(K_REACH, MFG_INFO_DEST_REACH, 65, 0, 0.1); end_key();
  op(K_ITEMS, MFG_INFO_RESPAWN_ITEMS, 0, 0, 0.0); end_key();
  op(K_WATCH, MFG_INFO_WATCH_BIT, 1, 2, -0.5); end_key();
  op(K_DOOR0, MFG_INFO_DOOR_COLL, 0, 0, -0.01); end_key();
  op(K_DOOR40, MFG_INFO_DOOR_COLL, 0, 40, -0.02); end_key();
  op(K_DOOR70, MFG_INFO_DOOR_COLL, 0, 70, -0.03); end_key();
  op(K_DOOR127, MFG_INFO_DOOR_COLL, 0, 127, -0.04); end_key();
  op(K_MAINT33, MFG_INFO_MAINT_COLL, 0, 33, -0.05); end_key();
  op(K_DONE31, MFG_INFO_DONE_BIT, 0, 31, -2.0); end_key();
  op(K_MDONE, MFG_INFO_MAINT_DONE, 68, 3, -3.0); end_key();
  end_key();  // K_EMPTY: a key without ops is never present
  EXPECT((int)key_off.size() == N_KEYS + 1);

  std::vector<double> atab((size_t)A * MFG_MAX_ACTIONS * MFG_INFO_ATAB_N, 0.0);
  auto tab = [&](int a, int s, int c) -> double& { return atab[((size_t)a * MFG_MAX_ACTIONS + s) * MFG_INFO_ATAB_N + c]; };
  tab(0, 2, 0) = 0.5; tab(0, 2, 1) = -0.5; tab(0, 2, 2) = 7.0; tab(0, 2, 3) = -7.0;
  tab(69, 31, 0) = 1.5; tab(69, 31, 1) = -1.5; tab(69, 31, 4) = 0.0625;
  std::vector<int32_t> n_actions(A, 3);
  n_actions[69] = 32;
  const double noop_cost = 0.03125;
  const int dest_max = 3, n_ops = (int)ops.size();

  EXPECT(mfg_info_check_program(ops.data(), n_ops, key_off.data(), N_KEYS, atab.data(), A, n_actions.data(), dest_max).empty());
  // the validator names what is wrong
  auto check = [&](const std::vector<mfg_info_op>& o, const std::vector<int32_t>& off, int nk, int na) {
    return mfg_info_check_program(o.data(), (int)o.size(), off.data(), nk, atab.data(), na, n_actions.data(), dest_max);
  };
  { auto o = ops; o[2].key = N_KEYS; EXPECT(check(o, key_off, N_KEYS, A).find("op key out of range") != std::string::npos); }
  { auto o = ops; o[2].key = -1; EXPECT(check(o, key_off, N_KEYS, A).find("op key out of range") != std::string::npos); }
  { auto o = ops; o[1].agent = A; EXPECT(check(o, key_off, N_KEYS, A).find("op agent index") != std::string::npos); }
  { auto o = ops; o[0].kind = MFG_INFO_KIND_N; EXPECT(check(o, key_off, N_KEYS, A).find("op kind") != std::string::npos); }
  { auto o = ops; o[12].i0 = MFG_MAX_DOORS; EXPECT(check(o, key_off, N_KEYS, A).find("op i0") != std::string::npos); }
  { auto f = key_off; f[3] = f[2] - 1; EXPECT(check(ops, f, N_KEYS, A).find("not monotone") != std::string::npos); }
  { auto f = key_off; f[N_KEYS] = n_ops + 1; EXPECT(check(ops, f, N_KEYS, A).find("key_off") != std::string::npos); }
  EXPECT(check(ops, key_off, MFG_INFO_MAX_KEYS + 1, A).find("n_keys out of range") != std::string::npos);
  EXPECT(check(ops, key_off, N_KEYS, MFG_MAX_AGENTS + 1).find("n_agents out of range") != std::string::npos);

  // one step: exact-size rows, so an index past A or past MFG_EV_MISC_N is a heap overflow the sanitizer reports
  std::vector<int32_t> actions(A, 0), misc(MFG_EV_MISC_N, 0);
  std::vector<uint8_t> eact(A, 0), ewatch(A, 0), slot(A, 0);
  std::vector<double> reward(A, 0.0);
  actions[0] = 2; eact[0] = 0x80 | 1 | 4;            // acted, valid, drop-off branch: aux0
  actions[69] = 99; eact[69] = 0x80 | 2;             // clamped to slot 31, failed, action collision
  ewatch[69] = 1 | 2;
  ewatch[65] = 5 << 3;                               // 5 destinations credited, dest_max 3
  ewatch[1] = 2;
  ewatch[68] = 4;
  misc[MFG_EVM_FLAGS] = 1;
  misc[MFG_EVM_DIRT_SPAWN] = 4; misc[MFG_EVM_RESPAWN_ITEMS] = -1;
  misc[MFG_EVM_DOOR_COLL_LO] = 1; misc[MFG_EVM_DOOR_COLL_HI] = 1 << 8; misc[MFG_EVM_DOOR_COLL_2] = 1 << 6;
  misc[MFG_EVM_DOOR_COLL_3] = INT32_MIN;
  misc[MFG_EVM_MAINT_COLL_HI] = 2;
  misc[MFG_EVM_DONE_MASK] = INT32_MIN | (1 << 3);
  misc[MFG_EVM_STEP] = 17;
  for (int a = 0; a < A; a++) reward[a] = 0.1 * (a + 1);
  mfg_info_clamp_slots(actions.data(), n_actions.data(), A, slot.data());
  EXPECT(slot[69] == 31 && slot[0] == 2);

  const MfgInfoProg P{ops.data(), key_off.data(), atab.data(), N_KEYS, A, noop_cost, dest_max};
  double v[N_KEYS + 2];
  bool p[N_KEYS + 2];
  for (int k = 0; k < N_KEYS + 2; k++)
    p[k] = mfg_info_eval_key(P, k, slot.data(), eact.data(), ewatch.data(), misc.data(), reward.data(), &v[k]);
  EXPECT(p[K_ACT0] && v[K_ACT0] == 7.0);
  EXPECT(p[K_ACT69] && v[K_ACT69] == -1.5);
  EXPECT(p[K_COLL69] && v[K_COLL69] == 0.0 + 1.0 + -0.25);
  EXPECT(p[K_AUTOCLOSE] && v[K_AUTOCLOSE] == 1.0);
  EXPECT(p[K_BAT_FIXED] && v[K_BAT_FIXED] == 0.125);
  EXPECT(p[K_BAT_TABLE] && v[K_BAT_TABLE] == 0.0625 + -1.0);
  EXPECT(p[K_DIRT] && v[K_DIRT] == 4.0);
  EXPECT(p[K_REACH] && v[K_REACH] == 0.0 + 0.1 + 0.1 + 0.1);
  EXPECT(!p[K_ITEMS] && v[K_ITEMS] == 0.0);
  EXPECT(p[K_WATCH] && v[K_WATCH] == -0.5);
  EXPECT(p[K_DOOR0] && p[K_DOOR40] && p[K_DOOR70] && p[K_DOOR127] && v[K_DOOR127] == -0.04 && v[K_DOOR70] == -0.03);
  EXPECT(p[K_MAINT33] && v[K_MAINT33] == -0.05);
  EXPECT(p[K_DONE31] && v[K_DONE31] == -2.0);
  EXPECT(p[K_MDONE] && v[K_MDONE] == -3.0);
  EXPECT(!p[K_EMPTY] && v[K_EMPTY] == 0.0);
  double s = 0.0;
  for (int a = 0; a < A; a++) s = s + reward[a];
  EXPECT(p[N_KEYS] && v[N_KEYS] == s);
  EXPECT(p[N_KEYS + 1] && v[N_KEYS + 1] == 17.0);

  // nothing fires: an agent that did not act pays the Noop cost; every event key is absent
  std::fill(eact.begin(), eact.end(), 0);
  std::fill(ewatch.begin(), ewatch.end(), 0);
  std::fill(misc.begin(), misc.end(), 0);
  misc[MFG_EVM_DIRT_SPAWN] = -1; misc[MFG_EVM_RESPAWN_ITEMS] = -1;
  int present = 0;
  for (int k = 0; k < N_KEYS; k++)
    present += mfg_info_eval_key(P, k, slot.data(), eact.data(), ewatch.data(), misc.data(), reward.data(), &v[k]);
  EXPECT(present == 2 && v[K_BAT_TABLE] == noop_cost && v[K_BAT_FIXED] == 0.125);

  if (g_bad) return 1;
  printf("info_eval_check ok\n");
  return 0;
}
