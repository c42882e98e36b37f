/* mfg_record.h — the batched state recorder: per-step state rows of chosen envs and the agents' cell-visit counts
 * of the whole batch, folded on the device; the batched form of utils/logging/recorder.py (EnvRecorder).
 *
 * Not part of the Factory.step boundary (include/mfg.h): it reads the env records (through mfg_layout,
 * mfg_state_ptr and mfg_state_bytes) and the buffers an mfg_step call wrote, and writes no engine state.
 *
 * One mfg_record_step call follows one K = 1 mfg_step made WITHOUT MFG_STEP_AUTO_RESET, so that the records still
 * hold the state that step left (an auto-reset would have overwritten the state of a done step); the caller resets
 * the done envs afterwards (mfg_reset with the done flags as the mask).
 *
 * Row of one (selected env, step): `row_words` u32 words (mfg_record_config), A = agents, D = doors, I = the item
 * slots of the env record (the SpawnItems quantity):
 *
 *   word 0                 env id
 *   word 1                 episode number, 1-based: the resets the env has done so far (the record's `episode`
 *                          header slot, which counts from 0, plus 1), as EnvRecorder._curr_episode counts
 *   word 2                 Gamestate.curr_step after the step (the record's `step` header slot)
 *   word 3                 flags: bit0 done, bit1 crashed (MFG_EVM_FLAGS bit1)
 *   o_cell + a   (a < A)   agent a's cell, row-major x * W + y (the record's agent position word)
 *   o_act + a    (a < A)   bits 0..7 the action index given for agent a, bits 8..15 its ev_act byte,
 *                          bits 16..23 its ev_watch byte
 *   o_bat + 2a, + 2a + 1   (specs with batteries; o_bat = -1 without) the low and the high word of agent a's battery
 *                          charge level, the record's f64 bit for bit
 *   o_door + d   (d < D)   door d's record word: bit0 open, bits 8..15 time_to_close, bit16 present
 *   o_items                n_items: the item slots in use
 *   o_items + 1            item_base: slot k is 'Item[item_base + k]'
 *   o_items + 2 + k (k < I) item slot k's record word: bits 0..15 the cell (0xFFFF: no position, carried by an
 *                          agent), bit16 alive (a member of the collection; dead slots are skipped)
 *
 * with o_cell = 4, o_act = 4 + A, o_bat = 4 + 2A, o_door = 4 + 2A (+ 2A with batteries), o_items = o_door + D and
 * row_words = o_items + 2 + I. That is exactly what Factory.summarize_state (environment/factory.py:281-292) keeps:
 * step, walls (static), doors, agents, items and batteries.
 *
 * Plain C, device pointers unless stated, launched on `stream` (a hipStream_t); every function returns 0, or a
 * negative value with a message in the last-error string of include/mfg.h (queried with a NULL engine). */
#ifndef MFG_RECORD_H
#define MFG_RECORD_H
#include <stdint.h>

#include "mfg.h"
#ifdef __cplusplus
extern "C" {
#endif

#define MFG_RECORD_MAX_EPISODES 4096      /* n_ep bound */
#define MFG_RECORD_MAX_CAPACITY (1 << 20) /* capacity bound */
#define MFG_RECORD_CFG_N 16               /* ints written by mfg_record_config */

/* mfg_record_config slots */
enum {
  MFG_RECORD_CFG_ROW_WORDS = 0,
  MFG_RECORD_CFG_N_SEL = 1,
  MFG_RECORD_CFG_CAPACITY = 2,
  MFG_RECORD_CFG_ROW_WAVES = 3,    /* row kernel: waves (selected envs) per workgroup */
  MFG_RECORD_CFG_ROW_GRID = 4,     /* ... and its workgroups (0: no env selected, no launch) */
  MFG_RECORD_CFG_OCC_THREADS = 5,  /* occupancy kernel: threads per workgroup */
  MFG_RECORD_CFG_OCC_ENVS = 6,     /* ... envs per workgroup */
  MFG_RECORD_CFG_OCC_GRID = 7,     /* ... workgroups (0: occupancy off) */
  MFG_RECORD_CFG_OCC_PATH = 8,     /* MFG_RECORD_OCC_* */
  MFG_RECORD_CFG_OCC_LDS = 9,      /* bytes of the LDS histogram (0 unless the LDS path) */
  MFG_RECORD_CFG_O_CELL = 10,
  MFG_RECORD_CFG_O_ACT = 11,
  MFG_RECORD_CFG_O_BAT = 12,       /* -1: the spec has no batteries */
  MFG_RECORD_CFG_O_DOOR = 13,
  MFG_RECORD_CFG_O_ITEMS = 14,
  MFG_RECORD_CFG_ITEM_CAP = 15
};
enum { MFG_RECORD_OCC_OFF = 0, MFG_RECORD_OCC_LDS = 1, MFG_RECORD_OCC_GLOBAL = 2 };

typedef struct mfg_record mfg_record;

/* A recorder over engine `e`, which was created from `spec` (HOST memory, read during this call only; its agent,
 * door and item counts are checked against the engine's record layout).
 *   envs       HOST i32 [n_sel]: the env ids to record, any order, no duplicates, 0 <= id < B; 0 <= n_sel <= B
 *   capacity   rows per selected env between two drains, 1 .. MFG_RECORD_MAX_CAPACITY
 *   episodes   HOST i32 [n_ep] or NULL (n_ep = 0): record only these episode numbers (>= 1, as word 1 counts);
 *              NULL: every episode; n_ep <= MFG_RECORD_MAX_EPISODES
 *   occupancy  1: count every agent's cell of EVERY env of the batch at each step into occ u64 [H * W]; 0: off
 *   occ_lds_cells  test-only. 0: the builder's choice (the workgroup histogram in LDS for levels of at most 8192
 *              cells, else adds straight to global memory); > 0: the LDS histogram only for levels of at most that
 *              many cells (and never above the builder's own bound)
 * Allocates, zeroed: rows u32 [n_sel][capacity][row_words], counters u32 [n_sel], occ u64 [H * W]. n_sel = 0 with
 * occupancy = 0 is refused (nothing to record). */
int mfg_record_create(mfg_engine* e, const mfg_spec* spec, const int32_t* envs, int64_t n_sel, int64_t capacity,
                      const int32_t* episodes, int n_ep, int occupancy, int occ_lds_cells, mfg_record** out);
int mfg_record_destroy(mfg_record* h);

/* out[MFG_RECORD_CFG_N]: the row shape and the launch shapes the builder chose (slots above). */
int mfg_record_config(const mfg_record* h, int32_t* out);

/* Record the step a K = 1 mfg_step (no MFG_STEP_AUTO_RESET) just made, from that call's buffers: actions i32 [B][A]
 * (the action indices given to mfg_step), ev_act / ev_watch u8 [B][A], ev_misc i32 [B][MFG_EV_MISC_N], done u8 [B].
 * Each selected env whose episode number passes the filter takes the next row index of its counter and writes its
 * row if the index is below capacity; the counter keeps counting past capacity (the excess is dropped, nothing is
 * written out of bounds). With occupancy, every agent of every env adds 1 to occ[its cell]. The five buffers may be
 * NULL when no env is selected. */
int mfg_record_step(mfg_record* h, const int32_t* actions, const uint8_t* ev_act, const uint8_t* ev_watch,
                    const int32_t* ev_misc, const uint8_t* done, void* stream);

/* Copy the counters to HOST counts_out u32 [n_sel] and, of selected env s (the order of `envs`), its first
 * min(count, capacity) rows to HOST rows_out u32 [n_sel][capacity][row_words] (either may be NULL), then reset the
 * counters to 0. Waits for `stream`. */
int mfg_record_drain(mfg_record* h, uint32_t* rows_out, uint32_t* counts_out, void* stream);

/* Copy the occupancy map to HOST out u64 [H * W] (row-major cells); it is not cleared. Waits for `stream`. */
int mfg_record_occupancy(mfg_record* h, uint64_t* out, void* stream);
int mfg_record_clear_occupancy(mfg_record* h, void* stream);

/* Copy env `env`'s whole state record (mfg_layout[0] bytes) to HOST out: the record a header summary is read from
 * without exporting the batch. Waits for `stream`. */
int mfg_record_env_state(mfg_record* h, int64_t env, void* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
