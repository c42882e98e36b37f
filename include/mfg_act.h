/*
 * mfg_act.h — masked acting: mfg_policy_act (include/mfg_learn.h) with an action mask (mfg_action_mask, include/mfg.h).
 * Same library (csrc/mfg_act.hip), same conventions as mfg_learn.h: device pointers, stream-ordered, 0 or -1.
 */
#ifndef MFG_ACT_H_
#define MFG_ACT_H_

#include "mfg_learn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* mfg_policy_act plus `mask`: u32 [n_envs][n_agents] in engine order (device), or NULL for mfg_policy_act itself, which
 * is this function's NULL-mask case (one kernel, the same bits). Before the sample or the argmax a logit whose bit is
 * clear counts as -inf: an action of probability 0, which mfg_policy_act's arithmetic never picks. A row whose word has
 * no bit set among its first n_act[net] is acted unmasked (a crashed env, a paralysed agent). A word with every bit of
 * [0, n_act[net]) set changes nothing. h and logits_out are what mfg_policy_act writes: logits_out holds the
 * network's raw logits, so act_out is mfg_sample_categorical at the same u on logits_out with the masked entries set
 * to -inf. */
int mfg_policy_act_masked(const float* emb, int64_t emb_env, int64_t emb_agent, int64_t n_envs, int n_agents, int g,
                          int e_dim, int ae_dim, int hd, int n_max, const mfg_actor_weights* w, const int32_t* n_act,
                          const int32_t* prev_action, const uint8_t* prev_done, float* h, int64_t h_env, int64_t h_agent,
                          const float* u, int greedy, const uint32_t* mask, int32_t* act_out, float* logits_out,
                          void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MFG_ACT_H_ */
