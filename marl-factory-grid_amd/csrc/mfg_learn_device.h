// Device helpers shared by the learner-side units (mfg_learn.hip, mfg_ppo.hip, mfg_seac.hip, mfg_act.hip). Those units
// build with -ffp-contract=off and rely on separately rounded products and sums: nothing here uses fmaf or
// reassociates, and every expression keeps the operand order its callers' results are pinned to.
#ifndef MFG_LEARN_DEVICE_H
#define MFG_LEARN_DEVICE_H
#include <hip/hip_runtime.h>

namespace {

__device__ __forceinline__ float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }

// sum of v over the block's 256 threads, the same tree every run; the result is valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* sh) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  __syncthreads();  // sh may still be read from a previous call
  if (lane == 0) sh[wv] = v;
  __syncthreads();
  return threadIdx.x == 0 ? ((sh[0] + sh[1]) + (sh[2] + sh[3])) : 0.0;
}

// mx = max_j l[j] and s = sum_j expf(l[j] - mx) over a row of n logits. fmaxf drops a NaN operand, the sum keeps it:
// s is finite and positive exactly when the row is a distribution: no NaN, no +inf, and not -inf throughout (a -inf
// logit beside finite ones adds expf(-inf) = 0, an action of probability 0). The sampling callers test that.
__device__ __forceinline__ void row_max_expsum(const float* __restrict__ l, int n, float& mx, float& s) {
  mx = l[0];
  for (int j = 1; j < n; j++) mx = fmaxf(mx, l[j]);
  s = 0.0f;
  for (int j = 0; j < n; j++) s += expf(l[j] - mx);
}

// The loss heads' view of a row: lse = log sum_j exp(l[j]) as mx + logf(s), and true exactly when every logit is
// finite. A -inf logit that is not the maximum leaves mx and s finite (row_max_expsum), but its entropy term
// expf(-inf) * -inf is NaN and no gradient through it exists, so the heads count such a row as bad as well
// (include/mfg_learn.h: zero gradients for the element, a NaN loss): row_max_expsum's two passes with the smallest
// l[j] - mx kept beside the sum (one more instruction per logit, no further load; mx and s are the same bits).
__device__ __forceinline__ bool row_lse_finite(const float* __restrict__ l, int n, float& lse) {
  float mx = l[0];
  for (int j = 1; j < n; j++) mx = fmaxf(mx, l[j]);
  float s = 0.0f, lo = 0.0f;
  for (int j = 0; j < n; j++) {
    const float d = l[j] - mx;
    s += expf(d);
    lo = fminf(lo, d);
  }
  lse = mx + logf(s);
  return s > 0.0f && !isinf(s) && !isinf(mx) && !isinf(lo);
}

// The action of a row with valid mx / s (row_max_expsum): greedy: the argmax, lowest index on ties; otherwise the
// inversion of the CDF at u * s (u uniform in [0, 1)); rounding past the last bin picks the last action.
__device__ __forceinline__ int row_pick(const float* __restrict__ l, int n, float mx, float s, bool greedy, float u) {
  if (greedy) {
    int pick = 0;
    for (int a = 1; a < n; a++)
      if (l[a] > l[pick]) pick = a;
    return pick;
  }
  const float thr = u * s;
  float c = 0.0f;
  for (int a = 0; a < n; a++) {
    c += expf(l[a] - mx);
    if (thr < c) return a;
  }
  return n - 1;
}

}  // namespace
#endif
