/* sfmi_policy.h -- the policy head: actions, log-probabilities and entropies from a batch of logits, in one launch.
 *
 * sfmi.h declares the ABI whose list of entry points is fixed per object; the call below is declared here and exported by the
 * same library, libsfmi.so.  It stands where the reference's trainer has softmax, log_softmax, multinomial(1) or max(1)[1], and
 * gather (rl/networks.py:65-76) between the network and the env: sf_step_sampled draws uniform actions inside the step launch,
 * this call draws them from the policy's own distribution, on the same kind of stream -- Philox4x32-10 with a per-tile tick kept
 * on the device, so that a captured graph draws new actions at every replay.
 *
 * sf_policy_sample: logits_dev is float32 [n_envs] rows of n_actions values, row i at logits_dev + i * row_stride (in floats).
 *
 *   Per row, x[0 .. A-1]:
 *     1. m = max_k x[k].
 *     2. e[k] = expf(x[k] - m), in float32.  x[k] = -inf gives exactly 0: a masked action.
 *     3. c[k] = c[k-1] + (double)e[k]: a float64 running sum in index order; S = c[A-1].
 *
 *   mode 0, sample: w is word 0 of Philox4x32-10 with key = seed (low word, high word) and counter
 *     (first_lane + i, tick, 0x504F4C, 0).  The third counter word keeps this stream apart from sf_step_sampled's, whose counter
 *     is (lane, tick, 0, 0).  t = (((double)w + 0.5) * 2^-32) * S, and the action is the smallest k with t < c[k].  It always
 *     exists (t < S), and it is never an action with e[k] == 0 (there c[k] == c[k-1]).
 *     tick is ticks_dev[i / 64]: every lane of the wave reads it, and after the wave's reads its first lane stores tick + 1.
 *     A replayed graph therefore draws anew, and no wave depends on another.  ticks_dev is uint32 [ceil(n_envs / 64)],
 *     caller-owned; zero it to start a stream.  A shard that holds envs [k, k + n) of a larger batch passes first_lane = k and
 *     draws what the whole batch draws for those envs (k need not be a multiple of 64: the tick is per call, the lane is global).
 *   mode 1, argmax (deterministic=True, rl/networks.py:71-72): the action is the first index of the maximum.  ticks_dev is
 *     neither read nor written and may be NULL.
 *
 *   Outputs, with a the action: actions_out_dev[i] = a as uint8, int32 or int64 (act_type 1 / 4 / 8, as sf_step reads them);
 *     logp_out_dev[i]    = (x[a] - m) - logf((float)S)
 *     entropy_out_dev[i] = logf((float)S) - (sum_k e[k] * (x[k] - m)) / (float)S
 *   float32, the sum in index order with the terms of e[k] == 0 skipped: what -(log_probs * probs).sum(-1) gives per row.
 *   Either of the two may be NULL.  The translation unit is compiled without contraction (no fused multiply-add).
 *
 *   Bad rows: a row that holds a NaN, a +inf, or nothing but -inf.  It plays action 0 -- never an action outside the set --,
 *   writes NaN to logp and entropy, adds 1 to *bad_rows_dev (uint64, may be NULL) and, in mode 0, consumes its tick like any
 *   other row.
 *
 *   Plain stream work: no allocation, no synchronise, no batch handle; it can be captured in a HIP graph.
 *
 *   SF_ERR_ARG (with a text, nothing launched): NULL logits or actions; n_envs <= 0; n_actions outside [1, 32];
 *   row_stride < n_actions; a mode other than 0 or 1; an act_type other than 1, 4 or 8; mode 0 with NULL ticks_dev; logits not
 *   4-byte aligned. */
#ifndef SFMI_POLICY_H
#define SFMI_POLICY_H

#include "sfmi.h"

#define SF_POLICY_SAMPLE 0
#define SF_POLICY_ARGMAX 1
#define SF_POLICY_MAX_ACTIONS 32
#define SF_POLICY_COUNTER_WORD 0x504F4Cu

#ifdef __cplusplus
extern "C" {
#endif

int sf_policy_sample(const float* logits_dev, int n_envs, int n_actions, size_t row_stride, int mode, uint64_t seed,
                     uint32_t first_lane, uint32_t* ticks_dev, void* actions_out_dev, int act_type, float* logp_out_dev,
                     float* entropy_out_dev, uint64_t* bad_rows_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SFMI_POLICY_H */
