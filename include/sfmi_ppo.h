/* sfmi_ppo.h -- the policy head's update side: the log-probabilities and entropies of GIVEN actions, the PPO loss, and the
 * gradients of both with respect to the logits (and the values), each in one launch.
 *
 * sfmi_policy.h declares the rollout side (sf_policy_sample); the calls below are exported by the same library, libsfmi.so, and
 * stand where the reference's trainer has softmax, log_softmax, gather and -(log_probs*probs).sum(-1).mean() (rl/networks.py:78-86),
 * the clipped surrogate (rl/train.py:123-129: exp, two products, clamp, min, three means, the weighted sum) and autograd's way
 * back through all of it.
 *
 * All calls are plain stream work: no batch handle, no allocation, no synchronise; they can be captured in a HIP graph.  The
 * translation unit is compiled without contraction (no fused multiply-add).
 *
 * THE ROW.  logits_dev is float32 [n_rows] rows of n_actions values, row i at logits_dev + i * row_stride (in floats); a row's
 * arithmetic is sf_policy_sample's, operation by operation (x[0 .. A-1] the row):
 *     m    = max_k x[k]
 *     d[k] = x[k] - m                       float32 (-inf stays -inf)
 *     e[k] = expf(d[k])                     float32; exactly 0 at -inf
 *     S    = sum_k (double)e[k]             a float64 running sum in index order
 *     Sf   = (float)S,  lse = logf(Sf)
 *     dot  = sum_k e[k] * d[k]              float32, index order, the terms of e[k] == 0 skipped
 *     H    = lse - dot / Sf                 the row's entropy
 *   and with a = actions_dev[i] (uint8, int32 or int64: act_type 1 / 4 / 8, as sf_step reads them)
 *     logp = d[a] - lse
 *   so the log-probability a rollout stored through sf_policy_sample and the one recomputed here from the same logits are the
 *   same bits.
 *
 * BAD ROWS.  A row that holds a NaN or a +inf, or nothing but -inf (sf_policy_sample's definition), or whose action lies outside
 * [0, n_actions).  Every output of a bad row is NaN, every gradient entry k < n_actions of its logits row is NaN (and so is its
 * entry of grad_values_out), the forward calls add 1 to *bad_rows_dev (uint64, may be NULL) -- one vector atomic per wave that
 * saw one -- and in sf_ppo_loss it makes all four of sums_out NaN.  An action in range whose logit is -inf is NOT bad: IEEE
 * arithmetic gives logp = -inf (and r = 0 below).
 *
 * sf_policy_evaluate:  logp_out_dev[i] = logp, entropy_out_dev[i] = H; float32 [n_rows]; either may be NULL.
 *
 * sf_policy_evaluate_backward:  grad_logp_dev / grad_entropy_dev are float32 [n_rows], the upstream gradients g_l, g_H of the two
 *   outputs; either may be NULL and then counts as 0.  Row i of grad_logits_out_dev (at + i * grad_row_stride floats) receives,
 *   for k < n_actions only, all in float32 and in this order of operations:
 *     p    = e[k] / Sf
 *     t1   = g_l * ((k == a ? 1 : 0) - p)
 *     t2   = (g_H * p) * ((d[k] - lse) + H)            taken as 0 where e[k] == 0
 *     grad = t1 - t2
 *   and grad = 0 exactly where x[k] == -inf: a masked logit is a constant.
 *
 * sf_ppo_loss:  values_dev, old_logp_dev, adv_dev, returns_dev are float32 [n_rows] (dense).  Per row, in float32, in this order:
 *     r = expf(logp - old_logp)
 *     s = min(r * adv, clampf(r, clip_lo, clip_hi) * adv)          (min and clamp hand a NaN on, as torch's do)
 *     q = (v - ret) * (v - ret)
 *   row_terms_out_dev: float32 [n_rows][3] = (s, q, H), may be NULL.  sums_out_dev: float32 [4] =
 *     action_loss = -mean s,  value_loss = mean q,  entropy = mean H,
 *     loss        = (action_loss + value_coef * value_loss) - entropy_coef * entropy        (float32, on the three rounded means)
 *   A mean is a float64 sum in a fixed order -- a fixed shuffle tree within the wave (lane l takes lane l ^ 32, then ^ 16, ... ^ 1),
 *   the four waves of a block in index order, the blocks in index order -- divided by n_rows and rounded once to float32: two
 *   calls on equal inputs give equal bits, and no float atomic is used.  workspace_dev: sf_ppo_loss_workspace_bytes(n_rows) bytes,
 *   8-byte aligned, caller-owned, holds the blocks' partial sums between the two launches of the call.
 *   clip_lo / clip_hi are floats: the caller passes (float)(1.0 - clip) and (float)(1.0 + clip), rounded from the double, which is
 *   what torch.clamp makes of a Python scalar.
 *
 * sf_ppo_loss_backward:  the same inputs; grad_loss_dev is ONE float on the device, the upstream gradient g of `loss`.  The row is
 *   recomputed, nothing is kept from the forward.  With M = n_rows, per row in float32:
 *     gm   = g / (float)M
 *     c_l  = -((gm * adv) * r)        where  r * adv < clampf(r) * adv  or  clip_lo <= r <= clip_hi  (or either product is NaN);
 *                                     else 0.  (torch's rule: minimum halves the gradient on a tie, clamp passes it on its
 *                                     closed range, and the halves add up to the whole on a tie inside it.  One kind of tie
 *                                     is left: r an ulp outside the range whose product with adv ROUNDS to the bound's; torch
 *                                     hands on half there, this rule none -- at the point where the gradient jumps anyway)
 *     c_H  = -(gm * entropy_coef)
 *     c_v  = (gm * value_coef) * (2 * (v - ret))
 *   grad_values_out_dev[i] = c_v (float32 [n_rows]; may be NULL), and row i of grad_logits_out_dev is sf_policy_evaluate_backward's
 *   with g_l = c_l and g_H = c_H.
 *
 * SF_ERR_ARG (with a text, nothing launched): a NULL logits, actions, values, old_logp, adv, returns, sums_out, grad_loss or
 * grad_logits_out; n_rows <= 0; n_actions outside [1, 32]; row_stride or grad_row_stride below n_actions; an act_type other than
 * 1, 4 or 8; logits, a gradient or any other float array not 4-byte aligned; a NULL workspace or one not 8-byte aligned. */
#ifndef SFMI_PPO_H
#define SFMI_PPO_H

#include "sfmi_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

int sf_policy_evaluate(const float* logits_dev, int n_rows, int n_actions, size_t row_stride, const void* actions_dev, int act_type,
                       float* logp_out_dev, float* entropy_out_dev, uint64_t* bad_rows_dev, void* stream);

int sf_policy_evaluate_backward(const float* logits_dev, int n_rows, int n_actions, size_t row_stride, const void* actions_dev,
                                int act_type, const float* grad_logp_dev, const float* grad_entropy_dev, float* grad_logits_out_dev,
                                size_t grad_row_stride, void* stream);

size_t sf_ppo_loss_workspace_bytes(int n_rows);

int sf_ppo_loss(const float* logits_dev, const float* values_dev, const void* actions_dev, const float* old_logp_dev,
                const float* adv_dev, const float* returns_dev, int n_rows, int n_actions, size_t row_stride, int act_type,
                float clip_lo, float clip_hi, float value_coef, float entropy_coef, float* row_terms_out_dev, float* sums_out_dev,
                void* workspace_dev, uint64_t* bad_rows_dev, void* stream);

int sf_ppo_loss_backward(const float* logits_dev, const float* values_dev, const void* actions_dev, const float* old_logp_dev,
                         const float* adv_dev, const float* returns_dev, int n_rows, int n_actions, size_t row_stride, int act_type,
                         float clip_lo, float clip_hi, float value_coef, float entropy_coef, const float* grad_loss_dev,
                         float* grad_logits_out_dev, size_t grad_row_stride, float* grad_values_out_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SFMI_PPO_H */
