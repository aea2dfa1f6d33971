/* sfmi_optim.h -- the two lines that end every PPO update (rl/train.py:131-132): clip_grad_norm_ over all parameters and one
 * Adam step, for a whole table of float32 tensors, in three launches whose bookkeeping lives on the device.
 *
 * The calls are exported by libsfmi.so next to sfmi_ppo.h's.  All of them are plain stream work: no batch handle, no
 * allocation, no synchronise; they can be captured in a HIP graph.  The translation unit is compiled without contraction.
 *
 * sf_adam_step:  one optimiser step for tensors[0 .. n_tensors-1], n_tensors in [1, SF_OPT_MAX_TENSORS].  The table is read on the
 *   host during the call and travels to the kernels BY VALUE, in their arguments: a caller may build it afresh per call (eager
 *   .grad pointers move) and a captured graph keeps the one it was captured with.  Every tensor is dense float32, numel > 0, its
 *   four pointers 4-byte aligned; param, exp_avg and exp_avg_sq are updated in place, grad is only read.
 *
 *   CHUNKS.  A tensor is cut into chunks of SF_OPT_CHUNK = 2048 elements (the last one may be short); chunk order is table order,
 *   then offset; a block of 256 lanes takes one chunk in the first and in the third launch.  Lane l of the block holds the
 *   elements 4 l .. 4 l + 3 and 1024 + 4 l .. 1024 + 4 l + 3 of its chunk.  Where all four pointers of a tensor are 16-byte aligned
 *   a lane moves each group of four that lies wholly inside the tensor as 16 bytes; the tensor's last numel % 4 elements, and
 *   every element of a tensor with a pointer that is only 4-byte aligned, move 4 bytes at a time.  The arithmetic does not depend
 *   on the path.
 *
 *   THE NORM (launch 1: the chunks' partial sums; launch 2: one block).  With g the concatenation of all grads in table order
 *     S    = sum (double)g * (double)g             every product is exact; the sum is float64 in a FIXED order:
 *              in a lane:  acc = 0, then acc = acc + (the product) over the lane's up to eight elements in ascending index
 *                          (an element beyond the tensor's end contributes +0.0)
 *              in a chunk: sf_fixed_sum.h's order over the 256 lane values, by that header's code -- the tree within the wave
 *                          (lane l takes lane l ^ 32, then ^ 16, ... ^ 1), the four waves in index order
 *              the chunks in index order, one running sum from 0.0
 *     norm = sqrt(S)
 *     coef = min(1, max_grad_norm / (norm + 1e-6))                float64; clip_grad_norm_'s expression and clamp
 *   max_grad_norm <= 0 (or a NaN): no clipping, coef = 1; the norm is computed all the same.  No float atomic is used: equal inputs
 *   give equal bits.
 *
 *   THE STATE BLOCK.  state_dev: SF_ADAM_STATE_BYTES = 128 bytes, 16-byte aligned, made by sf_adam_state_init:
 *     offset  0  int64   t            steps taken
 *             8  double  beta1_pow    beta1^t as a running product: 1.0 at t = 0, multiplied by beta1 once per step (no pow)
 *            16  double  beta2_pow    beta2^t, likewise
 *            24  double  lr           read at every step: whoever rewrites it (a scheduler) changes the next step, a replay of a
 *                                     captured call included
 *            32  double  beta1
 *            40  double  beta2
 *            48  double  eps
 *            56  double  norm         of the last call (an inf or a NaN where the step was skipped)
 *            64  double  coef         of the last call (0.0 where the step was skipped)
 *            72  uint64  skipped      calls that were skipped, see below
 *            80  float   [8]          the last step's float32 scalars as the update reads them:
 *                                     coef, b1, 1 - b1, b2, 1 - b2, sqrt(bc2), eps, step_size
 *           112  uint32  apply        1: the last call stepped; 0: it was skipped
 *           116  ..      zero
 *   Launch 2 finishes the sum and, where S is finite, in float64:
 *     t = t + 1;  beta1_pow = beta1_pow * beta1;  beta2_pow = beta2_pow * beta2
 *     bc1 = 1 - beta1_pow;  bc2 = 1 - beta2_pow;  step_size = lr / bc1;  the float32 scalars are (float) of coef, beta1,
 *     1.0 - beta1, beta2, 1.0 - beta2, sqrt(bc2), eps, step_size
 *   so a captured call performs step t, t + 1, t + 2, ... on successive replays.
 *
 *   THE UPDATE (launch 3), per element in float32, operation by operation, no contraction (torch.optim.Adam's order with
 *   weight_decay = 0, amsgrad = False, maximize = False):
 *     g  = grad * coef
 *     m' = b1 * m + (1 - b1) * g
 *     v' = b2 * v + ((1 - b2) * g) * g
 *     d  = sqrt(v') / sqrt(bc2) + eps
 *     p' = p - step_size * (m' / d)
 *   m', v' and p' are stored.  The division and the square root are correctly rounded.  The multiplication by coef is made in
 *   every call: coef = 1 gives g = grad exactly.  The grads are NOT written: norm and coef in the state block are what
 *   clip_grad_norm_'s return value and its scaling were for.
 *
 *   NON-FINITE GRADIENTS.  S not finite (a NaN or an inf in any grad, or a sum of squares beyond float64): the step is SKIPPED.
 *   No parameter, moment, t or running product changes, byte for byte; `skipped` goes up by one and so does *errors_dev (uint64,
 *   may be NULL; one vector atomic from one lane).  This differs from torch on purpose: clip_grad_norm_ with its default
 *   error_if_nonfinite=False multiplies every grad by NaN, and Adam then writes NaN into every parameter and moment.
 *
 *   workspace_dev: sf_adam_workspace_bytes(total chunks) bytes, 8-byte aligned, caller-owned: the chunks' partial sums between
 *   launches 1 and 2.  total chunks = sum over the table of sf_adam_chunks(numel).
 *
 * sf_adam_state_init:  t = 0, both products 1.0, skipped = 0, norm = coef = 0 and the four hyper-parameters; a one-thread launch.
 *
 * SF_ERR_ARG (with a text, nothing launched): sf_adam_step -- a NULL table, state or workspace; n_tensors outside
 *   [1, SF_OPT_MAX_TENSORS]; a NULL param, grad, exp_avg or exp_avg_sq, or one not 4-byte aligned; numel <= 0; more than
 *   SF_OPT_MAX_CHUNKS chunks in all; state_dev not 16-byte, workspace_dev or errors_dev not 8-byte aligned.  sf_adam_state_init --
 *   a NULL or misaligned state_dev; lr, eps negative or not finite; a beta outside [0, 1).
 *
 * Out of scope: weight_decay != 0, amsgrad, maximize, more than one parameter group. */
#ifndef SFMI_OPTIM_H
#define SFMI_OPTIM_H

#include "sfmi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SF_OPT_MAX_TENSORS 64
#define SF_OPT_CHUNK 2048
#define SF_OPT_MAX_CHUNKS (1 << 30)
#define SF_ADAM_STATE_BYTES 128

typedef struct sf_opt_tensor {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t numel;
} sf_opt_tensor;

int64_t sf_adam_chunks(int64_t numel);

size_t sf_adam_workspace_bytes(int64_t total_chunks);

size_t sf_adam_state_bytes(void);

int sf_adam_state_init(void* state_dev, double lr, double beta1, double beta2, double eps, void* stream);

int sf_adam_step(const sf_opt_tensor* tensors, int n_tensors, double max_grad_norm, void* state_dev, void* workspace_dev,
                 uint64_t* errors_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SFMI_OPTIM_H */
