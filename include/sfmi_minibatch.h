/* sfmi_minibatch.h -- the stretch of the PPO update between compute_returns and the loss: the normalised advantages
 * (rl/train.py:107-108) and the minibatches of rl/storage.py:65-122, each minibatch in one gather launch whose cursor lives on
 * the device.
 *
 * The calls are exported by libsfmi.so next to sfmi_ppo.h's.  All of them are plain stream work: no batch handle, no
 * allocation, no synchronise; they can be captured in a HIP graph.  The translation unit is compiled without contraction.
 *
 * sf_advantages:  returns_dev and values_dev are float32; their first M elements are the trainer's returns[:-1] and
 *   value_preds[:-1] (contiguous prefixes of the [T + 1, n, 1] tensors, M = T n).  Operation by operation:
 *     raw[i] = ret[i] - val[i]                               float32 (torch's own subtraction: the same bits)
 *     mean   = (sum_i (double)raw[i]) / (double)M            a float64 sum in a FIXED order
 *     S2     = sum_i ((double)raw[i] - mean)^2               float64, the same order (a second pass over the data, not
 *                                                            sum x^2 - (sum x)^2 / M, which cancels)
 *     std    = sqrt(S2 / (double)(M - 1))                    torch.std's unbiased form; M == 1 gives 0/0 = NaN, as torch does
 *     out[i] = (raw[i] - (float)mean) / ((float)std + (float)eps)      float32, no contraction
 *   The fixed order is sf_ppo_loss's (sfmi_ppo.h), by the same code: a fixed shuffle tree within the wave (lane l takes lane
 *   l ^ 32, then ^ 16, ... ^ 1), the four waves of a 256-lane block in index order, the blocks in index order.  No float atomic
 *   is used: two calls on equal inputs give equal bits.  A NaN or an inf in the input propagates by IEEE rules -- every
 *   element of adv_out is NaN then, as torch's are.
 *   adv_out_dev: float32 [M].  raw_out_dev: float32 [M], may be NULL.  stats_out_dev: double [2] = (mean, std), may be NULL.
 *   workspace_dev: sf_advantages_workspace_bytes(M) bytes, 8-byte aligned, caller-owned; holds the blocks' partial sums between
 *   the three launches of the call (the differences; the squares; the division).
 *
 * sf_minibatch_gather:  ONE launch copies row r = 0 .. mb-1 of a minibatch out of up to SF_MB_MAX_COLUMNS columns at once.
 *   A column is (src_dev, row_bytes, dst_dev): n_rows_src rows of row_bytes bytes at src_dev, mb rows at dst_dev, both dense.
 *   With c the cursor's value at launch (*cursor_dev, a uint32 on the device; or the argument `first` where cursor_dev is NULL):
 *     flat mode (traj_T == 0):            j = c * mb + r,              g = index[j]
 *     trajectory mode (traj_T = T > 0):   the index holds ENVS, mb = per * T and n_rows_src = T * traj_n:
 *                                         j = c * per + r / T,  e = index[j],  t = r % T,  g = t * traj_n + e
 *                                         (the order recurrent_generator's cat produces: env by env, step by step)
 *   and every column copies row_bytes bytes from src + g * row_bytes to dst + r * row_bytes; idx_out_dev[r] = g (int64 [mb],
 *   may be NULL).  index_dev: n_index elements, int32 or int64 (idx_type 4 / 8, as sf_gather_stacks takes them).  Duplicate
 *   indices are legal.
 *   BAD ROWS.  A g outside [0, n_rows_src), a j at or beyond n_index, a cursor at or beyond n_batches: the row is written as
 *   zeros in every column, idx_out[r] = -1, and the row is counted in *errors_dev (uint64, may be NULL) -- one vector atomic
 *   per wave that saw one.
 *   THE CURSOR.  With a non-NULL cursor_dev the cursor holds (c + 1) % n_batches after the call (a cursor at or beyond
 *   n_batches stays as it is), so a graph that captured ONE call yields minibatch 0, 1, 2, ... on successive replays.  The
 *   advance is a one-thread launch behind the gather on the same stream: stream order puts it behind every block's read.
 *   row_bytes: a multiple of 4 in [4, 65 536]; src_dev and dst_dev 4-byte aligned.  A column whose row_bytes is a multiple
 *   of 16 and whose two pointers are 16-byte aligned moves 16 bytes per lane, every other one 4.
 *
 * SF_ERR_ARG (with a text, nothing launched): sf_advantages -- a NULL returns, values, adv_out or workspace; M <= 0; a float
 *   array not 4-byte aligned; stats_out or the workspace not 8-byte aligned.  sf_minibatch_gather -- a NULL table or index;
 *   n_cols outside [1, SF_MB_MAX_COLUMNS]; a NULL src or dst, a misaligned one, a bad row_bytes; n_rows_src <= 0; n_index < 0;
 *   mb <= 0; n_batches == 0; an idx_type other than 4 or 8; traj_T < 0, or traj_T > 0 with mb not a multiple of it, traj_n <= 0
 *   or n_rows_src != traj_T * traj_n; index_dev not aligned to its element; cursor_dev not 4-byte, idx_out_dev or errors_dev
 *   not 8-byte aligned. */
#ifndef SFMI_MINIBATCH_H
#define SFMI_MINIBATCH_H

#include "sfmi.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SF_MB_MAX_COLUMNS 8
#define SF_MB_MAX_ROW_BYTES 65536

typedef struct sf_mb_column {
  const void* src_dev;
  size_t row_bytes;
  void* dst_dev;
} sf_mb_column;

size_t sf_advantages_workspace_bytes(int M);

int sf_advantages(const float* returns_dev, const float* values_dev, int M, double eps, float* adv_out_dev, float* raw_out_dev,
                  double* stats_out_dev, void* workspace_dev, void* stream);

int sf_minibatch_gather(const sf_mb_column* columns, int n_cols, int64_t n_rows_src, const void* index_dev, int idx_type,
                        int64_t n_index, int mb, uint32_t* cursor_dev, uint32_t first, uint32_t n_batches, int traj_T, int64_t traj_n,
                        int64_t* idx_out_dev, uint64_t* errors_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SFMI_MINIBATCH_H */
