// sf_minibatch.hip -- between compute_returns and the loss (include/sfmi_minibatch.h): the normalised advantages of
// rl/train.py:107-108 with a fixed arithmetic, and the minibatches of rl/storage.py:65-122 as one gather launch each.
//
//   sf_adv_sum_kernel      raw = ret - val (stored where asked for), the blocks' partial sums of (double)raw.
//   sf_adv_dev_kernel      every block adds the partial sums up in index order (the same total in every block: no launch of
//                          one block in between), mean = total / M, then the blocks' partial sums of ((double)raw - mean)^2.
//   sf_adv_apply_kernel    every block adds both rows of partial sums up again, mean and std, the float32 division; block 0
//                          writes the two statistics.
//   The sums are sf_fixed_sum.h's, the code sf_ppo_loss runs: one element per lane, the tree, the waves, the blocks.
//
//   sf_mb_gather_kernel    a block of 256 lanes per 64 output rows.  Wave 0 turns the cursor and the index into the 64 source
//                          rows (LDS), writes idx_out and counts the bad ones; then, column by column, the block walks the
//                          DESTINATION bytes of its 64 rows in order, 16 (or 4) bytes per lane: a 4-byte column is a lane per
//                          row, a 1 KiB row is 64 lanes across the row, and whatever lies between is as dense as the
//                          destination, which leaves as full lines.  The source side reads whole rows, each contiguous.
//   sf_mb_advance_kernel   one thread: cursor = (cursor + 1) % n_batches, behind the gather in stream order.
//
// Plain global loads and stores only.  Compiled with -ffp-contract=off like the rest.
#include <hip/hip_runtime.h>

#include "sf_fixed_sum.h"
#include "sf_internal.h"
#include "sfmi_minibatch.h"

namespace {

// ------------------------------------------------------------------------------------------------------------ advantages
__global__ __launch_bounds__(SF_SUM_BLOCK) void sf_adv_sum_kernel(const float* __restrict__ ret, const float* __restrict__ val, int n,
                                                                  float* __restrict__ raw_out, double* __restrict__ part1) {
  __shared__ double part[4][1];
  const size_t gi = (size_t)blockIdx.x * SF_SUM_BLOCK + threadIdx.x;
  const bool live = gi < (size_t)n;
  const size_t i = live ? gi : (size_t)n - 1;  // (a lane beyond n reads the last element and contributes nothing: no lane
                                               // leaves in front of the shuffles and the barrier)
  const float raw = ret[i] - val[i];
  if (live && raw_out) raw_out[i] = raw;
  double v[1] = {live ? (double)raw : 0.0};
  sf_block_partials<1>(v, part, part1);
}

// the total of a row of partial sums, the same in every lane of every block
__device__ __forceinline__ double sf_adv_total(const double* __restrict__ partials, int nblocks, double* buf, double* tot) {
  const double acc = sf_blocks_in_order<1>(partials, nblocks, buf);
  if (threadIdx.x == 0) *tot = acc;
  __syncthreads();
  return *tot;
}

__global__ __launch_bounds__(SF_SUM_BLOCK) void sf_adv_dev_kernel(const float* __restrict__ ret, const float* __restrict__ val, int n,
                                                                  const double* __restrict__ part1, double* __restrict__ part2) {
  __shared__ double buf[SF_SUM_CHUNK];
  __shared__ double part[4][1];
  __shared__ double tot;
  const double mean = sf_adv_total(part1, (int)gridDim.x, buf, &tot) / (double)n;
  const size_t gi = (size_t)blockIdx.x * SF_SUM_BLOCK + threadIdx.x;
  const bool live = gi < (size_t)n;
  const size_t i = live ? gi : (size_t)n - 1;
  const float raw = ret[i] - val[i];
  const double d = (double)raw - mean;
  double v[1] = {live ? d * d : 0.0};
  sf_block_partials<1>(v, part, part2);
}

__global__ __launch_bounds__(SF_SUM_BLOCK) void sf_adv_apply_kernel(const float* __restrict__ ret, const float* __restrict__ val, int n,
                                                                    float eps, const double* __restrict__ part1,
                                                                    const double* __restrict__ part2, float* __restrict__ out,
                                                                    double* __restrict__ stats) {
  __shared__ double buf[SF_SUM_CHUNK];
  __shared__ double tot1, tot2;
  const double mean = sf_adv_total(part1, (int)gridDim.x, buf, &tot1) / (double)n;
  const double S2 = sf_adv_total(part2, (int)gridDim.x, buf, &tot2);
  const double sd = sqrt(S2 / (double)(n - 1));
  if (stats && blockIdx.x == 0 && threadIdx.x == 0) {
    stats[0] = mean;
    stats[1] = sd;
  }
  const size_t i = (size_t)blockIdx.x * SF_SUM_BLOCK + threadIdx.x;
  if (i >= (size_t)n) return;
  const float raw = ret[i] - val[i];
  out[i] = (raw - (float)mean) / ((float)sd + eps);
}

// ---------------------------------------------------------------------------------------------------------------- gather
#define SF_MB_TILE 64  // output rows per block: wave 0 holds a row's index per lane

struct SfMbColumns {
  const unsigned char* src[SF_MB_MAX_COLUMNS];
  unsigned char* dst[SF_MB_MAX_COLUMNS];
  unsigned row_bytes[SF_MB_MAX_COLUMNS];
  int n;
};

// the `rows` rows of one column whose source rows are g[0 .. rows-1] (-1: zeros), V at a time, in the destination's order
template <typename V>
__device__ __forceinline__ void sf_mb_copy(const unsigned char* __restrict__ src, unsigned char* __restrict__ dst, unsigned row_bytes,
                                           int rows, const long long* g) {
  const unsigned upr = row_bytes / (unsigned)sizeof(V);  // units per row
  const unsigned total = (unsigned)rows * upr;           // (at most 64 x 16 384)
  V* const out = reinterpret_cast<V*>(dst);
  for (unsigned u = threadIdx.x; u < total; u += 256) {
    const unsigned r = u / upr, k = u - r * upr;
    const long long gr = g[r];
    V v = {};
    if (gr >= 0) v = reinterpret_cast<const V*>(src + (size_t)gr * row_bytes)[k];
    out[u] = v;
  }
}

__global__ __launch_bounds__(256) void sf_mb_gather_kernel(SfMbColumns C, long long n_rows_src, const void* __restrict__ index, int idx64,
                                                           long long n_index, int mb, const unsigned* __restrict__ cursor, unsigned first,
                                                           unsigned n_batches, int traj_T, long long traj_n, long long* __restrict__ idx_out,
                                                           unsigned long long* errors) {
  __shared__ long long g[SF_MB_TILE];
  const int r0 = (int)blockIdx.x * SF_MB_TILE;
  const int rows = mb - r0 < SF_MB_TILE ? mb - r0 : SF_MB_TILE;
  if (threadIdx.x < SF_MB_TILE) {  // wave 0
    const int r = r0 + (int)threadIdx.x;
    const bool live = (int)threadIdx.x < rows;
    const unsigned c = cursor ? *cursor : first;
    long long gr = -1;
    if (live && c < n_batches) {
      long long j, t = 0;
      if (traj_T > 0) {
        j = (long long)c * (mb / traj_T) + r / traj_T;
        t = r % traj_T;
      } else {
        j = (long long)c * mb + r;
      }
      if (j < n_index) {
        const long long e = idx64 ? reinterpret_cast<const long long*>(index)[j] : (long long)reinterpret_cast<const int*>(index)[j];
        // (t * traj_n < n_rows_src: an e beyond +-n_rows_src cannot give a row, and the sum below cannot overflow)
        if (e > -n_rows_src && e < n_rows_src) {
          const long long cand = t * traj_n + e;
          if (cand >= 0 && cand < n_rows_src) gr = cand;
        }
      }
    }
    g[threadIdx.x] = gr;
    if (live && idx_out) idx_out[r] = gr;
    const bool bad = live && gr < 0;
    if (errors) {  // one atomic per wave that saw a bad row
      const unsigned long long votes = __ballot(bad);
      if (bad && (unsigned)__lane_id() == (unsigned)__builtin_ctzll(votes)) atomicAdd(errors, (unsigned long long)__popcll(votes));
    }
  }
  __syncthreads();
  for (int col = 0; col < C.n; col++) {
    const unsigned rb = C.row_bytes[col];
    const unsigned char* const src = C.src[col];
    unsigned char* const dst = C.dst[col] + (size_t)r0 * rb;
    const bool wide = (rb & 15u) == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(C.dst[col])) & 15u) == 0;
    if (wide)
      sf_mb_copy<uint4>(src, dst, rb, rows, g);
    else
      sf_mb_copy<unsigned>(src, dst, rb, rows, g);
  }
}

__global__ void sf_mb_advance_kernel(unsigned* cursor, unsigned n_batches) {
  const unsigned c = *cursor;
  if (c < n_batches) *cursor = c + 1 < n_batches ? c + 1 : 0;
}

int sf_mb_launched(const char* who) {
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) {
    sf_set_error("%s: %s", who, hipGetErrorString(err));
    return SF_ERR_HIP;
  }
  return SF_OK;
}

inline bool sf_mb_misaligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

inline unsigned sf_adv_blocks(int M) { return (unsigned)(((size_t)M + SF_SUM_BLOCK - 1) / SF_SUM_BLOCK); }

}  // namespace

extern "C" size_t sf_advantages_workspace_bytes(int M) { return M > 0 ? (size_t)sf_adv_blocks(M) * 2 * sizeof(double) : 0; }

extern "C" int sf_advantages(const float* returns_dev, const float* values_dev, int M, double eps, float* adv_out_dev, float* raw_out_dev,
                             double* stats_out_dev, void* workspace_dev, void* stream) {
  const char* who = "sf_advantages";
  if (!returns_dev || !values_dev || !adv_out_dev) {
    sf_set_error("%s: returns_dev, values_dev and adv_out_dev must not be null", who);
    return SF_ERR_ARG;
  }
  if (M <= 0) {
    sf_set_error("%s: M %d: need at least one element", who, M);
    return SF_ERR_ARG;
  }
  if (sf_mb_misaligned(returns_dev, 4) || sf_mb_misaligned(values_dev, 4) || sf_mb_misaligned(adv_out_dev, 4) ||
      sf_mb_misaligned(raw_out_dev, 4)) {
    sf_set_error("%s: returns_dev, values_dev, adv_out_dev and raw_out_dev must be 4-byte aligned", who);
    return SF_ERR_ARG;
  }
  if (sf_mb_misaligned(stats_out_dev, 8)) {
    sf_set_error("%s: stats_out_dev must be 8-byte aligned", who);
    return SF_ERR_ARG;
  }
  if (!workspace_dev || sf_mb_misaligned(workspace_dev, 8)) {
    sf_set_error("%s: workspace_dev must be %zu bytes (sf_advantages_workspace_bytes), 8-byte aligned, not null", who,
                 sf_advantages_workspace_bytes(M));
    return SF_ERR_ARG;
  }
  const dim3 grid(sf_adv_blocks(M)), block(SF_SUM_BLOCK);
  hipStream_t s = (hipStream_t)stream;
  double* const part1 = reinterpret_cast<double*>(workspace_dev);
  double* const part2 = part1 + grid.x;
  hipLaunchKernelGGL(sf_adv_sum_kernel, grid, block, 0, s, returns_dev, values_dev, M, raw_out_dev, part1);
  hipLaunchKernelGGL(sf_adv_dev_kernel, grid, block, 0, s, returns_dev, values_dev, M, part1, part2);
  hipLaunchKernelGGL(sf_adv_apply_kernel, grid, block, 0, s, returns_dev, values_dev, M, (float)eps, part1, part2, adv_out_dev,
                     stats_out_dev);
  return sf_mb_launched(who);
}

extern "C" int sf_minibatch_gather(const sf_mb_column* columns, int n_cols, int64_t n_rows_src, const void* index_dev, int idx_type,
                                   int64_t n_index, int mb, uint32_t* cursor_dev, uint32_t first, uint32_t n_batches, int traj_T,
                                   int64_t traj_n, int64_t* idx_out_dev, uint64_t* errors_dev, void* stream) {
  const char* who = "sf_minibatch_gather";
  if (!columns || !index_dev) {
    sf_set_error("%s: columns and index_dev must not be null", who);
    return SF_ERR_ARG;
  }
  if (n_cols < 1 || n_cols > SF_MB_MAX_COLUMNS) {
    sf_set_error("%s: n_cols %d outside [1, %d]", who, n_cols, SF_MB_MAX_COLUMNS);
    return SF_ERR_ARG;
  }
  if (n_rows_src <= 0 || n_index < 0 || mb <= 0 || n_batches == 0) {
    sf_set_error("%s: need n_rows_src > 0, n_index >= 0, mb > 0 and n_batches > 0 (got %lld, %lld, %d, %u)", who, (long long)n_rows_src,
                 (long long)n_index, mb, n_batches);
    return SF_ERR_ARG;
  }
  if (idx_type != SF_ACT_I32 && idx_type != SF_ACT_I64) {
    sf_set_error("%s: idx_type must be 4 or 8 (got %d)", who, idx_type);
    return SF_ERR_ARG;
  }
  if (traj_T < 0 || (traj_T > 0 && (mb % traj_T != 0 || traj_n <= 0 || n_rows_src / traj_T != traj_n || n_rows_src % traj_T != 0))) {
    sf_set_error("%s: trajectory mode needs traj_T > 0, mb a multiple of it, traj_n > 0 and n_rows_src = traj_T * traj_n "
                 "(got traj_T %d, mb %d, traj_n %lld, n_rows_src %lld)", who, traj_T, mb, (long long)traj_n, (long long)n_rows_src);
    return SF_ERR_ARG;
  }
  if (sf_mb_misaligned(index_dev, (unsigned)idx_type) || sf_mb_misaligned(cursor_dev, 4) || sf_mb_misaligned(idx_out_dev, 8) ||
      sf_mb_misaligned(errors_dev, 8)) {
    sf_set_error("%s: index_dev must be aligned to its element, cursor_dev to 4 bytes, idx_out_dev and errors_dev to 8", who);
    return SF_ERR_ARG;
  }
  SfMbColumns C = {};
  C.n = n_cols;
  for (int k = 0; k < n_cols; k++) {
    const sf_mb_column& c = columns[k];
    if (!c.src_dev || !c.dst_dev || sf_mb_misaligned(c.src_dev, 4) || sf_mb_misaligned(c.dst_dev, 4)) {
      sf_set_error("%s: column %d: src_dev and dst_dev must be 4-byte aligned, not null", who, k);
      return SF_ERR_ARG;
    }
    if (c.row_bytes < 4 || c.row_bytes > SF_MB_MAX_ROW_BYTES || (c.row_bytes & 3) != 0) {
      sf_set_error("%s: column %d: row_bytes %zu must be a multiple of 4 in [4, %d]", who, k, c.row_bytes, SF_MB_MAX_ROW_BYTES);
      return SF_ERR_ARG;
    }
    C.src[k] = reinterpret_cast<const unsigned char*>(c.src_dev);
    C.dst[k] = reinterpret_cast<unsigned char*>(c.dst_dev);
    C.row_bytes[k] = (unsigned)c.row_bytes;
  }
  const dim3 grid((unsigned)(((size_t)mb + SF_MB_TILE - 1) / SF_MB_TILE)), block(256);
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(sf_mb_gather_kernel, grid, block, 0, s, C, (long long)n_rows_src, index_dev, idx_type == SF_ACT_I64 ? 1 : 0,
                     (long long)n_index, mb, (const unsigned*)cursor_dev, first, n_batches, traj_T, (long long)traj_n,
                     reinterpret_cast<long long*>(idx_out_dev), reinterpret_cast<unsigned long long*>(errors_dev));
  if (cursor_dev) hipLaunchKernelGGL(sf_mb_advance_kernel, dim3(1), dim3(1), 0, s, cursor_dev, n_batches);
  return sf_mb_launched(who);
}
