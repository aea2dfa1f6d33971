// sf_policy_eval.hip -- the policy head's update side (include/sfmi_ppo.h): what the reference's PPO update does to the logits
// of a minibatch (rl/networks.py:78-86: softmax, log_softmax, gather, the entropy; rl/train.py:123-129: the clipped surrogate, the
// three means, the weighted sum) and what autograd does on the way back, as one launch each way (the loss's forward: two).
//
//   sf_eval_kernel<AMAX>        one lane per row, the row in registers (AMAX = 4, 8, 16 or 32, the loops unrolled to AMAX and
//                               cut at A by a wave-uniform compare, as in sf_policy.hip): logp of the given action, the entropy.
//   sf_eval_bwd_kernel<AMAX>    the same row again, then the A gradient entries of the header's formula.
//   sf_ppo_loss_kernel<AMAX>    the row, r, s, q, H; the three terms as float64 through a fixed xor tree of the wave, the block's
//                               four waves in index order through LDS, one partial triple per block into the workspace.
//   sf_ppo_finish_kernel        one block: the partial triples in index order (staged through LDS 1024 blocks at a time, three
//                               lanes add), the division by M, the rounding, the weighted sum.
//   sf_ppo_loss_bwd_kernel<AMAX> the row and r again, the three factors, the gradient entries and the value's gradient.
//
// The row arithmetic restates sf_policy.hip's operation for operation (m, d, expf, the float64 running sum, logf, the float32
// dot with its skipped terms), and both units are compiled with -ffp-contract=off: the log-probability recomputed here for an
// action sf_policy_sample played is the one it stored, bit for bit (tests/test_gpu_policy_eval.py holds that).
// Nothing here is bound by anything but launch latency (327 680 x 5 floats = 6.5 MB); there is no LDS in the row passes.
#include <hip/hip_runtime.h>

#include "sf_fixed_sum.h"
#include "sf_internal.h"
#include "sfmi_ppo.h"

namespace {

template <int AMAX>
struct SfRow {
  float d[AMAX], e[AMAX];  // x[k] - m (x[k] itself on a bad row), expf of it
  float Sf, lse, H, da;  // da: d[a] of the row's action
  bool bad;
};

// the row of sfmi_ppo.h; `bad` comes in as "the action is out of range" and leaves as the row's verdict.  d[a] is picked up by
// a compare per unrolled k: indexing the register array with a would send it to scratch
template <int AMAX>
__device__ __forceinline__ void sf_row_eval(const float* __restrict__ row, int A, int a, bool bad, SfRow<AMAX>& R) {
  const float inf = __builtin_inff();
  float m = -inf;
#pragma unroll
  for (int k = 0; k < AMAX; k++) {
    R.d[k] = k < A ? row[k] : -inf;
    if (k < A) {
      bad = bad || !(R.d[k] < inf);
      if (R.d[k] > m) m = R.d[k];
    }
  }
  bad = bad || m == -inf;
  if (bad) m = 0.0f;  // (the arithmetic below stays defined; its results are not used)
  double S = 0.0;
  float dot = 0.0f, da = 0.0f;
#pragma unroll
  for (int k = 0; k < AMAX; k++) {
    R.e[k] = 0.0f;
    if (k < A) {
      const float d = R.d[k] - m;
      R.d[k] = d;
      da = k == a ? d : da;
      R.e[k] = bad ? 0.0f : expf(d);
      S = S + (double)R.e[k];
      if (R.e[k] != 0.0f) dot = dot + R.e[k] * d;
    }
  }
  R.Sf = (float)S;
  R.lse = logf(R.Sf);
  R.H = R.lse - dot / R.Sf;
  R.da = da;
  R.bad = bad;
}

// the action of row i and whether it lies outside [0, A); an action outside reads as 0
__device__ __forceinline__ int sf_row_action(const void* actions, int act_type, size_t i, int A, bool& outside) {
  long long a;
  if (act_type == SF_ACT_U8)
    a = (long long)reinterpret_cast<const uint8_t*>(actions)[i];
  else if (act_type == SF_ACT_I32)
    a = (long long)reinterpret_cast<const int32_t*>(actions)[i];
  else
    a = (long long)reinterpret_cast<const int64_t*>(actions)[i];
  outside = a < 0 || a >= (long long)A;
  return outside ? 0 : (int)a;
}

// the gradient entries k < A of one logits row (sfmi_ppo.h: sf_policy_evaluate_backward)
template <int AMAX>
__device__ __forceinline__ void sf_row_grad(const SfRow<AMAX>& R, int A, int a, float gl, float gH, float* __restrict__ out) {
  const float inf = __builtin_inff();
#pragma unroll
  for (int k = 0; k < AMAX; k++) {
    if (k < A) {
      const float p = R.e[k] / R.Sf;
      const float t1 = gl * ((k == a ? 1.0f : 0.0f) - p);
      float t2 = 0.0f;
      if (R.e[k] != 0.0f) t2 = (gH * p) * ((R.d[k] - R.lse) + R.H);
      float g = t1 - t2;
      if (R.d[k] == -inf) g = 0.0f;  // a masked logit is a constant
      if (R.bad) g = __builtin_nanf("");
      out[k] = g;
    }
  }
}

__device__ __forceinline__ void sf_count_bad(bool bad, unsigned long long* bad_rows) {
  if (bad_rows) {  // one atomic per wave that saw a bad row
    const unsigned long long votes = __ballot(bad);
    if (bad && (unsigned)__lane_id() == (unsigned)__builtin_ctzll(votes)) atomicAdd(bad_rows, (unsigned long long)__popcll(votes));
  }
}

template <int AMAX>
__global__ __launch_bounds__(256) void sf_eval_kernel(const float* __restrict__ logits, int n, int A, size_t row_stride,
                                                      const void* __restrict__ actions, int act_type, float* logp_out, float* entropy_out,
                                                      unsigned long long* bad_rows) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)n) return;
  bool outside;
  const int a = sf_row_action(actions, act_type, i, A, outside);
  SfRow<AMAX> R;
  sf_row_eval<AMAX>(logits + i * row_stride, A, a, outside, R);
  float logp = R.da - R.lse, ent = R.H;
  if (R.bad) logp = ent = __builtin_nanf("");
  if (logp_out) logp_out[i] = logp;
  if (entropy_out) entropy_out[i] = ent;
  sf_count_bad(R.bad, bad_rows);
}

template <int AMAX>
__global__ __launch_bounds__(256) void sf_eval_bwd_kernel(const float* __restrict__ logits, int n, int A, size_t row_stride,
                                                          const void* __restrict__ actions, int act_type,
                                                          const float* __restrict__ grad_logp, const float* __restrict__ grad_entropy,
                                                          float* __restrict__ grad_logits, size_t grad_row_stride) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)n) return;
  bool outside;
  const int a = sf_row_action(actions, act_type, i, A, outside);
  SfRow<AMAX> R;
  sf_row_eval<AMAX>(logits + i * row_stride, A, a, outside, R);
  const float gl = grad_logp ? grad_logp[i] : 0.0f, gH = grad_entropy ? grad_entropy[i] : 0.0f;
  sf_row_grad<AMAX>(R, A, a, gl, gH, grad_logits + i * grad_row_stride);
}

// r, and the surrogate's two products, of one row (sfmi_ppo.h: sf_ppo_loss)
struct SfSurr {
  float r, s1, s2, s;
};
__device__ __forceinline__ SfSurr sf_surrogate(float logp, float old_logp, float adv, float clip_lo, float clip_hi) {
  SfSurr u;
  u.r = expf(logp - old_logp);
  const float c = u.r < clip_lo ? clip_lo : (u.r > clip_hi ? clip_hi : u.r);  // (a NaN passes through, as torch.clamp's does)
  u.s1 = u.r * adv;
  u.s2 = c * adv;
  u.s = (u.s1 < u.s2 || u.s1 != u.s1) ? u.s1 : u.s2;  // torch.min: the smaller one, a NaN if there is one
  return u;
}

template <int AMAX>
__global__ __launch_bounds__(256) void sf_ppo_loss_kernel(const float* __restrict__ logits, const float* __restrict__ values,
                                                          const void* __restrict__ actions, const float* __restrict__ old_logp,
                                                          const float* __restrict__ adv, const float* __restrict__ returns, int n, int A,
                                                          size_t row_stride, int act_type, float clip_lo, float clip_hi,
                                                          float* __restrict__ row_terms, double* __restrict__ partials,
                                                          unsigned long long* bad_rows) {
  __shared__ double part[4][3];
  const size_t gi = (size_t)blockIdx.x * 256 + threadIdx.x;
  const bool live = gi < (size_t)n;
  const size_t i = live ? gi : (size_t)n - 1;  // (a lane beyond n works on the last row and contributes nothing: no lane leaves
                                               // in front of the shuffles and the barrier)
  bool outside;
  const int a = sf_row_action(actions, act_type, i, A, outside);
  SfRow<AMAX> R;
  sf_row_eval<AMAX>(logits + i * row_stride, A, a, outside, R);
  const float logp = R.da - R.lse;
  const SfSurr u = sf_surrogate(logp, old_logp[i], adv[i], clip_lo, clip_hi);
  const float dv = values[i] - returns[i];
  float s = u.s, q = dv * dv, H = R.H;
  if (R.bad) s = q = H = __builtin_nanf("");
  if (live && row_terms) {
    row_terms[3 * i + 0] = s;
    row_terms[3 * i + 1] = q;
    row_terms[3 * i + 2] = H;
  }
  sf_count_bad(live && R.bad, bad_rows);
  // the fixed order (sf_fixed_sum.h): the tree in the wave, the block's four waves and then the blocks in index order
  double v[3] = {live ? (double)s : 0.0, live ? (double)q : 0.0, live ? (double)H : 0.0};
  sf_block_partials<3>(v, part, partials);
}

__global__ __launch_bounds__(256) void sf_ppo_finish_kernel(const double* __restrict__ partials, int nblocks, int n, float value_coef,
                                                            float entropy_coef, float* __restrict__ sums) {
  __shared__ double buf[SF_SUM_CHUNK * 3];
  __shared__ double tot[3];
  const int tid = threadIdx.x;
  const double acc = sf_blocks_in_order<3>(partials, nblocks, buf);
  if (tid < 3) tot[tid] = acc;
  __syncthreads();
  if (tid == 0) {
    const double M = (double)n;
    const float action_loss = (float)(-(tot[0] / M)), value_loss = (float)(tot[1] / M), entropy = (float)(tot[2] / M);
    sums[0] = action_loss;
    sums[1] = value_loss;
    sums[2] = entropy;
    sums[3] = (action_loss + value_coef * value_loss) - entropy_coef * entropy;
  }
}

template <int AMAX>
__global__ __launch_bounds__(256) void sf_ppo_loss_bwd_kernel(const float* __restrict__ logits, const float* __restrict__ values,
                                                              const void* __restrict__ actions, const float* __restrict__ old_logp,
                                                              const float* __restrict__ adv, const float* __restrict__ returns, int n,
                                                              int A, size_t row_stride, int act_type, float clip_lo, float clip_hi,
                                                              float value_coef, float entropy_coef, const float* __restrict__ grad_loss,
                                                              float* __restrict__ grad_logits, size_t grad_row_stride,
                                                              float* __restrict__ grad_values) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)n) return;
  bool outside;
  const int a = sf_row_action(actions, act_type, i, A, outside);
  SfRow<AMAX> R;
  sf_row_eval<AMAX>(logits + i * row_stride, A, a, outside, R);
  const float logp = R.da - R.lse;
  const float av = adv[i];
  const SfSurr u = sf_surrogate(logp, old_logp[i], av, clip_lo, clip_hi);
  const float gm = *grad_loss / (float)n;
  const bool pass = u.s1 < u.s2 || (clip_lo <= u.r && u.r <= clip_hi) || u.s1 != u.s1 || u.s2 != u.s2;
  const float cl = pass ? -((gm * av) * u.r) : 0.0f;
  const float cH = -(gm * entropy_coef);
  sf_row_grad<AMAX>(R, A, a, cl, cH, grad_logits + i * grad_row_stride);
  if (grad_values) {
    const float cv = (gm * value_coef) * (2.0f * (values[i] - returns[i]));
    grad_values[i] = R.bad ? __builtin_nanf("") : cv;
  }
}

// what every call refuses about the logits and the actions; 0 if fine
int sf_eval_args(const char* who, const void* logits, int n_rows, int n_actions, size_t row_stride, const void* actions, int act_type) {
  if (!logits || !actions) {
    sf_set_error("%s: logits_dev and actions_dev must not be null", who);
    return SF_ERR_ARG;
  }
  if (n_rows <= 0) {
    sf_set_error("%s: n_rows %d: need at least one row", who, n_rows);
    return SF_ERR_ARG;
  }
  if (n_actions < 1 || n_actions > SF_POLICY_MAX_ACTIONS) {
    sf_set_error("%s: n_actions %d outside [1, %d]", who, n_actions, SF_POLICY_MAX_ACTIONS);
    return SF_ERR_ARG;
  }
  if (row_stride < (size_t)n_actions) {
    sf_set_error("%s: row_stride %zu below n_actions %d", who, row_stride, n_actions);
    return SF_ERR_ARG;
  }
  if (act_type != SF_ACT_U8 && act_type != SF_ACT_I32 && act_type != SF_ACT_I64) {
    sf_set_error("%s: act_type %d (1, 4 or 8: the bytes of an action)", who, act_type);
    return SF_ERR_ARG;
  }
  if (((uintptr_t)logits & 3) != 0) {
    sf_set_error("%s: logits_dev must be 4-byte aligned", who);
    return SF_ERR_ARG;
  }
  return SF_OK;
}

int sf_eval_aligned4(const char* who, const char* what, const void* p) {
  if (((uintptr_t)p & 3) != 0) {
    sf_set_error("%s: %s must be 4-byte aligned", who, what);
    return SF_ERR_ARG;
  }
  return SF_OK;
}

int sf_eval_grad_args(const char* who, const void* grad_logits, size_t grad_row_stride, int n_actions) {
  if (!grad_logits) {
    sf_set_error("%s: grad_logits_out_dev must not be null", who);
    return SF_ERR_ARG;
  }
  if (grad_row_stride < (size_t)n_actions) {
    sf_set_error("%s: grad_row_stride %zu below n_actions %d", who, grad_row_stride, n_actions);
    return SF_ERR_ARG;
  }
  return sf_eval_aligned4(who, "grad_logits_out_dev", grad_logits);
}

int sf_ppo_args(const char* who, const float* values, const float* old_logp, const float* adv, const float* returns) {
  if (!values || !old_logp || !adv || !returns) {
    sf_set_error("%s: values_dev, old_logp_dev, adv_dev and returns_dev must not be null", who);
    return SF_ERR_ARG;
  }
  if (sf_eval_aligned4(who, "values_dev", values) || sf_eval_aligned4(who, "old_logp_dev", old_logp) ||
      sf_eval_aligned4(who, "adv_dev", adv) || sf_eval_aligned4(who, "returns_dev", returns))
    return SF_ERR_ARG;
  return SF_OK;
}

int sf_eval_launched(const char* who) {
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) {
    sf_set_error("%s: %s", who, hipGetErrorString(err));
    return SF_ERR_HIP;
  }
  return SF_OK;
}

inline unsigned sf_eval_blocks(int n_rows) { return (unsigned)(((size_t)n_rows + 255) / 256); }

}  // namespace

#define SF_EVAL_DISPATCH(KERNEL, ...)                                            \
  do {                                                                           \
    if (n_actions <= 4)                                                          \
      hipLaunchKernelGGL(KERNEL<4>, grid, block, 0, s, __VA_ARGS__);             \
    else if (n_actions <= 8)                                                     \
      hipLaunchKernelGGL(KERNEL<8>, grid, block, 0, s, __VA_ARGS__);             \
    else if (n_actions <= 16)                                                    \
      hipLaunchKernelGGL(KERNEL<16>, grid, block, 0, s, __VA_ARGS__);            \
    else                                                                         \
      hipLaunchKernelGGL(KERNEL<32>, grid, block, 0, s, __VA_ARGS__);            \
  } while (0)

extern "C" int sf_policy_evaluate(const float* logits_dev, int n_rows, int n_actions, size_t row_stride, const void* actions_dev,
                                  int act_type, float* logp_out_dev, float* entropy_out_dev, uint64_t* bad_rows_dev, void* stream) {
  const char* who = "sf_policy_evaluate";
  if (sf_eval_args(who, logits_dev, n_rows, n_actions, row_stride, actions_dev, act_type)) return SF_ERR_ARG;
  if (sf_eval_aligned4(who, "logp_out_dev", logp_out_dev) || sf_eval_aligned4(who, "entropy_out_dev", entropy_out_dev)) return SF_ERR_ARG;
  const dim3 grid(sf_eval_blocks(n_rows)), block(256);
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* const bad = reinterpret_cast<unsigned long long*>(bad_rows_dev);
  SF_EVAL_DISPATCH(sf_eval_kernel, logits_dev, n_rows, n_actions, row_stride, actions_dev, act_type, logp_out_dev, entropy_out_dev, bad);
  return sf_eval_launched(who);
}

extern "C" int sf_policy_evaluate_backward(const float* logits_dev, int n_rows, int n_actions, size_t row_stride, const void* actions_dev,
                                           int act_type, const float* grad_logp_dev, const float* grad_entropy_dev,
                                           float* grad_logits_out_dev, size_t grad_row_stride, void* stream) {
  const char* who = "sf_policy_evaluate_backward";
  if (sf_eval_args(who, logits_dev, n_rows, n_actions, row_stride, actions_dev, act_type)) return SF_ERR_ARG;
  if (sf_eval_grad_args(who, grad_logits_out_dev, grad_row_stride, n_actions)) return SF_ERR_ARG;
  if (sf_eval_aligned4(who, "grad_logp_dev", grad_logp_dev) || sf_eval_aligned4(who, "grad_entropy_dev", grad_entropy_dev))
    return SF_ERR_ARG;
  const dim3 grid(sf_eval_blocks(n_rows)), block(256);
  hipStream_t s = (hipStream_t)stream;
  SF_EVAL_DISPATCH(sf_eval_bwd_kernel, logits_dev, n_rows, n_actions, row_stride, actions_dev, act_type, grad_logp_dev, grad_entropy_dev,
                   grad_logits_out_dev, grad_row_stride);
  return sf_eval_launched(who);
}

extern "C" size_t sf_ppo_loss_workspace_bytes(int n_rows) {
  return n_rows > 0 ? (size_t)sf_eval_blocks(n_rows) * 3 * sizeof(double) : 0;
}

extern "C" int sf_ppo_loss(const float* logits_dev, const float* values_dev, const void* actions_dev, const float* old_logp_dev,
                           const float* adv_dev, const float* returns_dev, int n_rows, int n_actions, size_t row_stride, int act_type,
                           float clip_lo, float clip_hi, float value_coef, float entropy_coef, float* row_terms_out_dev,
                           float* sums_out_dev, void* workspace_dev, uint64_t* bad_rows_dev, void* stream) {
  const char* who = "sf_ppo_loss";
  if (sf_eval_args(who, logits_dev, n_rows, n_actions, row_stride, actions_dev, act_type)) return SF_ERR_ARG;
  if (sf_ppo_args(who, values_dev, old_logp_dev, adv_dev, returns_dev)) return SF_ERR_ARG;
  if (!sums_out_dev) {
    sf_set_error("%s: sums_out_dev must not be null", who);
    return SF_ERR_ARG;
  }
  if (sf_eval_aligned4(who, "sums_out_dev", sums_out_dev) || sf_eval_aligned4(who, "row_terms_out_dev", row_terms_out_dev))
    return SF_ERR_ARG;
  if (!workspace_dev || ((uintptr_t)workspace_dev & 7) != 0) {
    sf_set_error("%s: workspace_dev must be %zu bytes (sf_ppo_loss_workspace_bytes), 8-byte aligned, not null", who,
                 sf_ppo_loss_workspace_bytes(n_rows));
    return SF_ERR_ARG;
  }
  const dim3 grid(sf_eval_blocks(n_rows)), block(256);
  hipStream_t s = (hipStream_t)stream;
  unsigned long long* const bad = reinterpret_cast<unsigned long long*>(bad_rows_dev);
  double* const partials = reinterpret_cast<double*>(workspace_dev);
  SF_EVAL_DISPATCH(sf_ppo_loss_kernel, logits_dev, values_dev, actions_dev, old_logp_dev, adv_dev, returns_dev, n_rows, n_actions,
                   row_stride, act_type, clip_lo, clip_hi, row_terms_out_dev, partials, bad);
  hipLaunchKernelGGL(sf_ppo_finish_kernel, dim3(1), block, 0, s, partials, (int)grid.x, n_rows, value_coef, entropy_coef, sums_out_dev);
  return sf_eval_launched(who);
}

extern "C" int sf_ppo_loss_backward(const float* logits_dev, const float* values_dev, const void* actions_dev, const float* old_logp_dev,
                                    const float* adv_dev, const float* returns_dev, int n_rows, int n_actions, size_t row_stride,
                                    int act_type, float clip_lo, float clip_hi, float value_coef, float entropy_coef,
                                    const float* grad_loss_dev, float* grad_logits_out_dev, size_t grad_row_stride,
                                    float* grad_values_out_dev, void* stream) {
  const char* who = "sf_ppo_loss_backward";
  if (sf_eval_args(who, logits_dev, n_rows, n_actions, row_stride, actions_dev, act_type)) return SF_ERR_ARG;
  if (sf_ppo_args(who, values_dev, old_logp_dev, adv_dev, returns_dev)) return SF_ERR_ARG;
  if (!grad_loss_dev) {
    sf_set_error("%s: grad_loss_dev must not be null", who);
    return SF_ERR_ARG;
  }
  if (sf_eval_grad_args(who, grad_logits_out_dev, grad_row_stride, n_actions)) return SF_ERR_ARG;
  if (sf_eval_aligned4(who, "grad_loss_dev", grad_loss_dev) || sf_eval_aligned4(who, "grad_values_out_dev", grad_values_out_dev))
    return SF_ERR_ARG;
  const dim3 grid(sf_eval_blocks(n_rows)), block(256);
  hipStream_t s = (hipStream_t)stream;
  SF_EVAL_DISPATCH(sf_ppo_loss_bwd_kernel, logits_dev, values_dev, actions_dev, old_logp_dev, adv_dev, returns_dev, n_rows, n_actions,
                   row_stride, act_type, clip_lo, clip_hi, value_coef, entropy_coef, grad_loss_dev, grad_logits_out_dev, grad_row_stride,
                   grad_values_out_dev);
  return sf_eval_launched(who);
}
