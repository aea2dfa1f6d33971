// sf_policy.hip -- the policy head (include/sfmi_policy.h): what the reference's trainer does between the network and the env
// (rl/networks.py:65-76: softmax, log_softmax, multinomial(1) or max(1)[1], gather), as ONE launch over the [N, A] logits.
//
//   sf_policy_kernel<AMAX>   one lane per env.  The lane holds its row in registers (AMAX = 4, 8, 16 or 32 of them, the loops
//                            unrolled to AMAX and cut at A by a wave-uniform compare), takes the maximum, the float32
//                            exponentials with their float64 running sum, draws one Philox4x32-10 word on
//                            (first_lane + i, tick, 0x504F4C, 0), walks the running sum again for the action, and writes the
//                            action, its log-probability and the row's entropy.  The tick is one word per wave, read by every
//                            lane and stored back + 1 by the wave's first lane: waves do not depend on each other.
//
// The working set is tiny (65 536 x 5 floats = 1.3 MB) and the launch is latency-bound: a lane reads its row directly -- the
// wave's 64 * A floats are contiguous for a dense batch, so the A loads of a wave touch the same 5 to 32 cache lines -- and
// there is no barrier and no LDS in the pass.
// The arithmetic is the header's, operation by operation, compiled with -ffp-contract=off: tests/policyref.py restates it.
#include <hip/hip_runtime.h>

#include "sf_internal.h"
#include "sfmi_policy.h"

namespace {

// Philox4x32-10 on all four counter words (sf_kernels.hip has the two-word form of the step's sampler); word 0 of the output
__device__ __forceinline__ unsigned sf_policy_philox(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const unsigned lo0 = 0xD2511F53u * c0, hi0 = __umulhi(0xD2511F53u, c0);
    const unsigned lo1 = 0xCD9E8D57u * c2, hi1 = __umulhi(0xCD9E8D57u, c2);
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c0;
}

template <int AMAX>
__global__ __launch_bounds__(256) void sf_policy_kernel(const float* __restrict__ logits, int n, int A, size_t row_stride, int mode,
                                                        unsigned k0, unsigned k1, unsigned first_lane, uint32_t* ticks,
                                                        void* actions_out, int act_type, float* logp_out, float* entropy_out,
                                                        unsigned long long* bad_rows) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;  // (whole waves beyond n leave here: ticks has ceil(n / 64) words)
  const float* row = logits + (size_t)i * row_stride;
  const float inf = __builtin_inff();
  float x[AMAX];
#pragma unroll
  for (int k = 0; k < AMAX; k++) x[k] = k < A ? row[k] : -inf;
  unsigned tick = 0u;
  if (mode == SF_POLICY_SAMPLE) {
    uint32_t* tp = ticks + (i >> 6);
    tick = *tp;
    if ((i & 63) == 0) *tp = tick + 1u;  // (after the wave's reads: the value stored depends on the one loaded)
  }
  // 1. the maximum and its first index; a NaN or a +inf makes the row bad, and so does a maximum of -inf
  float m = -inf;
  int first = 0;
  bool bad = false;
#pragma unroll
  for (int k = 0; k < AMAX; k++) {
    if (k < A) {
      bad = bad || !(x[k] < inf);
      if (x[k] > m) {
        m = x[k];
        first = k;
      }
    }
  }
  bad = bad || m == -inf;
  if (bad) m = 0.0f;  // (the arithmetic below stays defined; its results are not used)
  // 2., 3. e[k] in float32, their running sum in float64, the entropy's sum in float32
  float e[AMAX];
  double S = 0.0;
  float dot = 0.0f;
#pragma unroll
  for (int k = 0; k < AMAX; k++) {
    e[k] = 0.0f;
    if (k < A) {
      const float d = x[k] - m;
      e[k] = bad ? 0.0f : expf(d);
      S = S + (double)e[k];
      if (e[k] != 0.0f) dot = dot + e[k] * d;
    }
  }
  int a = first;
  if (mode == SF_POLICY_SAMPLE) {
    const unsigned w = sf_policy_philox(first_lane + (unsigned)i, tick, SF_POLICY_COUNTER_WORD, 0u, k0, k1);
    const double t = (((double)w + 0.5) * 0x1p-32) * S;
    double c = 0.0;
    a = 0;
#pragma unroll
    for (int k = 0; k < AMAX; k++) {
      if (k < A) {
        c = c + (double)e[k];
        a += c <= t ? 1 : 0;  // (c is non-decreasing: the smallest k with t < c[k] is the number of k with c[k] <= t)
      }
    }
    a = a < A ? a : A - 1;  // (t < S = c[A-1] on every good row; a bad row is overruled below)
  }
  float xa = x[0];
#pragma unroll
  for (int k = 1; k < AMAX; k++) xa = k == a ? x[k] : xa;
  const float Sf = (float)S;
  const float lse = logf(Sf);
  float logp = (xa - m) - lse;
  float ent = lse - dot / Sf;
  if (bad) {
    a = 0;
    logp = ent = __builtin_nanf("");
  }
  if (act_type == SF_ACT_U8)
    reinterpret_cast<uint8_t*>(actions_out)[i] = (uint8_t)a;
  else if (act_type == SF_ACT_I32)
    reinterpret_cast<int32_t*>(actions_out)[i] = a;
  else
    reinterpret_cast<int64_t*>(actions_out)[i] = (int64_t)a;
  if (logp_out) logp_out[i] = logp;
  if (entropy_out) entropy_out[i] = ent;
  if (bad_rows) {  // one atomic per wave that saw a bad row
    const unsigned long long votes = __ballot(bad);
    if (bad && (unsigned)__lane_id() == (unsigned)__builtin_ctzll(votes)) atomicAdd(bad_rows, (unsigned long long)__popcll(votes));
  }
}

}  // namespace

extern "C" int sf_policy_sample(const float* logits_dev, int n_envs, int n_actions, size_t row_stride, int mode, uint64_t seed,
                                uint32_t first_lane, uint32_t* ticks_dev, void* actions_out_dev, int act_type, float* logp_out_dev,
                                float* entropy_out_dev, uint64_t* bad_rows_dev, void* stream) {
  if (!logits_dev || !actions_out_dev) {
    sf_set_error("sf_policy_sample: logits_dev and actions_out_dev must not be null");
    return SF_ERR_ARG;
  }
  if (n_envs <= 0) {
    sf_set_error("sf_policy_sample: n_envs %d: need at least one env", n_envs);
    return SF_ERR_ARG;
  }
  if (n_actions < 1 || n_actions > SF_POLICY_MAX_ACTIONS) {
    sf_set_error("sf_policy_sample: n_actions %d outside [1, %d]", n_actions, SF_POLICY_MAX_ACTIONS);
    return SF_ERR_ARG;
  }
  if (row_stride < (size_t)n_actions) {
    sf_set_error("sf_policy_sample: row_stride %zu below n_actions %d", row_stride, n_actions);
    return SF_ERR_ARG;
  }
  if (mode != SF_POLICY_SAMPLE && mode != SF_POLICY_ARGMAX) {
    sf_set_error("sf_policy_sample: mode %d (0: sample, 1: argmax)", mode);
    return SF_ERR_ARG;
  }
  if (act_type != SF_ACT_U8 && act_type != SF_ACT_I32 && act_type != SF_ACT_I64) {
    sf_set_error("sf_policy_sample: act_type %d (1, 4 or 8: the bytes of an action)", act_type);
    return SF_ERR_ARG;
  }
  if (mode == SF_POLICY_SAMPLE && !ticks_dev) {
    sf_set_error("sf_policy_sample: sampling needs ticks_dev (uint32 [ceil(n_envs / 64)], zeroed to start a stream)");
    return SF_ERR_ARG;
  }
  if (((uintptr_t)logits_dev & 3) != 0) {
    sf_set_error("sf_policy_sample: logits_dev must be 4-byte aligned");
    return SF_ERR_ARG;
  }
  const dim3 grid((unsigned)((n_envs + 255) / 256)), block(256);
  const unsigned k0 = (unsigned)(seed & 0xFFFFFFFFull), k1 = (unsigned)(seed >> 32);
  unsigned long long* const bad = reinterpret_cast<unsigned long long*>(bad_rows_dev);
  hipStream_t s = (hipStream_t)stream;
#define SF_POLICY_LAUNCH(AMAX)                                                                                                   \
  hipLaunchKernelGGL(sf_policy_kernel<AMAX>, grid, block, 0, s, logits_dev, n_envs, n_actions, row_stride, mode, k0, k1, first_lane, \
                     ticks_dev, actions_out_dev, act_type, logp_out_dev, entropy_out_dev, bad)
  if (n_actions <= 4)
    SF_POLICY_LAUNCH(4);
  else if (n_actions <= 8)
    SF_POLICY_LAUNCH(8);
  else if (n_actions <= 16)
    SF_POLICY_LAUNCH(16);
  else
    SF_POLICY_LAUNCH(32);
#undef SF_POLICY_LAUNCH
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) {
    sf_set_error("sf_policy_sample: %s", hipGetErrorString(err));
    return SF_ERR_HIP;
  }
  return SF_OK;
}
