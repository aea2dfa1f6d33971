// sf_optim.hip -- the end of a PPO update (include/sfmi_optim.h): clip_grad_norm_ and one Adam step over a table of float32
// tensors, three launches, the step's bookkeeping in a state block on the device.
//
//   sf_adam_sumsq_kernel    a block per chunk of SF_OPT_CHUNK elements of one tensor: each lane adds the exact float64 squares
//                           of its up to eight grads in index order, then sf_fixed_sum.h's tree and waves; one partial sum per
//                           chunk.
//   sf_adam_finish_kernel   one block: the chunks' partial sums in index order, the norm and coef; where the sum is finite it
//                           advances t and the running products and leaves the step's float32 scalars in the state block, else
//                           it counts a skipped step.
//   sf_adam_update_kernel   a block per chunk again: reads the scalars, leaves at once where the step is skipped, else the
//                           element update -- 28 bytes moved per element, 16 per lane and access where the tensor allows it.
//   sf_adam_init_kernel     one thread: the state block of sf_adam_state_init.
//
// The table of tensors travels in the kernels' arguments (SfOptTable, 2.8 KB at SF_OPT_MAX_TENSORS = 64; the limit is 4 KB): a
// block finds its tensor by walking the table's chunk starts, which are wave-uniform scalar loads.
// Plain global loads and stores only.  Compiled with -ffp-contract=off like the rest.
#include <hip/hip_runtime.h>

#include "sf_fixed_sum.h"
#include "sf_internal.h"
#include "sfmi_optim.h"

namespace {

#define SF_OPT_PASSES (SF_OPT_CHUNK / (SF_SUM_BLOCK * 4))  // groups of four elements per lane and chunk

static_assert(SF_OPT_CHUNK % (SF_SUM_BLOCK * 4) == 0, "a chunk is a whole number of passes of four elements per lane");

struct SfOptTable {
  float* param[SF_OPT_MAX_TENSORS];
  const float* grad[SF_OPT_MAX_TENSORS];
  float* exp_avg[SF_OPT_MAX_TENSORS];
  float* exp_avg_sq[SF_OPT_MAX_TENSORS];
  long long numel[SF_OPT_MAX_TENSORS];
  unsigned chunk_start[SF_OPT_MAX_TENSORS + 1];  // tensor k owns the chunks [chunk_start[k], chunk_start[k + 1])
  int n;
};

static_assert(sizeof(SfOptTable) + 64 <= 4096, "the table and the other arguments must fit the kernel-argument segment");

struct SfAdamState {  // sfmi_optim.h: THE STATE BLOCK
  long long t;
  double beta1_pow, beta2_pow;
  double lr, beta1, beta2, eps;
  double norm, coef;
  unsigned long long skipped;
  float f_coef, f_b1, f_omb1, f_b2, f_omb2, f_sqrt_bc2, f_eps, f_step_size;
  unsigned apply;
  unsigned pad[3];
};

static_assert(sizeof(SfAdamState) == SF_ADAM_STATE_BYTES, "the state block's layout is part of the interface");

// the tensor that owns chunk `b` (wave-uniform: b is blockIdx.x)
__device__ __forceinline__ int sf_opt_find(const SfOptTable& T, unsigned b) {
  int k = 0;
  while (k + 1 < T.n && b >= T.chunk_start[k + 1]) k++;
  return k;
}

__device__ __forceinline__ bool sf_opt_aligned16(const void* a, const void* b, const void* c, const void* d) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
           reinterpret_cast<uintptr_t>(d)) & 15u) == 0;
}

__global__ __launch_bounds__(SF_SUM_BLOCK) void sf_adam_sumsq_kernel(SfOptTable T, double* __restrict__ partials) {
  __shared__ double part[4][1];
  const int k = sf_opt_find(T, blockIdx.x);
  const float* __restrict__ const grad = T.grad[k];
  const long long numel = T.numel[k];
  const long long off = (long long)(blockIdx.x - T.chunk_start[k]) * SF_OPT_CHUNK;
  const bool wide = sf_opt_aligned16(T.param[k], grad, T.exp_avg[k], T.exp_avg_sq[k]);
  double acc = 0.0;
#pragma unroll
  for (int pass = 0; pass < SF_OPT_PASSES; pass++) {
    const long long i = off + pass * (SF_SUM_BLOCK * 4) + 4 * (int)threadIdx.x;
    const long long left = numel - i;
    float g[4] = {0.0f, 0.0f, 0.0f, 0.0f};  // (beyond the tensor's end: +0.0, whose square adds nothing)
    if (wide && left >= 4) {
      const float4 v = *reinterpret_cast<const float4*>(grad + i);
      g[0] = v.x, g[1] = v.y, g[2] = v.z, g[3] = v.w;
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++)
        if (j < left) g[j] = grad[i + j];
    }
#pragma unroll
    for (int j = 0; j < 4; j++) acc = acc + (double)g[j] * (double)g[j];
  }
  double v[1] = {acc};
  sf_block_partials<1>(v, part, partials);  // (every lane of the block is here: nobody left above)
}

__global__ __launch_bounds__(SF_SUM_BLOCK) void sf_adam_finish_kernel(const double* __restrict__ partials, int n_chunks,
                                                                      double max_grad_norm, SfAdamState* __restrict__ st,
                                                                      unsigned long long* errors) {
  __shared__ double buf[SF_SUM_CHUNK];
  const double S = sf_blocks_in_order<1>(partials, n_chunks, buf);
  if (threadIdx.x != 0) return;
  const double norm = sqrt(S);
  st->norm = norm;
  if (!(S - S == 0.0)) {  // an inf or a NaN: the step is skipped
    st->coef = 0.0;
    st->apply = 0u;
    st->skipped = st->skipped + 1ull;
    if (errors) atomicAdd(errors, 1ull);
    return;
  }
  double coef = 1.0;
  if (max_grad_norm > 0.0) {
    coef = max_grad_norm / (norm + 1e-6);
    if (coef > 1.0) coef = 1.0;
  }
  const double b1 = st->beta1, b2 = st->beta2;
  const double p1 = st->beta1_pow * b1, p2 = st->beta2_pow * b2;
  st->t = st->t + 1;
  st->beta1_pow = p1;
  st->beta2_pow = p2;
  const double bc1 = 1.0 - p1, bc2 = 1.0 - p2;
  st->coef = coef;
  st->f_coef = (float)coef;
  st->f_b1 = (float)b1;
  st->f_omb1 = (float)(1.0 - b1);
  st->f_b2 = (float)b2;
  st->f_omb2 = (float)(1.0 - b2);
  st->f_sqrt_bc2 = (float)sqrt(bc2);
  st->f_eps = (float)st->eps;
  st->f_step_size = (float)(st->lr / bc1);
  st->apply = 1u;
}

struct SfAdamScalars {
  float coef, b1, omb1, b2, omb2, sqrt_bc2, eps, step_size;
};

__device__ __forceinline__ void sf_adam_element(const SfAdamScalars& c, float grad, float& p, float& m, float& v) {
  const float g = grad * c.coef;
  m = c.b1 * m + c.omb1 * g;
  v = c.b2 * v + (c.omb2 * g) * g;
  const float d = sqrtf(v) / c.sqrt_bc2 + c.eps;
  p = p - c.step_size * (m / d);
}

__global__ __launch_bounds__(SF_SUM_BLOCK) void sf_adam_update_kernel(SfOptTable T, const SfAdamState* __restrict__ st) {
  if (st->apply == 0u) return;  // (wave-uniform: a skipped step touches nothing)
  const SfAdamScalars c = {st->f_coef, st->f_b1, st->f_omb1, st->f_b2, st->f_omb2, st->f_sqrt_bc2, st->f_eps, st->f_step_size};
  const int k = sf_opt_find(T, blockIdx.x);
  float* const param = T.param[k];
  const float* const grad = T.grad[k];
  float* const ea = T.exp_avg[k];
  float* const es = T.exp_avg_sq[k];
  const long long numel = T.numel[k];
  const long long off = (long long)(blockIdx.x - T.chunk_start[k]) * SF_OPT_CHUNK;
  const bool wide = sf_opt_aligned16(param, grad, ea, es);
#pragma unroll
  for (int pass = 0; pass < SF_OPT_PASSES; pass++) {
    const long long i = off + pass * (SF_SUM_BLOCK * 4) + 4 * (int)threadIdx.x;
    const long long left = numel - i;
    if (wide && left >= 4) {
      const float4 g = *reinterpret_cast<const float4*>(grad + i);
      float4 p = *reinterpret_cast<const float4*>(param + i);
      float4 m = *reinterpret_cast<const float4*>(ea + i);
      float4 v = *reinterpret_cast<const float4*>(es + i);
      sf_adam_element(c, g.x, p.x, m.x, v.x);
      sf_adam_element(c, g.y, p.y, m.y, v.y);
      sf_adam_element(c, g.z, p.z, m.z, v.z);
      sf_adam_element(c, g.w, p.w, m.w, v.w);
      *reinterpret_cast<float4*>(ea + i) = m;
      *reinterpret_cast<float4*>(es + i) = v;
      *reinterpret_cast<float4*>(param + i) = p;
    } else {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        if (j < left) {
          float p = param[i + j], m = ea[i + j], v = es[i + j];
          sf_adam_element(c, grad[i + j], p, m, v);
          ea[i + j] = m;
          es[i + j] = v;
          param[i + j] = p;
        }
      }
    }
  }
}

__global__ void sf_adam_init_kernel(SfAdamState* st, double lr, double beta1, double beta2, double eps) {
  SfAdamState s = {};
  s.beta1_pow = 1.0;
  s.beta2_pow = 1.0;
  s.lr = lr;
  s.beta1 = beta1;
  s.beta2 = beta2;
  s.eps = eps;
  *st = s;
}

int sf_opt_launched(const char* who) {
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) {
    sf_set_error("%s: %s", who, hipGetErrorString(err));
    return SF_ERR_HIP;
  }
  return SF_OK;
}

inline bool sf_opt_misaligned(const void* p, unsigned a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) != 0; }

}  // namespace

extern "C" int64_t sf_adam_chunks(int64_t numel) { return numel > 0 ? (numel - 1) / SF_OPT_CHUNK + 1 : 0; }

extern "C" size_t sf_adam_workspace_bytes(int64_t total_chunks) { return total_chunks > 0 ? (size_t)total_chunks * sizeof(double) : 0; }

extern "C" size_t sf_adam_state_bytes(void) { return SF_ADAM_STATE_BYTES; }

extern "C" int sf_adam_state_init(void* state_dev, double lr, double beta1, double beta2, double eps, void* stream) {
  const char* who = "sf_adam_state_init";
  if (!state_dev || sf_opt_misaligned(state_dev, 16)) {
    sf_set_error("%s: state_dev must be %d bytes, 16-byte aligned, not null", who, SF_ADAM_STATE_BYTES);
    return SF_ERR_ARG;
  }
  if (!(lr >= 0.0 && lr - lr == 0.0) || !(eps >= 0.0 && eps - eps == 0.0) || !(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) {
    sf_set_error("%s: need finite lr >= 0 and eps >= 0 and both betas in [0, 1) (got lr %g, betas %g %g, eps %g)", who, lr, beta1, beta2,
                 eps);
    return SF_ERR_ARG;
  }
  hipLaunchKernelGGL(sf_adam_init_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, reinterpret_cast<SfAdamState*>(state_dev), lr, beta1,
                     beta2, eps);
  return sf_opt_launched(who);
}

extern "C" int sf_adam_step(const sf_opt_tensor* tensors, int n_tensors, double max_grad_norm, void* state_dev, void* workspace_dev,
                            uint64_t* errors_dev, void* stream) {
  const char* who = "sf_adam_step";
  if (!tensors) {
    sf_set_error("%s: tensors must not be null", who);
    return SF_ERR_ARG;
  }
  if (n_tensors < 1 || n_tensors > SF_OPT_MAX_TENSORS) {
    sf_set_error("%s: n_tensors %d outside [1, %d]", who, n_tensors, SF_OPT_MAX_TENSORS);
    return SF_ERR_ARG;
  }
  if (!state_dev || sf_opt_misaligned(state_dev, 16)) {
    sf_set_error("%s: state_dev must be %d bytes (sf_adam_state_init), 16-byte aligned, not null", who, SF_ADAM_STATE_BYTES);
    return SF_ERR_ARG;
  }
  if (!workspace_dev || sf_opt_misaligned(workspace_dev, 8)) {
    sf_set_error("%s: workspace_dev must be sf_adam_workspace_bytes(total chunks) bytes, 8-byte aligned, not null", who);
    return SF_ERR_ARG;
  }
  if (sf_opt_misaligned(errors_dev, 8)) {
    sf_set_error("%s: errors_dev must be 8-byte aligned", who);
    return SF_ERR_ARG;
  }
  SfOptTable T = {};
  T.n = n_tensors;
  int64_t chunks = 0;
  for (int k = 0; k < n_tensors; k++) {
    const sf_opt_tensor& t = tensors[k];
    if (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq || sf_opt_misaligned(t.param, 4) || sf_opt_misaligned(t.grad, 4) ||
        sf_opt_misaligned(t.exp_avg, 4) || sf_opt_misaligned(t.exp_avg_sq, 4)) {
      sf_set_error("%s: tensor %d: param, grad, exp_avg and exp_avg_sq must be 4-byte aligned, not null", who, k);
      return SF_ERR_ARG;
    }
    if (t.numel <= 0) {
      sf_set_error("%s: tensor %d: numel %lld: need at least one element", who, k, (long long)t.numel);
      return SF_ERR_ARG;
    }
    T.param[k] = t.param;
    T.grad[k] = t.grad;
    T.exp_avg[k] = t.exp_avg;
    T.exp_avg_sq[k] = t.exp_avg_sq;
    T.numel[k] = (long long)t.numel;
    T.chunk_start[k] = (unsigned)chunks;
    chunks += sf_adam_chunks(t.numel);
    if (chunks > SF_OPT_MAX_CHUNKS) {
      sf_set_error("%s: more than %d chunks of %d elements in all", who, SF_OPT_MAX_CHUNKS, SF_OPT_CHUNK);
      return SF_ERR_ARG;
    }
  }
  for (int k = n_tensors; k <= SF_OPT_MAX_TENSORS; k++) T.chunk_start[k] = (unsigned)chunks;
  const dim3 grid((unsigned)chunks), block(SF_SUM_BLOCK);
  hipStream_t s = (hipStream_t)stream;
  SfAdamState* const st = reinterpret_cast<SfAdamState*>(state_dev);
  double* const partials = reinterpret_cast<double*>(workspace_dev);
  hipLaunchKernelGGL(sf_adam_sumsq_kernel, grid, block, 0, s, T, partials);
  hipLaunchKernelGGL(sf_adam_finish_kernel, dim3(1), block, 0, s, (const double*)partials, (int)chunks, max_grad_norm, st,
                     reinterpret_cast<unsigned long long*>(errors_dev));
  hipLaunchKernelGGL(sf_adam_update_kernel, grid, block, 0, s, T, (const SfAdamState*)st);
  return sf_opt_launched(who);
}
