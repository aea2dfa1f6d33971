// sf_frame_store.hip -- the image rollout storage that keeps every 84x84 frame ONCE and assembles the trainer's
// frame stacks when they are read (rl/train.py:38-41,51-56,92-97; the sampling of rl/storage.py:66-122).
//
// A frame store holds, per env, `rows` = (S - 1) + T + 1 frames of 7 056 bytes -- S - 1 rows of history in front of the
// rollout's T + 1 -- and one START flag byte per stored frame (1: this frame is the first observation of a new game).
// Store row r holds the frame of step r - (S - 1).  The stack of (t, e) as the trainer builds it (`current_obs *= masks`,
// shift by a frame, new frame last) is a pure function of the store:
//
//     slot j of stack(t, e) = row t + j of env e    if none of the rows t + j + 1 .. t + S - 1 of env e carries a start flag
//                           = 0                      otherwise                       (slot S - 1 is always row t + S - 1)
//
//   sf_gather_kernel   one workgroup of 256 lanes per sample.  The S - 1 flag bytes are read once per sample (uniform across
//                      the workgroup) into a mask of live slots; then every lane moves pieces of 16 OUTPUT bytes: it loads
//                      16 / 8 / 4 frame bytes (uint8 / float16 / float32 output), converts, and stores one dwordx4 --
//                      consecutive lanes at consecutive addresses on both sides (a slot is 441 / 882 / 1 764 pieces).  Zeroed
//                      slots are stored without loading.  Plain global loads and stores, no LDS.  An index outside
//                      [0, T * n_envs) is range-checked BEFORE any address is formed: a zero stack, counted on the device.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include "sf_internal.h"

namespace {

constexpr int kFrameBytes = SF_IMAGE_OUT * SF_IMAGE_OUT;  // 7 056 = 441 * 16
static_assert(kFrameBytes % 16 == 0, "a frame is a whole number of 16-byte pieces");

__device__ unsigned long long sf_gather_bad_indices;  // sticky count of out-of-range indices (sf_gather_errors)

struct SfGatherArgs {
  const uint8_t* frames;
  const uint8_t* start;   // [rows][n_envs]
  int64_t env_stride;     // bytes from one env's frame to the next env's, same row
  int64_t row_stride;     // bytes from one row to the next, same env
  const void* index;      // n_samples flat transition indices t * n_envs + e, or NULL: the n_envs stacks of step `step`
  int64_t n_transitions;  // T * n_envs
  int64_t step;
  void* out;
  int n_envs, num_stack, idx64;
};

// PIX = frame bytes behind one 16-byte piece of output
template <typename In, int PIX> struct Convert;
template <> struct Convert<uint4, 16> {
  static __device__ __forceinline__ uint4 to(uint4 v) { return v; }
};
template <> struct Convert<uint2, 8> {  // 8 bytes -> 8 float16 (exact for 0 .. 255)
  static __device__ __forceinline__ uint4 to(uint2 v) {
    union { __half2 h[4]; uint4 u; } r;
    r.h[0] = __halves2half2(__ushort2half_rn(v.x & 255u), __ushort2half_rn((v.x >> 8) & 255u));
    r.h[1] = __halves2half2(__ushort2half_rn((v.x >> 16) & 255u), __ushort2half_rn(v.x >> 24));
    r.h[2] = __halves2half2(__ushort2half_rn(v.y & 255u), __ushort2half_rn((v.y >> 8) & 255u));
    r.h[3] = __halves2half2(__ushort2half_rn((v.y >> 16) & 255u), __ushort2half_rn(v.y >> 24));
    return r.u;
  }
};
template <> struct Convert<uint32_t, 4> {  // 4 bytes -> 4 float32
  static __device__ __forceinline__ uint4 to(uint32_t v) {
    union { float f[4]; uint4 u; } r;
    r.f[0] = (float)(v & 255u);
    r.f[1] = (float)((v >> 8) & 255u);
    r.f[2] = (float)((v >> 16) & 255u);
    r.f[3] = (float)(v >> 24);
    return r.u;
  }
};

template <typename In, int PIX>
__global__ __launch_bounds__(256) void sf_gather_kernel(SfGatherArgs a) {
  constexpr int kPieces = kFrameBytes / PIX;  // per slot
  const int64_t sample = blockIdx.x;
  const int S = a.num_stack;
  int64_t t, e;
  bool ok = true;
  if (a.index) {
    const int64_t idx = a.idx64 ? reinterpret_cast<const int64_t*>(a.index)[sample]
                                : (int64_t) reinterpret_cast<const int32_t*>(a.index)[sample];
    ok = idx >= 0 && idx < a.n_transitions;  // (uniform across the workgroup)
    t = ok ? idx / a.n_envs : 0;
    e = ok ? idx - t * a.n_envs : 0;
  } else {
    t = a.step;  // (checked on the host)
    e = sample;
  }
  // live slots: bit j set = slot j is a frame, clear = zeros
  unsigned live = 0;
  if (ok) {
    live = 1u << (S - 1);
    for (int j = S - 2; j >= 0; j--) {
      if (a.start[(t + j + 1) * a.n_envs + e]) break;
      live |= 1u << j;
    }
  } else if (threadIdx.x == 0) {
    atomicAdd(&sf_gather_bad_indices, 1ull);
  }
  const uint8_t* __restrict__ src = a.frames + e * a.env_stride + t * a.row_stride;
  uint4* __restrict__ dst = reinterpret_cast<uint4*>(a.out) + sample * ((int64_t)S * kPieces);
  const int total = S * kPieces;
#pragma unroll 4
  for (int p = threadIdx.x; p < total; p += 256) {
    const int j = p / kPieces, i = p - j * kPieces;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if ((live >> j) & 1u) v = Convert<In, PIX>::to(reinterpret_cast<const In*>(src + (int64_t)j * a.row_stride)[i]);
    dst[p] = v;
  }
}

}  // namespace

extern "C" int sf_gather_stacks(const uint8_t* frames_dev, const uint8_t* start_dev, int n_envs, int rows, int num_stack,
                                int64_t env_stride, int64_t row_stride, const void* index_dev, int idx_type, int64_t n_samples,
                                int64_t step, void* out_dev, int out_type, void* stream) {
  if (!frames_dev || !start_dev || n_envs <= 0 || num_stack < 1 || num_stack > 16 || rows < num_stack) {
    sf_set_error("sf_gather_stacks: need a store, its start flags, n_envs > 0, 1 <= num_stack <= 16 and rows >= num_stack");
    return SF_ERR_ARG;
  }
  // the two layouts a store can have, and nothing that would make frames overlap
  const bool env_major = row_stride >= kFrameBytes && env_stride >= (int64_t)rows * row_stride;
  const bool time_major = env_stride >= kFrameBytes && row_stride >= (int64_t)n_envs * env_stride;
  if (((uintptr_t)frames_dev & 15) != 0 || ((env_stride | row_stride) & 15) != 0 || !(env_major || time_major)) {
    sf_set_error("sf_gather_stacks: frames 16-byte aligned, strides multiples of 16 that keep the frames apart "
                 "(env-major [n][rows][7056] or time-major [rows][n][7056])");
    return SF_ERR_ARG;
  }
  const int64_t T = rows - num_stack;  // rows = (num_stack - 1) + T + 1
  if (index_dev) {
    if (idx_type != SF_ACT_I32 && idx_type != SF_ACT_I64) {
      sf_set_error("sf_gather_stacks: idx_type must be 4 or 8 (got %d)", idx_type);
      return SF_ERR_ARG;
    }
  } else if (n_samples != n_envs || step < 0 || step > T) {
    sf_set_error("sf_gather_stacks: without indices, n_samples = n_envs and 0 <= step <= %lld", (long long)T);
    return SF_ERR_ARG;
  }
  if (n_samples < 0 || n_samples > 0x7fffffffLL) {
    sf_set_error("sf_gather_stacks: 0 <= n_samples < 2^31");
    return SF_ERR_ARG;
  }
  if (out_type != SF_STACK_U8 && out_type != SF_STACK_F16 && out_type != SF_STACK_F32) {
    sf_set_error("sf_gather_stacks: out_type must be SF_STACK_U8, SF_STACK_F16 or SF_STACK_F32 (got %d)", out_type);
    return SF_ERR_ARG;
  }
  if (n_samples == 0) return SF_OK;
  if (!out_dev || ((uintptr_t)out_dev & 15) != 0) {
    sf_set_error("sf_gather_stacks: out_dev must be 16-byte aligned");
    return SF_ERR_ARG;
  }
  SfGatherArgs a{frames_dev, start_dev, env_stride, row_stride, index_dev, T * n_envs, step, out_dev, n_envs, num_stack,
                 idx_type == SF_ACT_I64 ? 1 : 0};
  const dim3 grid((unsigned)n_samples), block(256);
  if (out_type == SF_STACK_U8)
    hipLaunchKernelGGL((sf_gather_kernel<uint4, 16>), grid, block, 0, (hipStream_t)stream, a);
  else if (out_type == SF_STACK_F16)
    hipLaunchKernelGGL((sf_gather_kernel<uint2, 8>), grid, block, 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL((sf_gather_kernel<uint32_t, 4>), grid, block, 0, (hipStream_t)stream, a);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) {
    sf_set_error("sf_gather_stacks: %s", hipGetErrorString(err));
    return SF_ERR_HIP;
  }
  return SF_OK;
}

extern "C" int sf_gather_errors(uint64_t* count_out, int clear, void* stream) {
  unsigned long long c = 0;
  hipError_t err = hipStreamSynchronize((hipStream_t)stream);
  if (err == hipSuccess) err = hipMemcpyFromSymbol(&c, HIP_SYMBOL(sf_gather_bad_indices), sizeof(c));
  if (err == hipSuccess && clear && c) {
    const unsigned long long zero = 0;
    err = hipMemcpyToSymbol(HIP_SYMBOL(sf_gather_bad_indices), &zero, sizeof(zero));
  }
  if (err != hipSuccess) {
    sf_set_error("sf_gather_errors: %s", hipGetErrorString(err));
    return SF_ERR_HIP;
  }
  if (count_out) *count_out = c;
  if (c) {
    sf_set_error("sf_gather_stacks: %llu indices outside the rollout's transitions (their stacks are zero)", c);
    return SF_ERR_ACTION;
  }
  return SF_OK;
}
