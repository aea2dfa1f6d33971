// sf_final_frames.hip -- the device side of include/sfmi_final.h, off the hot path: the finished envs' last frames, and the
// history of a final stack.
//
// sf_final_frames_kernel: one workgroup per env, which returns at once when the env's done byte is zero -- on all but one tick
// in 5 295 per env.  A finished env's frame is painted from its STATE, which the step launch in front (auto-reset argument
// off) left as the finished game's, by the general renderer's own code (sf_generic_frame_dev.h: sfs::ScenePainter<false>, then
// the surface or its 84 x 84 INTER_AREA image) in the batch's geometry -- the default one included, with the default
// geometry's hexagons, INTER_AREA taps and glyph atlas in the general renderer's table forms (sf_final_capi.cpp).  It reads the
// state only: no picture cache, no explosion cache, no hint word, no draw record is read or written, so the ordinary frames
// behind it are what they would have been.
//
// sf_final_stack_shift_kernel: for the envs whose done byte is set, slots 1 .. S-1 of the previous stack into slots 0 .. S-2 of
// the final stack, in 16-byte pieces; slot S-1 is the final frame's own.
#include <hip/hip_runtime.h>

#include "sf_generic_frame_dev.h"

__global__ __launch_bounds__(sfgf::kThreads) void sf_final_frames_kernel(SfGenericArgs a, const uint8_t* done) {
  extern __shared__ __attribute__((aligned(16))) uint8_t g_fb[];
  __shared__ double mtab[SF_NSLOT][3];
  __shared__ __attribute__((aligned(16))) uint32_t torw[sftd::kLdsWordsBig];
  const int env = blockIdx.x;
  if (done[env] == 0) return;  // (uniform: the whole workgroup reads the one byte)
  sfgf::env_frame(a, env, g_fb, mtab, torw);
}

hipError_t sf_launch_final_frames(const unsigned char* state, const uint8_t* done, int n_envs, int W, int H, double sx, double sy,
                                  double vp_x, double vp_y, double line_w, const double* trig, const double* arcs, const uint8_t* bg,
                                  const uint32_t* tabs, uint8_t* out, size_t out_stride, int resize, const SfGlyphAtlas* glyphs,
                                  hipStream_t stream) {
  if (n_envs <= 0) return hipSuccess;
  SfGenericArgs a{state, n_envs, W, H, sx, sy, vp_x, vp_y, line_w, trig, arcs, bg, tabs, out, out_stride, resize, glyphs};
  hipLaunchKernelGGL(sf_final_frames_kernel, dim3((unsigned)n_envs), dim3(sfgf::kThreads), sfgf::surface_bytes(W, H), stream, a, done);
  return hipGetLastError();
}

namespace {
constexpr int kShiftThreads = 256;
}

// grid (n_envs, pieces of an env's S - 1 slots): `bytes` = (S - 1) * frame_bytes, a multiple of 16
__global__ __launch_bounds__(kShiftThreads) void sf_final_stack_shift_kernel(const uint8_t* prev, uint8_t* fin, size_t stack_bytes,
                                                                            size_t frame_bytes, size_t bytes, const uint8_t* done) {
  const size_t env = blockIdx.x;
  if (done[env] == 0) return;  // (uniform)
  const size_t i = ((size_t)blockIdx.y * kShiftThreads + threadIdx.x) * 16;
  if (i >= bytes) return;
  *reinterpret_cast<uint4*>(fin + env * stack_bytes + i) = *reinterpret_cast<const uint4*>(prev + env * stack_bytes + frame_bytes + i);
}

hipError_t sf_launch_final_stack_shift(const uint8_t* prev, uint8_t* fin, int num_stack, size_t frame_bytes, const uint8_t* done,
                                       int n_envs, hipStream_t stream) {
  const size_t bytes = (size_t)(num_stack - 1) * frame_bytes;
  if (n_envs <= 0 || bytes == 0) return hipSuccess;
  const size_t per_block = (size_t)kShiftThreads * 16;
  hipLaunchKernelGGL(sf_final_stack_shift_kernel, dim3((unsigned)n_envs, (unsigned)((bytes + per_block - 1) / per_block)),
                     dim3(kShiftThreads), 0, stream, prev, fin, (size_t)num_stack * frame_bytes, frame_bytes, bytes, done);
  return hipGetLastError();
}
