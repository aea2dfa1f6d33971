// sf_generic_frame_dev.h -- one env's frame in a run-time geometry, by one workgroup of sfgf::kThreads threads: the body the
// general renderer (sf_render_generic.hip: every env of a batch) and the final frames (sf_final_frames.hip: the envs that
// finished in the step in front) share.  The W x H surface lives in the caller's dynamic LDS; phases: all four waves copy the
// background in (16-byte pieces); wave 0 alone rasterises the objects, wave-synchronously (sfs::ScenePainter<false>,
// sf_scene_dev.h), and the score's glyphs with a lane per pixel of their box; all four waves leave the surface, or resample it
// to 84 x 84, four pixels and one 32-bit store per thread.  It reads the state, not the draw records.  Device only.
#pragma once
#include <hip/hip_runtime.h>

#include "sf_internal.h"
#include "sf_scene_dev.h"

struct SfGenericArgs {
  const unsigned char* state;
  int n_envs, W, H;
  double sx, sy, vx, vy, lw;
  const double* trig;
  const double* arcs;
  const uint8_t* bg;      // W * H bytes: the hexagons on black (sf_image.cpp: sf_image_background_geom)
  const uint32_t* tabs;   // resize != 0: 8 words per destination column, then per row: first, count, 4 weights, 2 pad
  uint8_t* out;
  size_t out_stride;
  int resize;
  const SfGlyphAtlas* glyphs;  // the score text's glyph atlas for THIS geometry (sf_glyphs.h); null or gw == 0: the fallback
};

namespace sfgf {
namespace {  // (device code of the translation unit that includes it)

constexpr int kThreads = 256;

// dynamic LDS of a launch: the surface in whole 16-byte pieces
inline size_t surface_bytes(int W, int H) { return ((size_t)W * H + 15) & ~(size_t)15; }

// g_fb: the launch's dynamic LDS (surface_bytes); mtab, torw: the kernel's static LDS.  Every thread of the workgroup calls it.
__device__ __forceinline__ void env_frame(const SfGenericArgs& a, int env, uint8_t* g_fb, double (*mtab)[3], uint32_t* torw) {
  const int tid = threadIdx.x;
  const int W = a.W, H = a.H;
  const sfs::ScenePainter<false> P{{}, g_fb, torw, W, H, tid, a.sx, a.sy, a.vx, a.vy, a.lw, a.trig, a.arcs};
  for (int i = tid; i < sftd::kLdsWordsBig; i += kThreads) torw[i] = 0u;
  const unsigned char* tile = a.state + (long)(env >> 6) * sfl::kTileBytes;
  const int l = env & 63;
  const sfs::LaneScene scene = sfs::load_lane_scene(tile, l);
  // the background: both hexagons stroked on black (SRC/draw.cpp:230-231,262-263)
  // (16 bytes per thread and piece, four pieces in flight: left byte by byte, every iteration waits out its own L2 round
  //  trip -- 64 of them, a hundred microseconds per frame.  The host pads the background to whole pieces.)
  {
    const uint4* src = reinterpret_cast<const uint4*>(a.bg);
    uint4* dst = reinterpret_cast<uint4*>(g_fb);
    const int n16 = (W * H + 15) >> 4;
    for (int base = 0; base < n16; base += 4 * kThreads) {
      uint4 v[4];
#pragma unroll
      for (int k = 0; k < 4; k++) v[k] = src[min(base + k * kThreads + tid, n16 - 1)];
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (base + k * kThreads + tid < n16) dst[base + k * kThreads + tid] = v[k];
    }
  }
  sfs::file_missiles(tile, l, scene.n_pool, tid, kThreads, mtab);
  if (tid < 64) P.draw(scene, mtab, tile, l * 16, a.glyphs);  // wave 0 composites
  __syncthreads();
  uint8_t* const frame_out = a.out + (size_t)env * a.out_stride;
  if (!a.resize) {
    // the raw frame leaves in 4-byte words at 4-byte aligned addresses (a frame of W * H bytes need not start on one: a few
    // bytes first): byte stores are one 64-byte write per wave instruction and were half of the launch
    const int head = (int)((0u - (unsigned)(uintptr_t)frame_out) & 3u), nw = (W * H - head) >> 2, tail = head + 4 * nw;
    if (tid < head) frame_out[tid] = g_fb[tid];
    for (int j = tid; j < nw; j += kThreads) {
      uint32_t v;
      __builtin_memcpy(&v, g_fb + head + 4 * j, 4);
      *reinterpret_cast<uint32_t*>(frame_out + head + 4 * j) = v;
    }
    if (tail + tid < W * H) frame_out[tail + tid] = g_fb[tail + tid];
    return;
  }
  // cv2.resize(frame, (84, 84), INTER_AREA): per source row buf = sum alpha * S in table order, sum (+)= beta * buf in table
  // order, saturate_cast<uchar> (round half to even) -- resizeArea_<uchar, float>.  Four destination pixels of a row per
  // thread, one aligned 32-bit store (the 84x84 frames are 16-byte aligned); the taps are loaded before the sums start.
  const uint4* ct4 = reinterpret_cast<const uint4*>(a.tabs);
  const uint4* rt4 = reinterpret_cast<const uint4*>(a.tabs + 8 * SF_OUT);
  for (int i = tid; i < SF_OUT * (SF_OUT / 4); i += kThreads) {
    const int oy = i / (SF_OUT / 4), ox0 = 4 * (i - oy * (SF_OUT / 4));
    const uint4 ra = rt4[2 * oy], rb = rt4[2 * oy + 1];  // first, count, b0, b1 | b2, b3, -, -
    uint4 ca[4], cb[4];
#pragma unroll
    for (int p = 0; p < 4; p++) {
      ca[p] = ct4[2 * (ox0 + p)];
      cb[p] = ct4[2 * (ox0 + p) + 1];
    }
    const int rf = (int)ra.x, rc = (int)ra.y;
    const float beta[4] = {__uint_as_float(ra.z), __uint_as_float(ra.w), __uint_as_float(rb.x), __uint_as_float(rb.y)};
    unsigned word = 0u;
#pragma unroll
    for (int p = 0; p < 4; p++) {
      const int cf = (int)ca[p].x, cc = (int)ca[p].y;
      const float al[4] = {__uint_as_float(ca[p].z), __uint_as_float(ca[p].w), __uint_as_float(cb[p].x), __uint_as_float(cb[p].y)};
      float sum = 0.f;
      for (int k = 0; k < rc; k++) {
        const uint8_t* S = g_fb + (rf + k) * W + cf;
        float bsum = 0.f;
#pragma unroll
        for (int j = 0; j < 4; j++)
          if (j < cc) bsum += (float)S[j] * al[j];
        const float bk = k == 0 ? beta[0] : (k == 1 ? beta[1] : (k == 2 ? beta[2] : beta[3]));
        sum = k == 0 ? bk * bsum : sum + bk * bsum;
      }
      int v = (int)rintf(sum);
      v = v < 0 ? 0 : (v > 255 ? 255 : v);
      word |= (unsigned)v << (8 * p);
    }
    *reinterpret_cast<uint32_t*>(frame_out + oy * SF_OUT + ox0) = word;
  }
}

}  // namespace
}  // namespace sfgf
