// sf_render_generic.hip -- the image observation in ANY geometry the reference's constructor takes:
//   SSF_Env(scale, viewport, ls)  ENV:50-60  ->  sf.Game(width = int(vw * scale), height = int(vh * scale), viewport, lw = ls)
//   drawGameStateScaled           SRC/draw.cpp:256-270: scale(w / vw, h / vh), translate(-vx, -vy), line width ls user units
// sf_render.hip is the frame kernel of the DEFAULT geometry (scale .2, viewport (130, 80, 450, 460), ls 3: the trainer's,
// BASELINE configs[4]): a wave per env, the 90x92 surface, its tap periods, picture caches and tables all compile-time
// facts.  This file is the general renderer behind sf_set_image_geometry: one WORKGROUP per env, the W x H surface in
// dynamic LDS, every cairo_stroke of the reference's draw order (SRC/draw.cpp:227-254,266-268) rasterised in place, one object
// after the other, the way cairo's image backend does it (sf_tor.h / sf_tor_dev.h: the same code as the default geometry's
// kernel, the geometry a run-time argument), no caches, no shortcuts -- sfs::ScenePainter<false>, sf_scene_dev.h: the painter
// this kernel shares with sf_render_view.hip, over the whole surface --; then cv2.resize(.., (84, 84), INTER_AREA) with per-batch
// tap tables for W, H < 3 * 84 (OpenCV's resizeArea_ arithmetic, sf_image.cpp).  It reads the state, not the draw records.
// Phases: all four waves copy the background in (16-byte pieces); wave 0 alone rasterises the objects, wave-synchronously, and
// the score's glyphs with a lane per pixel of their box; all four waves resample, four pixels and one 32-bit store per thread.
// Correctness in every geometry (tests/test_gpu_image.py: against frames the reference's own renderer drew in four of them);
// speed in the one the benchmark names.
#include <hip/hip_runtime.h>

#include "sf_internal.h"
#include "sf_scene_dev.h"

namespace {
constexpr int kThreads = 256;
}

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

__global__ __launch_bounds__(kThreads) void sf_render_generic_kernel(SfGenericArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t g_fb[];
  __shared__ double mtab[SF_NSLOT][3];
  __shared__ __attribute__((aligned(16))) uint32_t torw[sftd::kLdsWordsBig];
  const int tid = threadIdx.x, env = blockIdx.x;
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

hipError_t sf_launch_render_generic(const unsigned char* state, int n_envs, int W, int H, double sx, double sy, double vp_x, double vp_y,
                                    double line_w, const double* trig, const double* arcs, const uint8_t* bg, const uint32_t* tabs,
                                    uint8_t* out, size_t out_stride, int resize, const SfGlyphAtlas* glyphs, hipStream_t stream) {
  if (n_envs <= 0) return hipSuccess;
  SfGenericArgs a{state, n_envs, W, H, sx, sy, vp_x, vp_y, line_w, trig, arcs, bg, tabs, out, out_stride, resize, glyphs};
  const size_t lds = ((size_t)W * H + 15) & ~(size_t)15;
  hipLaunchKernelGGL(sf_render_generic_kernel, dim3((unsigned)n_envs), dim3(kThreads), lds, stream, a);
  return hipGetLastError();
}
