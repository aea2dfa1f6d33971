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

#include "sf_generic_frame_dev.h"

__global__ __launch_bounds__(sfgf::kThreads) void sf_render_generic_kernel(SfGenericArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t g_fb[];
  __shared__ double mtab[SF_NSLOT][3];
  __shared__ __attribute__((aligned(16))) uint32_t torw[sftd::kLdsWordsBig];
  sfgf::env_frame(a, blockIdx.x, g_fb, mtab, torw);
}

hipError_t sf_launch_render_generic(const unsigned char* state, int n_envs, int W, int H, double sx, double sy, double vp_x, double vp_y,
                                    double line_w, const double* trig, const double* arcs, const uint8_t* bg, const uint32_t* tabs,
                                    uint8_t* out, size_t out_stride, int resize, const SfGlyphAtlas* glyphs, hipStream_t stream) {
  if (n_envs <= 0) return hipSuccess;
  SfGenericArgs a{state, n_envs, W, H, sx, sy, vp_x, vp_y, line_w, trig, arcs, bg, tabs, out, out_stride, resize, glyphs};
  hipLaunchKernelGGL(sf_render_generic_kernel, dim3((unsigned)n_envs), dim3(sfgf::kThreads), sfgf::surface_bytes(W, H), stream, a);
  return hipGetLastError();
}
