// sf_view.h -- the launch of sf_render_view.hip (sf_render_view in include/sfmi.h): what the host resolved of a view
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "sf_glyphs.h"

struct SfViewLaunch {
  const unsigned char* state;
  int first_lane, n_lanes;
  int W, H, band_h;  // the surface; rows per workgroup (W * band_h a multiple of 16, band_h <= 32)
  int planes;        // 1 grey, 3 colour (B, G, R)
  int format;        // SF_VIEW_BGRX / SF_VIEW_RGB / SF_VIEW_GRAY
  double sx, sy, vx, vy, lw;
  const double* trig;    // sf_trig_table
  const double* arcs;    // sf_arc_table
  const double* circle;  // circle_k curves of the radius-7 circle, 8 doubles each (sft::ArcK)
  int circle_k;
  const uint8_t* bg;     // the grey hexagons, band b's rows at b * bg_stride (whole 16-byte pieces)
  size_t bg_stride;
  const SfGlyphAtlas* glyphs;  // gw == 0: the seven-segment fallback
  uint8_t* out;
  size_t lane_stride;
};

hipError_t sf_launch_render_view(const SfViewLaunch& v, hipStream_t stream);

// sf_view_host.cpp (no HIP calls): a caller's sf_view resolved against the config's size (the reference's defaulting,
// SRC/pymodule.cpp:345-349) and checked; the host tables of a resolved view
struct SfViewRes {
  int w, h, planes, format;
  double sx, sy, vx, vy, lw;  // sx = w / vp_w, sy = h / vp_h (SRC/draw.cpp:70-71)
  int band_h, circle_k;
  SfGlyphAtlas glyphs;        // gw == 0: the seven-segment fallback
};
struct sf_view;
int sf_view_resolve(const sf_view* v, int cfg_w, int cfg_h, SfViewRes* r);
// the grey hexagons band by band (band b's rows at b * *bg_stride); the circle's circle_k curves as sft::ArcK
int sf_view_tables(const SfViewRes& r, std::vector<uint8_t>* bg, size_t* bg_stride, std::vector<double>* circle);
