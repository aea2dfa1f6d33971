// sf_render_view.hip -- a lane's frame in any VIEW up to 1.0 pixel per user unit, grey or colour: what the reference's
// Game(config, lw, grayscale, width, height, viewport).draw() leaves in pb_pixels (SRC/pymodule.cpp:319-354, SRC/draw.cpp:
// 227-270), for the lanes of a batch, from their state.  sf_render_generic.hip keeps a whole surface in LDS and stops at
// 251 pixels a side; a view of the human-play front-end is 450 x 460 (207 KB a plane, 620 KB in colour), so this kernel
// TILES: one workgroup (one wave) per (lane, band of rows), the band's planes in LDS -- grey, or B, G, R --, every stroke of
// the reference's draw order that touches the band rasterised into it by the general renderer's code (sfs::ScenePainter<true>,
// sf_scene_dev.h, over sftd::raster in its band form: boxes clipped to the band's rows, whose rows depend on nothing outside
// them), then the score's glyphs and the bar, then the band's rows leave once, in 16-byte stores.
// Colour is the grey pipeline once per channel: one coverage per stroke, each channel lerped to the stroke's own source
// value (SRC/draw.cpp: hexagons 0,1,0; ship and fortress 1,1,0 (r, g, b); missiles 1,1,1; shells 1,0,0; explosion arcs 1,1,0
// below radius 60, 1,0,0 above; the closing circle 1,1,0; the score and the bar grey in both modes).
// The circle of radius 7 is cut by cairo into 2 Bezier segments per half up to 5.4 device pixels, 4 beyond (cairo-arc.c:
// _arc_segments_needed over the view matrix); the host counts them (sf_view_circle_segments) and the seams between every two
// consecutive curves go into the stroke's inclusion-exclusion (sftd::band_sources).
#include <hip/hip_runtime.h>

#include "sf_internal.h"
#include "sf_scene_dev.h"
#include "sf_view.h"

struct SfViewArgs {
  const unsigned char* state;
  int first_lane, W, H, band_h, planes, format;
  double sx, sy, vx, vy, lw;
  const double* trig;
  const double* arcs;
  const double* circle;
  int circle_k;
  const uint8_t* bg;        // the view's hexagons, grey, band after band: band b at b * bg_stride (16-byte pieces)
  size_t bg_stride;
  const SfGlyphAtlas* glyphs;
  uint8_t* out;
  size_t lane_stride;
};

__global__ __launch_bounds__(64) void sf_render_view_kernel(SfViewArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint8_t v_fb[];
  __shared__ double mtab[SF_NSLOT][3];
  __shared__ __attribute__((aligned(16))) uint32_t torw[sftd::kLdsWordsBig];
  const int tid = threadIdx.x, band = blockIdx.x, lane = a.first_lane + (int)blockIdx.y;
  const int W = a.W, r0 = band * a.band_h, r1 = min(r0 + a.band_h, a.H), rows = r1 - r0;
  const int plane = W * a.band_h;  // (a band's plane; the host keeps W * band_h a multiple of 16)
  const sfs::ScenePainter<true> P{{r0, r1, a.planes, plane, a.circle, a.circle_k},
                                  v_fb, torw, W, a.H, tid, a.sx, a.sy, a.vx, a.vy, a.lw, a.trig, a.arcs};
  for (int i = tid; i < sftd::kLdsWordsBig; i += 64) torw[i] = 0u;
  const unsigned char* tile = a.state + (long)(lane >> 6) * sfl::kTileBytes;
  const int l = lane & 63;
  const sfs::LaneScene scene = sfs::load_lane_scene(tile, l);
  // the background: the grey hexagons -- in colour their G plane (source 0, 1, 0), B and R black
  {
    const uint4* src = reinterpret_cast<const uint4*>(a.bg + (size_t)band * a.bg_stride);
    uint4* dst = reinterpret_cast<uint4*>(v_fb);
    const int n16 = plane >> 4, g = a.planes == 3 ? 1 : 0;
    for (int i = tid; i < n16; i += 64) {
      const uint4 v = src[i];
      dst[g * n16 + i] = v;
      if (a.planes == 3) {
        dst[i] = uint4{0u, 0u, 0u, 0u};
        dst[2 * n16 + i] = uint4{0u, 0u, 0u, 0u};
      }
    }
  }
  sfs::file_missiles(tile, l, scene.n_pool, tid, 64, mtab);
  P.draw(scene, mtab, tile, l * 16, a.glyphs);
  __syncthreads();
  // the band's rows leave once: byte j of them is pixel j / bpp, channel j % bpp of the format -- up to a 16-byte boundary byte by
  // byte, then 16 bytes per lane and store, then the tail
  const int bpp = a.format == SF_VIEW_GRAY ? 1 : (a.format == SF_VIEW_RGB ? 3 : 4);
  uint8_t* const dst = a.out + (size_t)blockIdx.y * a.lane_stride + (size_t)r0 * W * bpp;
  const int nbytes = rows * W * bpp;
  auto byte_at = [&](int j) -> uint8_t {
    const int px = j / bpp, ch = j - px * bpp;
    if (ch == 3) return 255;
    // BGRX: channel 0 = B = plane 0; RGB: channel 0 = R = plane 2; grey: the one plane
    const int pl = a.planes == 1 ? 0 : (a.format == SF_VIEW_RGB ? 2 - ch : ch);
    return v_fb[pl * plane + px];
  };
  const int head = min((int)((0u - (unsigned)(uintptr_t)dst) & 15u), nbytes), n16 = (nbytes - head) >> 4, tail = head + 16 * n16;
  if (tid < head) dst[tid] = byte_at(tid);
  for (int j = tid; j < n16; j += 64) {
    uint32_t w4[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int b = head + 16 * j + 4 * k;
      w4[k] = (uint32_t)byte_at(b) | (uint32_t)byte_at(b + 1) << 8 | (uint32_t)byte_at(b + 2) << 16 | (uint32_t)byte_at(b + 3) << 24;
    }
    *reinterpret_cast<uint4*>(dst + head + 16 * j) = uint4{w4[0], w4[1], w4[2], w4[3]};
  }
  for (int j = tail + tid; j < nbytes; j += 64) dst[j] = byte_at(j);
}

hipError_t sf_launch_render_view(const SfViewLaunch& v, hipStream_t stream) {
  if (v.n_lanes <= 0) return hipSuccess;
  SfViewArgs a{v.state, v.first_lane, v.W, v.H, v.band_h, v.planes, v.format, v.sx, v.sy, v.vx, v.vy, v.lw, v.trig, v.arcs,
               v.circle, v.circle_k, v.bg, v.bg_stride, v.glyphs, v.out, v.lane_stride};
  const int n_bands = (v.H + v.band_h - 1) / v.band_h;
  const size_t lds = (size_t)v.planes * v.W * v.band_h;
  hipLaunchKernelGGL(sf_render_view_kernel, dim3((unsigned)n_bands, (unsigned)v.n_lanes), dim3(64), lds, stream, a);
  return hipGetLastError();
}
