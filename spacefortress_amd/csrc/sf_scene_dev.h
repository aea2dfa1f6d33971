// sf_scene_dev.h -- the reference's scene, painted from a lane's state: drawGameStateScaled (SRC/draw.cpp:227-270) once, for
// the two kernels that draw it in a run-time geometry.  sf_render_generic.hip keeps a whole W x H surface in LDS
// (ScenePainter<false>: rows [0, H), one plane); sf_render_view.hip draws a band of rows of a larger surface, grey or B, G, R
// (ScenePainter<true>: rows [r0, r1), planes x pstride, strokes that cannot reach the band culled).  Each kernel keeps its own
// LDS arrangement, background copy-in and way out; everything between is here: the lane's decode, its missiles filed by slot,
// every cairo_stroke / cairo_fill of the draw order through sftd::raster, one wave, wave-synchronously.  Device only.
// (sf_render.hip, the default geometry's frame kernel, has its own compile-time forms and reads draw records, not the state.)
#pragma once
#include <hip/hip_runtime.h>

#include "sf_internal.h"
#include "sf_raster.h"
#include "sf_tor_dev.h"

namespace sfs {
namespace {  // (device code of the one translation unit that includes it)

struct d2_t {
  double x, y;
};
struct i4_t {
  int x, y, z, w;
};
#define SFS_CHUNK(group, s) (tile + sfl::chunk_offset(SF_G_##group, (s)))
#define SFS_LD(T, base, off) (*reinterpret_cast<const T*>((base) + (off)))

struct Seg4 {
  double ax, ay, bx, by;
};
// wireframe segments, SRC/wireframe.cpp:11-67: kind 0 ship, 1 fortress, 2 missile, 3 shell
__device__ __forceinline__ Seg4 wire_seg(int kind, int k) {
  if (kind == 0) return Seg4{k == 2 ? 0.0 : -18.0, k == 1 ? 18.0 : 0.0, k == 0 ? 18.0 : (k == 1 ? 0.0 : -18.0), k == 2 ? -18.0 : 0.0};
  if (kind == 1) return Seg4{k >= 2 ? 18.0 : 0.0, k == 0 ? 0.0 : (k == 3 ? 18.0 : -18.0), k == 0 ? 36.0 : (k == 3 ? 0.0 : 18.0), k == 0 ? 0.0 : (k == 1 ? -18.0 : 18.0)};
  if (kind == 2) return Seg4{0.0, 0.0, k == 0 ? -25.0 : -5.0, k == 0 ? 0.0 : (k == 1 ? 5.0 : -5.0)};
  return Seg4{k == 0 ? -8.0 : (k == 2 ? 16.0 : 0.0), k == 1 ? -6.0 : (k == 3 ? 6.0 : 0.0), k == 1 ? 16.0 : (k == 3 ? -8.0 : 0.0), k == 0 ? -6.0 : (k == 2 ? 6.0 : 0.0)};
}

// source values B | G << 8 | R << 16 of the colour mode (SRC/wireframe.cpp's colours, SRC/draw.cpp:116-145)
constexpr unsigned kYellow = 0x00FFFF00u, kRed = 0x00FF0000u, kWhite = 0x00FFFFFFu;

// what a frame needs of lane l's state (ship_pos, timers_b, score, misc, small)
struct LaneScene {
  d2_t ship;
  int ship_angle, fort_angle;
  unsigned flags, mmask, smask, n_pool;
  int pnts, vlner, vuln_timer;  // (timers_b.w)
};
__device__ __forceinline__ LaneScene load_lane_scene(const unsigned char* tile, int l) {
  const int o16 = l * 16;
  const d2_t sp = SFS_LD(d2_t, SFS_CHUNK(ship_pos, 0), o16);
  const i4_t tb = SFS_LD(i4_t, SFS_CHUNK(timers_b, 0), o16);
  const i4_t sc = SFS_LD(i4_t, SFS_CHUNK(score, 0), o16);
  const i4_t mi = SFS_LD(i4_t, SFS_CHUNK(misc, 0), o16);
  const i4_t sm = SFS_LD(i4_t, SFS_CHUNK(small, 0), o16);
  return LaneScene{sp, (int)(int16_t)(sm.x & 0xFFFF), (int)(int16_t)((unsigned)sm.x >> 16), ((unsigned)sm.y >> 16) & 0xFFu,
                   (unsigned)mi.z & SF_MASK_LOW, (unsigned)mi.w & SF_MASK_LOW, (unsigned)mi.z >> SF_MPOOL_SHIFT,
                   (int)__int_as_float(sc.x), sc.z & 0xFFF, tb.w};
}

// lane l's missiles, out of the tile's pool, filed by slot (the reference draws in slot order, SRC/draw.cpp:243-247): x, y,
// heading; the other slots zero (the table is read under mmask only).  All `threads` threads of the workgroup call it and meet
// at its barriers.
__device__ __forceinline__ void file_missiles(const unsigned char* tile, int l, unsigned n_pool, int tid, int threads, double (*mtab)[3]) {
  for (int s = tid; s < SF_NSLOT; s += threads) mtab[s][0] = mtab[s][1] = mtab[s][2] = 0.0;
  __syncthreads();
  for (unsigned e = tid; e < n_pool; e += threads) {
    const unsigned meta = SFS_LD(uint32_t, SFS_CHUNK(missile_meta, 0), e * 4u);
    if (SF_MM_OWNER(meta) == (unsigned)l) {
      const d2_t m = SFS_LD(d2_t, SFS_CHUNK(missile_pos, 0), e * 16u);
      double* t = mtab[SF_MM_SLOT(meta)];
      t[0] = m.x;
      t[1] = m.y;
      t[2] = (double)SF_MM_ANGLE(meta);
    }
  }
  __syncthreads();
}

// what only a band has: its rows, its planes, the circle's curves.  The whole surface has none of it -- rows [0, H), one plane
// and the circle's two halves out of the arc table are compile-time facts there, and the painter's layout is without them
template <bool kBand>
struct BandPart {
  int r0, r1, planes, pstride;
  const double* circle;  // the circle's K curves (sft::ArcK each)
  int circle_k;
};
template <>
struct BandPart<false> {};

// One wave paints.  kBand == false: fb is the whole surface.  kBand == true: fb holds rows [r0, r1) only.
template <bool kBand>
struct ScenePainter : BandPart<kBand> {
  uint8_t* fb;     // row r0 of the surface at fb[0]; plane c at fb + c * pstride
  uint32_t* tor;   // sftd::kLdsWordsBig words, zero
  int W, H, tid;
  double sx, sy, vx, vy, lw;  // scale_x = W / vp_w, scale_y = H / vp_h (SRC/draw.cpp:70-71), viewport origin, line width
  const double* trig;         // cos, sin of deg2rad(k)
  const double* arcs;         // sf_arc_table: the rings' 84 arcs, then the circle's two halves

  __device__ __forceinline__ int row0() const { if constexpr (kBand) return this->r0; else return 0; }
  __device__ __forceinline__ int row1() const { if constexpr (kBand) return this->r1; else return H; }
  __device__ __forceinline__ int n_planes() const { if constexpr (kBand) return this->planes; else return 1; }
  __device__ __forceinline__ int plane_stride() const { if constexpr (kBand) return this->pstride; else return 0; }
  __device__ __forceinline__ int n_curves() const { if constexpr (kBand) return this->circle_k; else return 2; }
  __device__ __forceinline__ const double* curves() const { if constexpr (kBand) return this->circle; else return arcs + 8 * 84; }
  __device__ __forceinline__ sftd::Ctx tc() const { return sftd::Ctx{tor, fb, W, H, tid, sftd::kMaxQuadsBig}; }
  __device__ __forceinline__ void sync() const { tc().sync(); }
  __device__ __forceinline__ sftd::Band band(unsigned rgb, unsigned seams = 0u) const {
    if constexpr (kBand) return sftd::Band{this->r0, this->r1, this->planes, this->pstride, rgb, seams};
    else return sftd::Band{};
  }
  // can rows [dy0, dy1] (device space) reach into the band's; the whole surface culls nothing here: it runs every stroke and
  // leaves it to the rasteriser's box clip
  __device__ __forceinline__ bool meets(double dy0, double dy1) const {
    if constexpr (kBand) return dy1 >= (double)this->r0 - 1.0 && dy0 <= (double)this->r1 + 1.0;
    else return true;
  }
  __device__ __forceinline__ uint8_t* pixel(int px, int py) const { return fb + (py - row0()) * W + px; }
  // one pixel, every plane: lerp8 to grey (the same value in B, G, R) or to rgb's bytes
  __device__ __forceinline__ void put(int px, int py, int al, unsigned rgb, int grey) const {
    uint8_t* p = pixel(px, py);
    if (n_planes() == 1) *p = (uint8_t)sft::lerp8(grey, al, *p);
    else
      for (int c = 0; c < 3; c++) p[c * plane_stride()] = (uint8_t)sft::lerp8((int)((rgb >> (8 * c)) & 255u), al, p[c * plane_stride()]);
  }

  // drawWireFrame (SRC/draw.cpp:82-100): one cairo_stroke of the wireframe's lines -- as a call, for the strokes a frame may
  // or may not have; stroke_wireframe is the same code in line, for the ship's (below)
  __device__ void wireframe(int kind, int deg, double px, double py) const { stroke_wireframe(kind, deg, px, py); }
  __device__ __forceinline__ void stroke_wireframe(int kind, int deg, double px, double py) const {
    const double ext = 37.0 + lw;  // every stroke of a wireframe lies within 36 + lw user units of its position
    if (!meets((py - ext - vy) * sy, (py + ext - vy) * sy)) return;
    deg = deg < 0 ? 0 : (deg > 359 ? 359 : deg);
    const int n = (kind == 0 || kind == 2) ? 3 : 4;
    const unsigned rgb = kind == 2 ? kWhite : (kind == 3 ? kRed : kYellow);
    const sft::Affine v = sft::view_matrix(sx, sy, vx, vy);
    const double2 cs = *reinterpret_cast<const double2*>(trig + 2 * deg);
    const sft::Affine m = sft::object_matrix(v, px, py, cs.x, cs.y);
    if (kind == 1 && m.xy == 0.0 && m.yx == 0.0) {  // the rectilinear stroker (heading 0): boxes, exact area
      fort_boxes(m, rgb);
      return;
    }
    sft::Quad q = {};
    if (tid < n) {
      const Seg4 g = wire_seg(kind, tid);
      int x1, y1, x2, y2;
      sft::to_device(m, g.ax, g.ay, &x1, &y1);
      sft::to_device(m, g.bx, g.by, &x2, &y2);
      q = sft::stroke_quad(x1, y1, x2, y2, sx, sy, lw / 2);
    }
    sftd::raster<4, kBand>(tc(), q, tid < n, 0, kind == 1 ? sftd::kKindFort : (kind == 3 ? sftd::kKindShell : sftd::kKindLines3), 255,
                           band(rgb));
  }
  // the fortress at heading 0 under a matrix without rotation: cairo strokes the four axis-aligned lines as BOXES
  // (cairo-path-stroke-boxes.c) and fills their union through the box converter: exact area, alpha = c - (c >> 8)
  __device__ void fort_boxes(const sft::Affine& m, unsigned rgb) const {
    const int hx = sft::fx_from_double(fabs(m.xx) * lw / 2.0), hy = sft::fx_from_double(fabs(m.yy) * lw / 2.0);
    int bx[4][4];
    int X0 = 1 << 30, Y0 = 1 << 30, X1 = -(1 << 30), Y1 = -(1 << 30);
    for (int k = 0; k < 4; k++) {
      const Seg4 g = wire_seg(1, k);
      int x1, y1, x2, y2;
      sft::to_device(m, g.ax, g.ay, &x1, &y1);
      sft::to_device(m, g.bx, g.by, &x2, &y2);
      if (y1 == y2) { y1 -= hy; y2 += hy; } else { x1 -= hx; x2 += hx; }
      bx[k][0] = min(x1, x2); bx[k][1] = min(y1, y2); bx[k][2] = max(x1, x2); bx[k][3] = max(y1, y2);
      X0 = min(X0, bx[k][0]); Y0 = min(Y0, bx[k][1]); X1 = max(X1, bx[k][2]); Y1 = max(Y1, bx[k][3]);
    }
    const int px0 = max(X0 >> 8, 0), py0 = max(Y0 >> 8, row0()), px1 = min((X1 + 255) >> 8, W), py1 = min((Y1 + 255) >> 8, row1());
    const int bw = px1 - px0, n = bw > 0 && py1 > py0 ? bw * (py1 - py0) : 0;
    for (int i = tid; i < n; i += 64) {
      const int ry = i / bw, px = px0 + (i - ry * bw), py = py0 + ry;
      // |A u B u C u D| = sum of the four - the overlaps of the pairs that can overlap: the bar through the upright
      // (0, 2) and the two corners (1, 2), (2, 3)
      auto ov = [&](int a0, int a1, int b0, int b1, int c0, int c1) { const int o = min(min(a1, b1), c1) - max(max(a0, b0), c0); return o > 0 ? o : 0; };
      const int PX0 = px << 8, PX1 = PX0 + 256, PY0 = py << 8, PY1 = PY0 + 256;
      long long area = 0;
      for (int k = 0; k < 4; k++)
        area += (long long)ov(bx[k][0], bx[k][2], PX0, PX1, PX0, PX1) * ov(bx[k][1], bx[k][3], PY0, PY1, PY0, PY1);
      const int pr[3][2] = {{0, 2}, {1, 2}, {2, 3}};
      for (int j = 0; j < 3; j++) {
        const int a = pr[j][0], b = pr[j][1];
        area -= (long long)ov(bx[a][0], bx[a][2], bx[b][0], bx[b][2], PX0, PX1) * ov(bx[a][1], bx[a][3], bx[b][1], bx[b][3], PY0, PY1);
      }
      const int al = sft::box_area_to_alpha(area);
      if (al) put(px, py, al, rgb, 255);
    }
    sync();
  }
  // drawExplosion (SRC/draw.cpp:116-145): 7 rings of twelve 10-degree arcs, each its own stroke, then the radius-7 circle.
  // Every curve is flattened as cairo flattens it at THIS geometry's scale (sft::flatten_faces: one piece per arc at scale .2,
  // two at .4): four arcs of up to four pieces per call.  The circle is K curves, 32 / K lanes each: the whole surface stops
  // at scale .75, below cairo's switch from 2 Bezier segments per circle to 4 (cairo-arc.c: _arc_segments_needed), and takes
  // its two halves from the arc table; a view is told (circle, circle_k) and hands the seams between consecutive curves on.
  __device__ void explosion(double cx, double cy) const {
    const double ext = 64.0 + lw;
    if (!meets((cy - ext - vy) * sy, (cy + ext - vy) * sy)) return;
    const sft::Affine v = sft::view_matrix(sx, sy, vx, vy);
    const double hw = (double)(float)lw / 2;
    for (int ring = 0; ring < 7; ring++) {
      const double rad = 15.0 + 8 * ring + lw;
      if (!meets((cy - rad - vy) * sy, (cy + rad - vy) * sy)) continue;
      const bool yellow = 15 + 8 * ring < 60;
      for (int chunk = 0; chunk < 3; chunk++) {
        sft::Quad q = {};
        bool valid = false;
        if (tid < 16) {
          const double* kp = arcs + 8 * (12 * ring + 4 * chunk + (tid >> 2));
          int px[6], py[6], tx[6], ty[6];
          const int n = sft::flatten_faces(sft::arc_knots(v, cx, cy, sft::ArcK{kp[0], kp[1], kp[2], kp[3], kp[4], kp[5], kp[6], kp[7]}), px, py, tx, ty, 5);
          const int p = tid & 3;
          if (p < n - 1) {
            valid = true;
            q = sft::faces_quad(px[p], py[p], tx[p], ty[p], px[p + 1], py[p + 1], tx[p + 1], ty[p + 1], sx, sy, hw);
          }
        }
        sftd::raster<4, kBand>(tc(), q, valid, tid & ~3, sftd::kKindSingle, yellow ? 191 : 128, band(yellow ? kYellow : kRed));
      }
    }
    if (!meets((cy - 8.0 - lw - vy) * sy, (cy + 8.0 + lw - vy) * sy)) return;
    const int K = n_curves(), per = 32 / K, cap = per + 1;
    sft::Quad q = {};
    bool valid = false;
    int n = 0;
    {
      int px[17], py[17], tx[17], ty[17];
      const int c = min(tid / per, K - 1);
      const double* kp = curves() + 8 * c;
      n = sft::flatten_faces(sft::arc_knots(v, cx, cy, sft::ArcK{kp[0], kp[1], kp[2], kp[3], kp[4], kp[5], kp[6], kp[7]}), px, py, tx, ty, cap);
      const int p = tid - c * per;
      if (tid < 32 && p < n - 1) {
        valid = true;
        q = sft::faces_quad(px[p], py[p], tx[p], ty[p], px[p + 1], py[p + 1], tx[p + 1], ty[p + 1], sx, sy, hw);
      }
    }
    if constexpr (kBand) {
      // the first piece of curves 1 .. K - 1 (pieces are numbered over the valid lanes, curve after curve)
      unsigned seams = (unsigned)K;
      int first = 0;
      for (int c = 0; c < K; c++) {
        if (c > 0) seams |= (unsigned)first << (8 + 6 * (c - 1));
        first += __builtin_amdgcn_readlane(n, c * per) - 1;
      }
      sftd::raster<16, true>(tc(), q, valid, 0, sftd::kKindRing, 191, band(kYellow, seams));
    } else {
      const int m0 = __builtin_amdgcn_readfirstlane(n - 1);  // (lane 0 flattened the first half)
      sftd::raster<16>(tc(), q, valid, 0, sftd::kKindRing | (m0 << 8), 191);
    }
  }
  // the score (drawScore, SRC/draw.cpp:161-173): "%07d", grey .5 through the coverage of this geometry's glyph atlas
  // (sf_glyphs.h) -- a lane per pixel of the text's box --, or, without one, the seven-segment FALLBACK (sf_raster.h: equal to
  // no reference pixels) -- a lane per pixel composites the segments that touch it in the strokes' order.  Grey in both modes.
  __device__ void score(int pnts, const SfGlyphAtlas* G) const {
    if (G && G->gw) {  // (uniform)
      const uint32_t chars = sfg::score_chars(pnts);
      const int bx0 = max((int)G->x_min, 0), bx1 = min((int)G->x_max + 6 * G->advance + G->gw, W);
      const int by0 = max(G->y0, row0()), by1 = min(G->y0 + G->gh, row1());
      const int bw = bx1 - bx0, n = bw > 0 && by1 > by0 ? bw * (by1 - by0) : 0;
      for (int i = tid; i < n; i += 64) {
        const int ry = i / bw, px = bx0 + (i - ry * bw), py = by0 + ry;
        uint8_t* p = pixel(px, py);
        for (int c = 0; c < n_planes(); c++) p[c * plane_stride()] = (uint8_t)sfg::text_pixel(G, chars, px, py, p[c * plane_stride()]);
      }
      sync();
      return;
    }
    // (the fallback: float64 here -- the segment model is ours, oracle/render_np.py evaluates it in float64, and these kernels have the time)
    const unsigned long long masks = sfr::score_masks(pnts);
    auto dx = [&](double x) { return (x - vx) * sx; };
    auto dy = [&](double y) { return (y - vy) * sy; };
    const double Wg = SF_TXT_W, Hg = SF_TXT_H, T = SF_TXT_T, m0 = 0.5 * (SF_TXT_H - SF_TXT_T), m1 = 0.5 * (SF_TXT_H + SF_TXT_T);
    const double sx0[7] = {0, Wg - T, Wg - T, 0, 0, 0, 0}, sx1[7] = {Wg, Wg, Wg, Wg, T, T, Wg};
    const double sy0[7] = {0, T, m1, Hg - T, m1, T, m0}, sy1[7] = {T, m0, Hg - T, Hg, Hg - T, m0, m1};
    const double tx0 = dx((double)SF_TXT_X0 + SF_TXT_PAD), tx1 = dx((double)SF_TXT_X0 + 6.0 * SF_TXT_ADV + SF_TXT_PAD + SF_TXT_W);
    const double ty0 = dy((double)SF_TXT_TOP), ty1 = dy((double)SF_TXT_TOP + SF_TXT_H);
    const int bx0 = max((int)floor(tx0), 0), by0 = max((int)floor(ty0), row0()), bx1 = min((int)ceil(tx1), W), by1 = min((int)ceil(ty1), row1());
    const int bw = bx1 - bx0, n = bw > 0 && by1 > by0 ? bw * (by1 - by0) : 0;
    for (int i = tid; i < n; i += 64) {
      const int ry = i / bw, px = bx0 + (i - ry * bw), py = by0 + ry;
      const double fpx = (double)px, fpy = (double)py;
      for (int c = 0; c < n_planes(); c++) {
        uint8_t* p = pixel(px, py) + c * plane_stride();
        int d = *p;
        for (int cell = 0; cell < 7; cell++) {
          const double gx = (double)SF_TXT_X0 + (double)SF_TXT_ADV * (double)cell + SF_TXT_PAD, gy = SF_TXT_TOP;
          const unsigned bits = (unsigned)(masks >> (7 * cell)) & 0x7Fu;
#pragma unroll
          for (int seg = 0; seg < 7; seg++) {
            if (!((bits >> seg) & 1u)) continue;
            // the model's own arithmetic: the segment's rectangle clipped to the pixel, its area (render_np.pixel_area)
            const double ox = fmin(dx(gx + sx1[seg]), fpx + 1.0) - fmax(dx(gx + sx0[seg]), fpx);
            const double oy = fmin(dy(gy + sy1[seg]), fpy + 1.0) - fmax(dy(gy + sy0[seg]), fpy);
            if (ox > 0.0 && oy > 0.0) {
              const int m = (int)(fmin(ox * oy, 1.0) * 255.0 + 0.5);
              if (m > 0) d = sfr::over_un8(d, 128, m);
            }
          }
        }
        *p = (uint8_t)d;
      }
    }
    sync();
  }
  // drawVlner (SRC/draw.cpp:207-225): cairo_rectangle(x, y, w, h) + cairo_fill: the box converter, grey in both modes
  __device__ void rect(double x, double y, double w, double h, int grey) const {
    const sft::Affine v = sft::view_matrix(sx, sy, vx, vy);
    int x0, y0;
    sft::to_device(v, x, y, &x0, &y0);
    int x1 = x0 + sft::fx_from_double(v.xx * w + v.xy * 0.0), y1 = y0 + sft::fx_from_double(v.yx * 0.0 + v.yy * h);
    if (x1 < x0) { const int t = x0; x0 = x1; x1 = t; }
    if (y1 < y0) { const int t = y0; y0 = y1; y1 = t; }
    const int px0 = max(x0 >> 8, 0), py0 = max(y0 >> 8, row0()), px1 = min((x1 + 255) >> 8, W), py1 = min((y1 + 255) >> 8, row1());
    const int bw = px1 - px0, n = bw > 0 && py1 > py0 ? bw * (py1 - py0) : 0;
    const unsigned rgb = (unsigned)grey * 0x010101u;
    for (int i = tid; i < n; i += 64) {
      const int ry = i / bw, px = px0 + (i - ry * bw), py = py0 + ry;
      const int ox = min(x1, (px + 1) << 8) - max(x0, px << 8), oy = min(y1, (py + 1) << 8) - max(y0, py << 8);
      if (ox > 0 && oy > 0) {
        const int al = sft::box_area_to_alpha((long long)ox * oy);
        if (al) put(px, py, al, rgb, grey);
      }
    }
    sync();
  }

  // drawGameStateScaled's objects, in its order (SRC/draw.cpp:233-254,266-268), over the background the kernel copied in
  __device__ __forceinline__ void draw(const LaneScene& s, const double (*mtab)[3], const unsigned char* tile, int o16, const SfGlyphAtlas* glyphs) const {
    // ship (:233-237), fortress (:238-242).  The ship's wireframe, the one stroke of nearly every frame, is in line: its kind a
    // constant, the painter's members in registers; every other stroke is a call (profiles/scene_painter.md).
    if (s.flags & SF_FL_SHIP_ALIVE) stroke_wireframe(0, s.ship_angle, s.ship.x, s.ship.y);
    else explosion(s.ship.x, s.ship.y);
    if (s.flags & SF_FL_FORT_ALIVE) wireframe(1, s.fort_angle, sfc::fort_x, sfc::fort_y);
    else explosion(sfc::fort_x, sfc::fort_y);
    // missiles (:243-247), shells (:248-253: only once clear of the fortress; drawWireFrame takes the heading as an int)
    for (int k = 0; k < SF_NSLOT; k++)
      if ((s.mmask >> k) & 1u) wireframe(2, (int)mtab[k][2], mtab[k][0], mtab[k][1]);
    for (int k = 0; k < SF_NSLOT; k++)
      if ((s.smask >> k) & 1u) {
        const d2_t p = SFS_LD(d2_t, SFS_CHUNK(shell_pos, k), o16), v = SFS_LD(d2_t, SFS_CHUNK(shell_vel, k), o16);
        const double ddx = p.x - sfc::fort_x, ddy = p.y - sfc::fort_y;
        if (sqrt(ddx * ddx + ddy * ddy) > 21.0) {
          double ang = atan2(v.y, v.x) * 180.0 / M_PI;
          if (ang < 0) ang += 360.0;
          wireframe(3, (int)ang, p.x, p.y);
        }
      }
    score(s.pnts, glyphs);
    // vulnerability bar (drawVlner, :205-225,268)
    const bool kill = s.vlner > 10 && s.vuln_timer < sfc::vuln_time;
    rect(355.0 - 100, 335.0 + 187, 200.0, 10.0, 84);
    if (s.vlner > 0) rect(355.0 - 100, 335.0 + 187, (double)(20 * (s.vlner > 10 ? 10 : s.vlner)), 10.0, kill ? 255 : 168);
  }
};

#undef SFS_CHUNK
#undef SFS_LD

}  // namespace
}  // namespace sfs
