// sf_render_view.hip -- a lane's frame in any VIEW up to 1.0 pixel per user unit, grey or colour: what the reference's
// Game(config, lw, grayscale, width, height, viewport).draw() leaves in pb_pixels (SRC/pymodule.cpp:319-354, SRC/draw.cpp:
// 227-270), for the lanes of a batch, from their state.  sf_render_generic.hip keeps a whole surface in LDS and stops at
// 251 pixels a side; a view of the human-play front-end is 450 x 460 (207 KB a plane, 620 KB in colour), so this kernel
// TILES: one workgroup (one wave) per (lane, band of rows), the band's planes in LDS -- grey, or B, G, R --, every stroke of
// the reference's draw order that touches the band rasterised into it by the general renderer's code (sftd::raster in its
// band form: boxes clipped to the band's rows, whose rows depend on nothing outside them), then the score's glyphs and the
// bar, then the band's rows leave once, in 16-byte stores.
// Colour is the grey pipeline once per channel: one coverage per stroke, each channel lerped to the stroke's own source
// value (SRC/draw.cpp: hexagons 0,1,0; ship and fortress 1,1,0 (r, g, b); missiles 1,1,1; shells 1,0,0; explosion arcs 1,1,0
// below radius 60, 1,0,0 above; the closing circle 1,1,0; the score and the bar grey in both modes).
// The circle of radius 7 is cut by cairo into 2 Bezier segments per half up to 5.4 device pixels, 4 beyond (cairo-arc.c:
// _arc_segments_needed over the view matrix); the host counts them (sf_view_circle_segments) and the seams between every two
// consecutive curves go into the stroke's inclusion-exclusion (sftd::band_sources).
#include <hip/hip_runtime.h>

#include "sf_internal.h"
#include "sf_raster.h"
#include "sf_tor_dev.h"
#include "sf_view.h"

namespace {

struct d2_t {
  double x, y;
};
struct i4_t {
  int x, y, z, w;
};
#define V_CHUNK(group, s) (tile + sfl::chunk_offset(SF_G_##group, (s)))
#define V_LD(T, base, off) (*reinterpret_cast<const T*>((base) + (off)))

struct Seg4 {
  double ax, ay, bx, by;
};
// wireframe segments, SRC/wireframe.cpp:11-67: kind 0 ship, 1 fortress, 2 missile, 3 shell (as sf_render_generic.hip)
__device__ __forceinline__ Seg4 wire_seg(int kind, int k) {
  if (kind == 0) return Seg4{k == 2 ? 0.0 : -18.0, k == 1 ? 18.0 : 0.0, k == 0 ? 18.0 : (k == 1 ? 0.0 : -18.0), k == 2 ? -18.0 : 0.0};
  if (kind == 1) return Seg4{k >= 2 ? 18.0 : 0.0, k == 0 ? 0.0 : (k == 3 ? 18.0 : -18.0), k == 0 ? 36.0 : (k == 3 ? 0.0 : 18.0), k == 0 ? 0.0 : (k == 1 ? -18.0 : 18.0)};
  if (kind == 2) return Seg4{0.0, 0.0, k == 0 ? -25.0 : -5.0, k == 0 ? 0.0 : (k == 1 ? 5.0 : -5.0)};
  return Seg4{k == 0 ? -8.0 : (k == 2 ? 16.0 : 0.0), k == 1 ? -6.0 : (k == 3 ? 6.0 : 0.0), k == 1 ? 16.0 : (k == 3 ? -8.0 : 0.0), k == 0 ? -6.0 : (k == 2 ? 6.0 : 0.0)};
}

// source values B | G << 8 | R << 16 of the colour mode (SRC/wireframe.cpp's colours, SRC/draw.cpp:116-145)
constexpr unsigned kYellow = 0x00FFFF00u, kRed = 0x00FF0000u, kWhite = 0x00FFFFFFu;

struct Ctx {
  uint8_t* fb;     // the band's planes: row r0 of the surface at fb[0]; plane c at fb + c * pstride
  uint32_t* tor;
  int W, H, tid, r0, r1, planes, pstride;
  double sx, sy, vx, vy, lw;
  const double* trig;
  const double* arcs;    // sf_arc_table: the rings' 84 arcs
  const double* circle;  // the circle's K curves (sft::ArcK each)
  int circle_k;
  __device__ __forceinline__ sftd::Ctx tc() const { return sftd::Ctx{tor, fb, W, H, tid, sftd::kMaxQuadsBig}; }
  __device__ __forceinline__ sftd::Band band(unsigned rgb, unsigned seams = 0u) const {
    return sftd::Band{r0, r1, planes, pstride, rgb, seams};
  }
  __device__ __forceinline__ static void order() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  // does [y0, y1) (24.8 fixed, device space) reach into the band's rows
  __device__ __forceinline__ bool meets(double dy0, double dy1) const { return dy1 >= (double)r0 - 1.0 && dy0 <= (double)r1 + 1.0; }
  // one pixel of the band, every plane: lerp8 to grey (the same value in B, G, R) or to rgb's bytes
  __device__ __forceinline__ void put(int px, int py, int al, unsigned rgb, int grey) const {
    uint8_t* p = fb + (py - r0) * W + px;
    if (planes == 1) *p = (uint8_t)sft::lerp8(grey, al, *p);
    else
      for (int c = 0; c < 3; c++) p[c * pstride] = (uint8_t)sft::lerp8((int)((rgb >> (8 * c)) & 255u), al, p[c * pstride]);
  }
  // drawWireFrame (SRC/draw.cpp:82-100): one cairo_stroke of the wireframe's lines
  __device__ void wireframe(int kind, int deg, double px, double py) const {
    // every stroke of a wireframe lies within 36 + lw user units of its position
    const double ext = 37.0 + lw;
    if (!meets((py - ext - vy) * sy, (py + ext - vy) * sy)) return;
    deg = deg < 0 ? 0 : (deg > 359 ? 359 : deg);
    const int n = (kind == 0 || kind == 2) ? 3 : 4;
    const unsigned rgb = kind == 2 ? kWhite : (kind == 3 ? kRed : kYellow);
    const sft::Affine v = sft::view_matrix(sx, sy, vx, vy);
    const double2 cs = *reinterpret_cast<const double2*>(trig + 2 * deg);
    const sft::Affine m = sft::object_matrix(v, px, py, cs.x, cs.y);
    if (kind == 1 && m.xy == 0.0 && m.yx == 0.0) {
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
    sftd::raster<4, true>(tc(), q, tid < n, 0, kind == 1 ? sftd::kKindFort : (kind == 3 ? sftd::kKindShell : sftd::kKindLines3), 255,
                          band(rgb));
  }
  // the fortress at heading 0: cairo's rectilinear stroker, boxes of exact area (sf_render_generic.hip: fort_boxes)
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
    const int px0 = max(X0 >> 8, 0), py0 = max(Y0 >> 8, r0), px1 = min((X1 + 255) >> 8, W), py1 = min((Y1 + 255) >> 8, r1);
    const int bw = px1 - px0, n = bw > 0 && py1 > py0 ? bw * (py1 - py0) : 0;
    for (int i = tid; i < n; i += 64) {
      const int ry = i / bw, px = px0 + (i - ry * bw), py = py0 + ry;
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
    order();
  }
  // drawExplosion (SRC/draw.cpp:116-145): 7 rings of twelve 10-degree arcs (one Bezier segment each at up to 1.0 pixel per
  // unit), each its own stroke, four arcs of up to four pieces per call; then the radius-7 circle: K curves, 32 / K lanes each
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
        sftd::raster<4, true>(tc(), q, valid, tid & ~3, sftd::kKindSingle, yellow ? 191 : 128, band(yellow ? kYellow : kRed));
      }
    }
    if (!meets((cy - 8.0 - lw - vy) * sy, (cy + 8.0 + lw - vy) * sy)) return;
    const int K = circle_k, per = 32 / K, cap = per + 1;
    sft::Quad q = {};
    bool valid = false;
    int n = 0;
    {
      int px[17], py[17], tx[17], ty[17];
      const int c = min(tid / per, K - 1);
      const double* kp = circle + 8 * c;
      n = sft::flatten_faces(sft::arc_knots(v, cx, cy, sft::ArcK{kp[0], kp[1], kp[2], kp[3], kp[4], kp[5], kp[6], kp[7]}), px, py, tx, ty, cap);
      const int p = tid - c * per;
      if (tid < 32 && p < n - 1) {
        valid = true;
        q = sft::faces_quad(px[p], py[p], tx[p], ty[p], px[p + 1], py[p + 1], tx[p + 1], ty[p + 1], sx, sy, hw);
      }
    }
    // the first piece of curves 1 .. K - 1 (pieces are numbered over the valid lanes, curve after curve)
    unsigned seams = (unsigned)K;
    int first = 0;
    for (int c = 0; c < K; c++) {
      if (c > 0) seams |= (unsigned)first << (8 + 6 * (c - 1));
      first += __builtin_amdgcn_readlane(n, c * per) - 1;
    }
    sftd::raster<8, true>(tc(), q, valid, 0, sftd::kKindRing, 191, band(kYellow, seams));
  }
  // drawScore (SRC/draw.cpp:161-173): grey .5 through the view's glyph atlas, or the seven-segment fallback (sf_raster.h)
  __device__ void score(int pnts, const SfGlyphAtlas* G) const {
    if (G && G->gw) {
      const uint32_t chars = sfg::score_chars(pnts);
      const int bx0 = max((int)G->x_min, 0), bx1 = min((int)G->x_max + 6 * G->advance + G->gw, W);
      const int by0 = max(G->y0, r0), by1 = min(G->y0 + G->gh, r1);
      const int bw = bx1 - bx0, n = bw > 0 && by1 > by0 ? bw * (by1 - by0) : 0;
      for (int i = tid; i < n; i += 64) {
        const int ry = i / bw, px = bx0 + (i - ry * bw), py = by0 + ry;
        uint8_t* p = fb + (py - r0) * W + px;
        for (int c = 0; c < planes; c++) p[c * pstride] = (uint8_t)sfg::text_pixel(G, chars, px, py, p[c * pstride]);
      }
      order();
      return;
    }
    const unsigned long long masks = sfr::score_masks(pnts);
    auto dx = [&](double x) { return (x - vx) * sx; };
    auto dy = [&](double y) { return (y - vy) * sy; };
    const double Wg = SF_TXT_W, Hg = SF_TXT_H, T = SF_TXT_T, m0 = 0.5 * (SF_TXT_H - SF_TXT_T), m1 = 0.5 * (SF_TXT_H + SF_TXT_T);
    const double sx0[7] = {0, Wg - T, Wg - T, 0, 0, 0, 0}, sx1[7] = {Wg, Wg, Wg, Wg, T, T, Wg};
    const double sy0[7] = {0, T, m1, Hg - T, m1, T, m0}, sy1[7] = {T, m0, Hg - T, Hg, Hg - T, m0, m1};
    const double tx0 = dx((double)SF_TXT_X0 + SF_TXT_PAD), tx1 = dx((double)SF_TXT_X0 + 6.0 * SF_TXT_ADV + SF_TXT_PAD + SF_TXT_W);
    const double ty0 = dy((double)SF_TXT_TOP), ty1 = dy((double)SF_TXT_TOP + SF_TXT_H);
    const int bx0 = max((int)floor(tx0), 0), by0 = max((int)floor(ty0), r0), bx1 = min((int)ceil(tx1), W), by1 = min((int)ceil(ty1), r1);
    const int bw = bx1 - bx0, n = bw > 0 && by1 > by0 ? bw * (by1 - by0) : 0;
    for (int i = tid; i < n; i += 64) {
      const int ry = i / bw, px = bx0 + (i - ry * bw), py = by0 + ry;
      const double fpx = (double)px, fpy = (double)py;
      for (int c = 0; c < planes; c++) {
        uint8_t* p = fb + (py - r0) * W + px + c * pstride;
        int d = *p;
        for (int cell = 0; cell < 7; cell++) {
          const double gx = (double)SF_TXT_X0 + (double)SF_TXT_ADV * (double)cell + SF_TXT_PAD, gy = SF_TXT_TOP;
          const unsigned bits = (unsigned)(masks >> (7 * cell)) & 0x7Fu;
          for (int seg = 0; seg < 7; seg++) {
            if (!((bits >> seg) & 1u)) continue;
            const double ox = fmin(dx(gx + sx1[seg]), fpx + 1.0) - fmax(dx(gx + sx0[seg]), fpx);
            const double oy = fmin(dy(gy + sy1[seg]), fpy + 1.0) - fmax(dy(gy + sy0[seg]), fpy);
            if (ox > 0.0 && oy > 0.0) {
              const int mm = (int)(fmin(ox * oy, 1.0) * 255.0 + 0.5);
              if (mm > 0) d = sfr::over_un8(d, 128, mm);
            }
          }
        }
        *p = (uint8_t)d;
      }
    }
    order();
  }
  // drawVlner (SRC/draw.cpp:207-225): cairo_rectangle + cairo_fill through the box converter, grey in both modes
  __device__ void rect(double x, double y, double w, double h, int grey) const {
    const sft::Affine v = sft::view_matrix(sx, sy, vx, vy);
    int x0, y0;
    sft::to_device(v, x, y, &x0, &y0);
    int x1 = x0 + sft::fx_from_double(v.xx * w + v.xy * 0.0), y1 = y0 + sft::fx_from_double(v.yx * 0.0 + v.yy * h);
    if (x1 < x0) { const int t = x0; x0 = x1; x1 = t; }
    if (y1 < y0) { const int t = y0; y0 = y1; y1 = t; }
    const int px0 = max(x0 >> 8, 0), py0 = max(y0 >> 8, r0), px1 = min((x1 + 255) >> 8, W), py1 = min((y1 + 255) >> 8, r1);
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
    order();
  }
};

}  // namespace

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
  const Ctx C{v_fb, torw, W, a.H, tid, r0, r1, a.planes, plane, a.sx, a.sy, a.vx, a.vy, a.lw, a.trig, a.arcs, a.circle, a.circle_k};
  for (int i = tid; i < sftd::kLdsWordsBig; i += 64) torw[i] = 0u;
  const unsigned char* tile = a.state + (long)(lane >> 6) * sfl::kTileBytes;
  const int l = lane & 63, o16 = l * 16;
  const d2_t sp = V_LD(d2_t, V_CHUNK(ship_pos, 0), o16);
  const i4_t tb = V_LD(i4_t, V_CHUNK(timers_b, 0), o16);
  const i4_t sc = V_LD(i4_t, V_CHUNK(score, 0), o16);
  const i4_t mi = V_LD(i4_t, V_CHUNK(misc, 0), o16);
  const i4_t sm = V_LD(i4_t, V_CHUNK(small, 0), o16);
  const int ship_angle = (int)(int16_t)(sm.x & 0xFFFF), fort_angle = (int)(int16_t)((unsigned)sm.x >> 16);
  const unsigned flags = ((unsigned)sm.y >> 16) & 0xFFu;
  const unsigned mmask = (unsigned)mi.z & SF_MASK_LOW, smask = (unsigned)mi.w & SF_MASK_LOW, n_pool = (unsigned)mi.z >> SF_MPOOL_SHIFT;
  const int pnts = (int)__int_as_float(sc.x), vlner = sc.z & 0xFFF;
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
  for (int s = tid; s < SF_NSLOT; s += 64) mtab[s][0] = mtab[s][1] = mtab[s][2] = 0.0;
  __syncthreads();
  for (unsigned e = tid; e < n_pool; e += 64) {
    const unsigned meta = V_LD(uint32_t, V_CHUNK(missile_meta, 0), e * 4u);
    if (SF_MM_OWNER(meta) == (unsigned)l) {
      const d2_t m = V_LD(d2_t, V_CHUNK(missile_pos, 0), e * 16u);
      double* t = mtab[SF_MM_SLOT(meta)];
      t[0] = m.x;
      t[1] = m.y;
      t[2] = (double)SF_MM_ANGLE(meta);
    }
  }
  __syncthreads();
  // SRC/draw.cpp:233-268, in order
  if (flags & SF_FL_SHIP_ALIVE) C.wireframe(0, ship_angle, sp.x, sp.y);
  else C.explosion(sp.x, sp.y);
  if (flags & SF_FL_FORT_ALIVE) C.wireframe(1, fort_angle, sfc::fort_x, sfc::fort_y);
  else C.explosion(sfc::fort_x, sfc::fort_y);
  for (int s = 0; s < SF_NSLOT; s++)
    if ((mmask >> s) & 1u) C.wireframe(2, (int)mtab[s][2], mtab[s][0], mtab[s][1]);
  for (int s = 0; s < SF_NSLOT; s++)
    if ((smask >> s) & 1u) {
      const d2_t p = V_LD(d2_t, V_CHUNK(shell_pos, s), o16), v = V_LD(d2_t, V_CHUNK(shell_vel, s), o16);
      const double ddx = p.x - sfc::fort_x, ddy = p.y - sfc::fort_y;
      if (sqrt(ddx * ddx + ddy * ddy) > 21.0) {
        double ang = atan2(v.y, v.x) * 180.0 / M_PI;
        if (ang < 0) ang += 360.0;
        C.wireframe(3, (int)ang, p.x, p.y);
      }
    }
  C.score(pnts, a.glyphs);
  {
    const bool kill = vlner > 10 && tb.w < sfc::vuln_time;
    C.rect(355.0 - 100, 335.0 + 187, 200.0, 10.0, 84);
    if (vlner > 0) C.rect(355.0 - 100, 335.0 + 187, (double)(20 * (vlner > 10 ? 10 : vlner)), 10.0, kill ? 255 : 168);
  }
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
