// sf_view_host.cpp -- the host side of sf_render_view (include/sfmi.h): a view's defaults, limits and tables.  No HIP calls:
// sf_view_check and sf_view_circle_segments work without a GPU (tests/test_view_host.py).
#include <math.h>
#include <string.h>

#include <vector>

#include "sf_internal.h"
#include "sf_tor.h"
#include "sf_view.h"

namespace {

constexpr int kMaxSide = 1024;
// a band's planes: at most 48 KiB of LDS; with the kernel's 5 856 static bytes a workgroup holds at most 55 008, so a CU of
// 160 KiB runs two of the widest colour bands (1 024 pixels, 16 rows) and more of every narrower one
constexpr size_t kBandBytes = 49152;

// cairo-arc.c: _arc_max_angle_for_tolerance_normalized's table (oracle/cairo_model.c: arc_max_angle)
double arc_max_angle(double tolerance) {
  static const struct {
    double angle, error;
  } table[] = {
      {M_PI / 1.0, 0.0185185185185185036127},   {M_PI / 2.0, 0.000272567143730179811158},
      {M_PI / 3.0, 2.38647043651461047433e-05}, {M_PI / 4.0, 4.2455377443222443279e-06},
      {M_PI / 5.0, 1.11281001494389081528e-06}, {M_PI / 6.0, 3.72662000942734705475e-07},
      {M_PI / 7.0, 1.47783685574284411325e-07}, {M_PI / 8.0, 6.63240432022601149057e-08},
      {M_PI / 9.0, 3.2715520137536980553e-08},  {M_PI / 10.0, 1.73863223499021216974e-08},
      {M_PI / 11.0, 9.81410988043554039085e-09},
  };
  for (int i = 0; i < 11; i++)
    if (table[i].error < tolerance) return table[i].angle;
  return M_PI / 12.0;
}

// the largest number of faces (pieces + 1) cairo's flattening gives an arc of the view: its centre at every 1/64 pixel of a
// pixel (the knots are rounded to 1/256 pixel, so the pieces depend on where the centre falls), uncapped
int max_faces(const SfViewRes& r, const sft::ArcK& k) {
  const sft::Affine v = sft::view_matrix(r.sx, r.sy, r.vx, r.vy);
  int most = 0;
  for (int i = 0; i < 64 * 64; i++) {
    int px[64], py[64], tx[64], ty[64];
    const double cx = 355.0 + (i & 63) / (64.0 * r.sx), cy = 315.0 + (i >> 6) / (64.0 * r.sy);
    const int n = sft::flatten_faces(sft::arc_knots(v, cx, cy, k), px, py, tx, ty, 64);
    most = n > most ? n : most;
  }
  return most;
}

}  // namespace

extern "C" int sf_view_circle_segments(double xx, double yx, double xy, double yy, double radius) {
  // _cairo_arc_segments_needed(angle pi, radius, ctm, tolerance 0.1): the major axis of the transformed circle
  // (_cairo_matrix_transformed_circle_major_axis), the largest table angle within tolerance / major axis
  if (!(radius > 0)) {
    sf_set_error("sf_view_circle_segments: radius must be positive");
    return SF_ERR_ARG;
  }
  const double i = xx * xx + yx * yx, j = xy * xy + yy * yy;
  const double f = 0.5 * (i + j), g = 0.5 * (i - j), h = xx * xy + yx * yy;
  const double major = (fabs(h) == 0 && fabs(g) == 0) ? radius * sqrt(f) : radius * sqrt(f + hypot(g, h));
  const double max_angle = arc_max_angle(0.1 / major);
  return (int)ceil(fabs(M_PI) / max_angle);
}

int sf_view_resolve(const sf_view* v, int cfg_w, int cfg_h, SfViewRes* r) {
  if (!v || !r) {
    sf_set_error("sf_view: null view");
    return SF_ERR_ARG;
  }
  memset(r, 0, sizeof(*r));
  // the reference's defaulting (SRC/pymodule.cpp:345-349): viewport size -1 -> the config's, surface -1 -> the viewport's
  const double vw = v->vp_w == -1 ? (double)cfg_w : v->vp_w, vh = v->vp_h == -1 ? (double)cfg_h : v->vp_h;
  if (!(vw > 0) || !(vh > 0) || !(vw < 1e6) || !(vh < 1e6) || !isfinite(v->vp_x) || !isfinite(v->vp_y)) {
    sf_set_error("sf_view: the viewport (%g, %g, %g, %g) needs a positive width and height (-1: the config's)", v->vp_x, v->vp_y,
                 v->vp_w, v->vp_h);
    return SF_ERR_ARG;
  }
  if (!(v->line_width > 0) || !isfinite(v->line_width)) {
    sf_set_error("sf_view: line width %g must be positive", v->line_width);
    return SF_ERR_ARG;
  }
  const int w = v->width == -1 ? (int)vw : v->width, h = v->height == -1 ? (int)vh : v->height;
  if (w < 1 || h < 1 || w > kMaxSide || h > kMaxSide) {
    sf_set_error("sf_view: a %d x %d surface: each side must lie in [1, %d] (-1: the viewport's size)", w, h, kMaxSide);
    return SF_ERR_ARG;
  }
  r->w = w;
  r->h = h;
  r->sx = (double)w / vw;
  r->sy = (double)h / vh;
  if (!(r->sx <= 1.0) || !(r->sy <= 1.0)) {
    sf_set_error("sf_view: %d x %d pixels for a %g x %g viewport is more than 1.0 pixel per user unit", w, h, vw, vh);
    return SF_ERR_ARG;
  }
  r->vx = v->vp_x;
  r->vy = v->vp_y;
  r->lw = v->line_width;
  r->planes = v->grayscale ? 1 : 3;
  r->format = v->format;
  if (r->format != SF_VIEW_BGRX && r->format != SF_VIEW_RGB && r->format != SF_VIEW_GRAY) {
    sf_set_error("sf_view: format %d is none of SF_VIEW_BGRX, SF_VIEW_RGB, SF_VIEW_GRAY", v->format);
    return SF_ERR_ARG;
  }
  if (r->format == SF_VIEW_GRAY && !v->grayscale) {
    sf_set_error("sf_view: SF_VIEW_GRAY is for grey views (grayscale = 1)");
    return SF_ERR_ARG;
  }
  // the circle: one or two Bezier segments per half (up to 1.0 pixel per unit), 32 lanes of pieces between its curves
  const int seg = sf_view_circle_segments(r->sx, 0.0, 0.0, r->sy, 7.0);
  if (seg < 1 || seg > 2) {
    sf_set_error("sf_view: the explosion's circle takes %d segments per half here", seg);
    return SF_ERR_ARG;
  }
  r->circle_k = 2 * seg;
  // rows per workgroup: W * band_h a whole number of 16-byte pieces, at most 32 rows (the rasteriser's row masks), the planes
  // within kBandBytes
  int m = 16;  // the smallest m with w * m a multiple of 16
  for (int c = 1; c <= 16; c <<= 1)
    if ((w * c) % 16 == 0) { m = c; break; }
  int bh = (int)(kBandBytes / ((size_t)r->planes * w));
  bh = bh > 32 ? 32 : bh;
  bh -= bh % m;
  r->band_h = bh < m ? m : bh;
  // the score text: the caller's atlas; or the built-in one of 1.0 pixel per unit at a whole viewport offset; or the fallback
  if (v->glyphs) {
    const int rc = sf_glyphs_pack(v->glyphs, v->glyph_alpha, nullptr, &r->glyphs);
    if (rc != SF_OK) return rc;
  } else if (r->sx == 1.0 && r->sy == 1.0 && r->vx == floor(r->vx) && r->vy == floor(r->vy) && fabs(r->vx) < 16384 && fabs(r->vy) < 16384) {
    SfGlyphAtlas& G = r->glyphs;
    const int ox = (int)r->vx, oy = (int)r->vy;
    G.gw = sfg::kUnitW;
    G.gh = sfg::kUnitH;
    G.advance = sfg::kUnitAdvance;
    G.y0 = sfg::kUnitY0 - oy;
    int lo = 32767, hi = -32768;
    for (int i = 0; i < SF_GLYPH_CHARS * 10; i++) {
      const int x = sfg::kUnitX0[i / 10][i % 10] - ox;
      G.x0[i] = (int16_t)x;
      lo = x < lo ? x : lo;
      hi = x > hi ? x : hi;
    }
    G.x_min = (int16_t)lo;
    G.x_max = (int16_t)hi;
    memcpy(G.alpha, sfg::kUnitAlpha, sizeof(sfg::kUnitAlpha));
  }
  return SF_OK;
}

int sf_view_tables(const SfViewRes& r, std::vector<uint8_t>* bg, size_t* bg_stride, std::vector<double>* circle) {
  // what the kernel's lanes hold: an explosion arc in up to four pieces (five faces), a curve of the circle in 32 / K (the
  // kernel's flatten_faces stops at that cap and would drop the rest silently).  The bound is tight: over the scales up to 1.0
  // the worst placement takes the cap exactly -- 17 faces of 17 for K = 2 (0.70 .. 0.77 pixels per unit), 9 of 9 for K = 4
  // (0.78 .. 1.0) --, the 10-degree arcs 3 of 5.  Checked here, once per view, over every 1/64-pixel placement of the centre.
  {
    const double kPi = 3.14159265358979323846;
    const int seg_k = r.circle_k / 2;
    for (int half = 0; half < 2; half++) {
      double amin = half == 0 ? 0.0 : 0.0 + (2 * kPi - 0.0) / 2.0, amax = half == 0 ? 0.0 + (2 * kPi - 0.0) / 2.0 : 2 * kPi;
      const double step = (amax - amin) / seg_k;
      for (int i = 0; i < seg_k; i++, amin += step) {
        const sft::ArcK k = sft::arc_k(7.0, amin, i == seg_k - 1 ? amax : amin + step);
        if (max_faces(r, k) > 32 / r.circle_k + 1) {
          sf_set_error("sf_view: the explosion's circle is flattened into more pieces than the renderer holds");
          return SF_ERR_ARG;
        }
      }
    }
    const sft::ArcK outer = sft::arc_k(63.0, 3 * 7 * kPi / 180, (3 * 7 + 10) * kPi / 180);
    if (max_faces(r, outer) > 5) {
      sf_set_error("sf_view: the explosion's arcs are flattened into more pieces than the renderer holds");
      return SF_ERR_ARG;
    }
  }
  std::vector<uint8_t> full((size_t)r.w * r.h);
  const int rc = sf_image_background_geom(r.w, r.h, r.vx, r.vy, r.w / r.sx, r.h / r.sy, r.lw, full.data());
  if (rc != SF_OK) return rc;
  const int n_bands = (r.h + r.band_h - 1) / r.band_h;
  *bg_stride = (size_t)r.w * r.band_h;
  bg->assign((size_t)n_bands * *bg_stride, 0);
  for (int b = 0; b < n_bands; b++) {
    const int r0 = b * r.band_h, r1 = r0 + r.band_h < r.h ? r0 + r.band_h : r.h;
    memcpy(bg->data() + (size_t)b * *bg_stride, full.data() + (size_t)r0 * r.w, (size_t)(r1 - r0) * r.w);
  }
  // cairo_arc(x, y, 7, 0, 2 pi): two halves (_cairo_arc_in_direction), each cut into circle_k / 2 segments of equal angle
  // (amin advances by the step; the last segment ends on the half's end)
  circle->clear();
  const double kPi = 3.14159265358979323846;
  const int seg_k = r.circle_k / 2;
  for (int half = 0; half < 2; half++) {
    double amin = half == 0 ? 0.0 : 0.0 + (2 * kPi - 0.0) / 2.0, amax = half == 0 ? 0.0 + (2 * kPi - 0.0) / 2.0 : 2 * kPi;
    const double step = (amax - amin) / seg_k;
    for (int i = 0; i < seg_k; i++, amin += step) {
      const sft::ArcK k = sft::arc_k(7.0, amin, i == seg_k - 1 ? amax : amin + step);
      const double v[8] = {k.rca, k.rsa, k.hrsa, k.hrca, k.rcb, k.rsb, k.hrsb, k.hrcb};
      circle->insert(circle->end(), v, v + 8);
    }
  }
  return SF_OK;
}

extern "C" int sf_view_check(const sf_view* view, int32_t* width, int32_t* height) {
  SfViewRes r;
  const int rc = sf_view_resolve(view, 710, 626, &r);  // (every config's playfield is 710 x 626, SRC/configs.cpp)
  if (rc != SF_OK) return rc;
  if (width) *width = r.w;
  if (height) *height = r.h;
  return SF_OK;
}
