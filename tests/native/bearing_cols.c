/* Host restatement of the observation's bearing columns as the kernels compute them (sf_lane_dev.h): sf_atan2_core with the
 * table step, sf_atan2<true> with both exact forms (near-axis, exact-degree), rad2deg through sf_div_const, compute_extras
 * (aim; vdir with its derived first angle and the two wraps; ndist) and what the three observation writers make of them
 * (features, normalized-features with Python's % and the clamps, monitors; the float32 forms are a plain (float)).  Operation
 * for operation, FMAs where the kernels have them, as atan2_core.c does it; v_rcp_f64 is modelled as the reciprocal rounded
 * to FLOAT, a worse seed than the instruction's.  `libm` as the first argument: the form of a new game's row, with the C
 * library's atan2 in place of the core (the exact forms stay).
 *
 * One switch per mutant, for the test that the bounds notice them (tests/test_bearing_columns_model.py):
 *   -DMUT_NO_SEVENTH   the series without its 1/7 term
 *   -DMUT_PI_LO        the near-axis form without the low parts of pi and pi/2
 *   -DMUT_VDIR_SIGN    M_PI - a_pos with the wrong sign where dy < 0: -(M_PI - a_pos) for -M_PI - a_pos
 *
 * reads rows of five doubles (sx, sy, vx, vy, angle) from the file argv[2], writes rows of NOUT doubles to argv[3].
 * gcc -O2 -ffp-contract=off -I spacefortress_amd/csrc bearing_cols.c -lm */
#define _GNU_SOURCE
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define __device__
#include "sf_deg_dd.h"

#define NOUT 22
static const double fort_x = 355, fort_y = 315, ndist_a = 40, ndist_b = (200 - 40) / 2.0;
static double atab[17];
static int use_libm;

static double div_const(double a, double c, double rc) {
  const double q = a * rc;
  const double rem = fma(-c, q, a);
  return fma(rem, rc, q);
}
#define DIV(a, C) div_const((a), (double)(C), 1.0 / (double)(C))
static double rad2deg(double a) { return DIV(a, M_PI) * 180; }

static double recip(double d) {
  double r = (double)(float)(1.0 / d);
  r = fma(fma(-d, r, 1.0), r, r);
  return fma(fma(-d, r, 1.0), r, r);
}
static double core(double y, double x) {
  const double ax = fabs(x), ay = fabs(y);
  const double u = fmax(ax, ay), v = fmin(ax, ay);
  const double ru = recip(u);
  double q = v * ru;
  q = fma(fma(-u, q, v), ru, q);
  const double k = rint(q * 16.0), c = k * 0.0625;
  const double den = fma(q, c, 1.0), num = q - c;
  const double rd = recip(den);
  double t = num * rd;
  t = fma(fma(-den, t, num), rd, t);
  const double s = t * t;
#ifdef MUT_NO_SEVENTH
  double p = s * (1.0 / 9.0);
#else
  double p = fma(s, 1.0 / 9.0, -1.0 / 7.0);
#endif
  p = fma(s, p, 0.2);
  p = fma(s, p, -1.0 / 3.0);
  double a = atab[k == k ? (int)k : 0] + fma(t, p * s, t); /* (0, 0) gives a NaN, which its caller discards; the host must not index with it */
  a = ay > ax ? 1.5707963267948966 - a : a;
  a = x < 0 ? 3.141592653589793 - a : a;
  return copysign(a, y);
}

/* sf_atan2<RAZOR>(y, x, atab or nullptr); form: 0 core / libm, 1 near-axis, 2 exact-degree */
static double sf_atan2(int razor, int with_core, double y, double x, int* form) {
  double r = with_core ? core(y, x) : atan2(y, x);
  const double ax = fabs(x), ay = fabs(y);
  const int ny = ax * 0x1p27 < ay;
  const int nx = (x < 0) & (ay * 0x1p27 < ax);
  *form = 0;
  if (ny | nx) {
    const double t = ny ? x / y : y / x;
    const double hi = ny ? 1.5707963267948966 : 3.141592653589793;
#ifdef MUT_PI_LO
    const double lo = 0.0;
#else
    const double lo = ny ? 6.123233995736766e-17 : 1.2246467991473532e-16;
#endif
    r = copysign(hi, y) + (ny ? copysign(lo, y) - t : copysign(lo, y) + t);
    *form = 1;
  }
  if (razor) {
    const double deg = DIV(fabs(r), M_PI) * 180, kd = rint(deg);
    const int rz = !(ny | nx) & (fabs(deg - kd) < 1e-9) & (y != 0.0);
    if (rz) {
      const double* e = kDegDD[(int)kd];
      const double ph = e[0], pl = e[1], ch = e[2], cl = e[3], sh = e[4], sl = e[5];
      const double p1 = ay * ch, e1 = fma(ay, ch, -p1);
      const double p2 = x * sh, e2 = fma(x, sh, -p2);
      const double d = p1 - p2;
      const double bb = d - p1, err = (p1 - (d - bb)) + (-p2 - bb);
      const double lo = err + (e1 - e2) + (ay * cl - x * sl);
      const double N = d + lo, D = x * ch + ay * sh;
      r = copysign(ph + (pl + N / D), y);
      *form = 2;
    }
  }
  return r;
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  use_libm = strcmp(argv[1], "libm") == 0;
  for (int k = 0; k <= 16; k++) atab[k] = atan(k / 16.0); /* (sf_host_fill_consts) */
  FILE* in = fopen(argv[2], "rb");
  FILE* out = fopen(argv[3], "wb");
  if (!in || !out) return 2;
  double row[5], o[NOUT];
  while (fread(row, sizeof(double), 5, in) == 5) {
    const double sx = row[0], sy = row[1], vx = row[2], vy = row[3], angle = row[4];
    int form, f2;
    /* the step kernel: a_pos = sf_atan2<true>(.., atab), a_vel = sf_atan2_core; a new game: sf_atan2<true>(..), sf_atan2<false>(..) */
    const double a_pos = sf_atan2(1, !use_libm, sy - fort_y, sx - fort_x, &form);
    const double a_vel = use_libm ? sf_atan2(0, 0, vy, vx, &f2) : core(vy, vx);
    /* compute_extras */
    double aim = rad2deg(a_pos) - angle + 180;
    if (aim < -180) aim = aim + 360;
    const double dy = sy - fort_y;
    double ov;
    if (dy == 0)
      ov = sf_atan2(0, 0, -(fort_y - sy), fort_x - sx, &f2);
    else
#ifdef MUT_VDIR_SIGN
      ov = dy < 0 ? -(M_PI - a_pos) : (M_PI - a_pos);
#else
      ov = dy < 0 ? (-M_PI - a_pos) : (M_PI - a_pos);
#endif
    double diff = a_vel - ov;
    if (diff > M_PI) diff -= M_PI * 2;
    if (diff < -M_PI) diff += M_PI * 2;
    const double vdir = (vx * vx + vy * vy == 0.0) ? 0.0 : rad2deg(diff);
    const double fdist = fabs(sx - fort_x);
    const double ndist = -1 + DIV(fdist - ndist_a, ndist_b);
    /* write_obs: normalized-features */
    double n6 = DIV(aim, 180), n7, n8 = ndist;
    {
      double m = fmod(vdir, 360.0);
      if (m != 0) {
        if (m < 0) m += 360.0;
      } else {
        m = 0.0;
      }
      n7 = DIV(m, 360);
    }
    n6 = n6 < -1 ? -1 : (n6 > 1 ? 1 : n6);
    n7 = n7 < -1 ? -1 : (n7 > 1 ? 1 : n7);
    n8 = n8 < -1 ? -1 : (n8 > 1 ? 1 : n8);
    o[0] = a_pos; o[1] = a_vel; o[2] = aim; o[3] = vdir; o[4] = ndist; o[5] = n6; o[6] = n7; o[7] = n8;
    /* monitors */
    o[8] = aim < 3 ? 0.5 : -0.5; o[9] = aim > 3 ? 0.5 : -0.5;
    o[10] = ndist > .75 ? 0.5 : -0.5; o[11] = ndist > .25 ? 0.5 : -0.5;
    o[12] = ndist < -.25 ? 0.5 : -0.5; o[13] = ndist < -.75 ? 0.5 : -0.5;
    /* the float32 batches: (T)v */
    o[14] = (float)aim; o[15] = (float)vdir; o[16] = (float)ndist; o[17] = (float)n6; o[18] = (float)n7; o[19] = (float)n8;
    o[20] = form; o[21] = ov;
    fwrite(o, sizeof(double), NOUT, out);
  }
  fclose(in);
  return fclose(out) != 0;
}
