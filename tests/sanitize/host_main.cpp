// Host-only entry points of libsfmi (sf_host.cpp, sf_image.cpp: no HIP calls) under -fsanitize=address,undefined
// (tests/test_sanitizers.py).  GPU sanitizers are not available on the pool; these are the CPU-side ones.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "sf_internal.h"
#include "sf_raster.h"
#include "sfmi.h"

// sf_field_values_fit on 3 envs, the value under test in the last one (the others 0): accepted?
static bool fits1(int field, int count, int elem, int idx, long value) {
  const long n = 3;
  std::vector<int32_t> v32(count * n, 0);
  std::vector<int16_t> v16(count * n, 0);
  if (elem == 2) v16[idx * n + n - 1] = (int16_t)value; else v32[idx * n + n - 1] = (int32_t)value;
  return sf_field_values_fit(field, elem == 2 ? (const void*)v16.data() : (const void*)v32.data(), n) == SF_OK;
}
static bool refused_naming(bool accepted, const char* what) { return !accepted && strstr(sf_last_error(), what) != nullptr; }

// the host-only logic behind sf_create, sf_set_image_geometry and sf_set_field (sf_internal.h); 0 or a distinct exit code
static int host_logic() {
  {  // the default geometry's taps: 84 columns of a 90-wide, then 84 rows of a 92-high surface, 4 words each, `first` in front
    uint32_t tabs[SF_TAB_WORDS];
    if (sf_area_tabs_default(tabs)) return 20;
    for (int i = 0; i < 84; i++)
      if ((int32_t)tabs[4 * i] < 0 || (int32_t)tabs[4 * i] >= 90 || (int32_t)tabs[4 * (84 + i)] < 0 || (int32_t)tabs[4 * (84 + i)] >= 92) return 21;
  }
  const int geoms[3][2] = {{112, 115}, {84, 84}, {251, 195}};  // (the smallest surface; a largest one under the 49 152-pixel cap)
  for (const int* g : geoms) {  // 8 words per destination: first, count, ...
    uint32_t tabs[16 * 84];
    if (sf_area_tabs_geom(g[0], g[1], tabs)) return 22;
    for (int ax = 0; ax < 2; ax++)
      for (int i = 0; i < 84; i++) {
        const int32_t first = (int32_t)tabs[8 * (ax * 84 + i)], count = (int32_t)tabs[8 * (ax * 84 + i) + 1];
        if (first < 0 || count < 1 || first + count > g[ax]) return 23;
      }
  }
  for (const char* name : {"youturn", "autoturn", "test-youturn", "test-autoturn"}) {
    sf_preset p;
    std::vector<double> consts(SF_CONST_DOUBLES);
    if (sf_preset_get(name, &p)) return 24;
    sf_host_fill_consts(p, consts.data());
    if (!sf_preset_compiled_in(p, consts.data())) return 25;
    sf_preset q = p;
    q.missile_speed += 1;
    if (sf_preset_compiled_in(q, consts.data())) return 26;
    q = p;
    q.big_hex = 201;
    if (sf_preset_compiled_in(q, consts.data())) return 27;
    consts[SF_LDS_SMALLHEX + 5] += 1.0;  // one hex-edge double
    if (sf_preset_compiled_in(p, consts.data())) return 28;
  }
  // the packed words of sf_layout.h's table, as literals: {field, bits, signed}
  const struct { int field, bits, sgn; } bf[] = {
      {SF_F_prev_vlner, 12, 0}, {SF_F_fire_timer, 16, 1}, {SF_F_thrust_timer, 16, 1}, {SF_F_left_timer, 16, 1},
      {SF_F_right_timer, 16, 1}, {SF_F_vlner, 12, 0}, {SF_F_time, 24, 0}, {SF_F_spawn_cursor, 24, 0},
      {SF_F_missile_mask, 20, 0}, {SF_F_shell_mask, 20, 0}, {SF_F_ep_kills, 8, 0}};
  for (const auto& f : bf) {
    if (f.sgn) {
      const long lo = -(1l << (f.bits - 1)), hi = (1l << (f.bits - 1)) - 1;
      if (!fits1(f.field, 1, 4, 0, lo) || !fits1(f.field, 1, 4, 0, hi)) return 30;
      if (!refused_naming(fits1(f.field, 1, 4, 0, lo - 1), "env 2") || !refused_naming(fits1(f.field, 1, 4, 0, hi + 1), "env 2")) return 31;
    } else {
      if (!fits1(f.field, 1, 4, 0, (1l << f.bits) - 1) || !fits1(f.field, 1, 4, 0, 0)) return 32;
      if (!refused_naming(fits1(f.field, 1, 4, 0, 1l << f.bits), "env 2") || !refused_naming(fits1(f.field, 1, 4, 0, -1), "env 2")) return 33;
    }
  }
  {  // stats [13][3]: every counter at its maximum in the last env, ship deaths (stats[3], 10 bits) = 3 * 255 = 765
    const int bits[13] = {8, 8, 8, 10, 16, 8, 16, 16, 16, 16, 16, 12, 12};
    const long n = 3;
    std::vector<int32_t> top(13 * n, 0);
    for (int k = 0; k < 13; k++) top[k * n + 2] = k == 3 ? 765 : (1 << bits[k]) - 1;
    if (sf_field_values_fit(SF_F_stats, top.data(), n)) return 34;
    for (int k = 0; k < 13; k++) {  // one over: the three deaths take the sum along, so that only the width can refuse
      std::vector<int32_t> v = top;
      v[k * n + 2] = 1 << bits[k];
      if (k < 3) v[3 * n + 2] = 766;
      if (!refused_naming(sf_field_values_fit(SF_F_stats, v.data(), n) == SF_OK, "env 2")) return 35;
      char want[32];
      snprintf(want, sizeof(want), "stats[%d]", k);
      if (!strstr(sf_last_error(), want)) return 36;
    }
    for (int d = -1; d <= 1; d += 2) {
      std::vector<int32_t> v = top;
      v[3 * n + 2] = 765 + d;
      if (!refused_naming(sf_field_values_fit(SF_F_stats, v.data(), n) == SF_OK, "env 2") || !strstr(sf_last_error(), "sum")) return 37;
    }
  }
  // missile_angle int16 [20][3]: nine bits, in the last slot of the last env
  if (!fits1(SF_F_missile_angle, 20, 2, 19, 0) || !fits1(SF_F_missile_angle, 20, 2, 19, 511)) return 38;
  for (long bad : {-1l, 512l})
    if (!refused_naming(fits1(SF_F_missile_angle, 20, 2, 19, bad), "env 2, slot 19")) return 39;
  return 0;
}

int main() {
  if (const int rc = host_logic()) return rc;
  std::vector<int16_t> sp(4 * 65536);
  if (sf_spawn_table(1, 65536, sp.data())) return 1;
  std::vector<double> trig(720);
  if (sf_trig_table(trig.data())) return 2;
  double hp[12];
  if (sf_hex_points(200, hp) || sf_hex_points(40, hp)) return 3;
  std::vector<uint8_t> fr(92 * 90), out(84 * 84);
  for (int v = 0; v < 4; v++) {
    if (sf_image_static(v, fr.data())) return 4;
    if (sf_resize_area_u8(fr.data(), 90, 92, out.data(), 84, 84)) return 5;
  }
  const char* names[] = {"youturn", "autoturn", "test-youturn", "test-autoturn", "bogus"};
  for (const char* n : names) {
    sf_preset p;
    uint8_t keys[16];
    int rc = sf_preset_get(n, &p);
    for (int as = -1; as <= 2; as++) sf_action_table(n, as, keys);
    printf("%s %d\n", n, rc);
  }
  // the image observation's host rasteriser (sf_cairo_host.cpp, sf_tor.h): every picture table and the test hooks, incl. objects
  // across the surface's borders and another geometry
  std::vector<uint8_t> fa(256), big(200 * 200);
  for (int k = 0; k < 36; k++)
    if (sf_image_fort_alpha(k, fa.data())) return 7;
  std::vector<double> arcs(86 * 8);
  if (sf_arc_table(arcs.data())) return 8;
  if (sf_image_background_geom(112, 115, 130, 80, 450, 460, 3.0, big.data())) return 9;
  for (int k = 0; k < 4; k++)
    for (int i = 0; i < 40; i++) {
      const double x = 125 + 11.7 * i, y = (i & 1) ? 78.3 + 11.9 * i : 541.2 - 3.3 * i;
      if (sf_image_object_alpha(k, x, y, (37 * i) % 360, 90, 92, 130, 80, 450, 460, 3.0, fr.data())) return 10;
      if (sf_image_object_alpha(k, x, y, (37 * i) % 360, 180, 184, 130, 80, 450, 460, 3.0, big.data())) return 11;
    }
  for (int i = 0; i < 6; i++) {
    if (sf_image_explosion_host(131.5 + 80 * i, 85.0 + 70 * i, 90, 92, 130, 80, 450, 460, 3.0, fr.data())) return 12;
    if (sf_image_explosion_host(131.5 + 80 * i, 85.0 + 70 * i, 180, 184, 130, 80, 450, 460, 3.0, big.data())) return 13;
    if (sf_image_arc_alpha(300.0, 300.0, 20.0 + 9 * i, 0.3 * i, 0.3 * i + 1.2, 180, 184, 130, 80, 450, 460, 3.0, big.data()) < 1) return 14;
  }
  int32_t f[84], c[84];
  float a[84 * 4];
  if (sf_resize_area_tab(90, 84, f, c, a) || sf_resize_area_tab(92, 84, f, c, a)) return 6;
  printf("ok %s\n", sf_last_error());
  return 0;
}
