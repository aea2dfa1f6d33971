// sf_lane_dev.h -- device code only: one env's state in registers (Lane) and what sf_kernels.hip (the hot path) and
// sf_state_ops.hip (the state tools) both do with it.  Macros, types and __forceinline__ functions in the anonymous
// namespace: each file compiles its own copy, so a change to one file's kernels leaves the other's code object alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sf_internal.h"
#include "sf_layout.h"
#include "sf_deg_dd.h"

#define SF_MAX_MISSILES_D 20.0 /* sf.MAX_MISSILES / sf.MAX_SHELLS as divisors (ENV:124-125) */
#ifndef M_PI
#define M_PI 3.14159265358979323846
#endif

// Field access inside the wave's tile (sf_layout.h): `tb` is the tile base -- wave-uniform, one
// SGPR pair for the whole state -- the group/slot offset is a compile-time constant and the lane
// contributes a 32-bit byte offset (one VGPR per chunk size: 16, 8, 4 or 2 bytes).
#define SF_CHUNK(group, s)                                   \
  (tb + sfl::chunk_offset(SF_G_##group, 0) +                 \
   (size_t)(s) * (size_t)(sfl::kGroups[SF_G_##group].chunk * sfl::kTileLanes))
#define SF_LD(T, base, off) (*reinterpret_cast<const T*>((base) + (off)))
// Stores of 16-byte chunks are write-through (`sc1`): the bytes leave L2 while the kernel still runs, so the
// end-of-kernel write-back has less to flush (A/B, tools/ab.py on one device, 65 536 envs: plain stores 11.20 us per
// launch, non-temporal 11.01, write-through 10.83.  With the earlier 1-8-byte rows `sc1` LOST 1 %: narrow
// write-through stores are one fabric write each).  Nothing stored this way is read again inside the launch.
// the cache bits of the write-through stores: inline-asm text and the builtins' aux value (1 = sc0, 2 = nt, 16 = sc1)
#define SF_SC_AUX 16
#define SF_SC_ASM "sc1"
template <typename T>
__device__ __forceinline__ void sf_store(T* p, T v) {
  if constexpr (sizeof(T) == 16) {
    // the s_nop belongs to the store: a store of more than 64 bits reads its data registers over several cycles and
    // the next VALU write of one of them needs a wait state in between, which the compiler cannot insert for an
    // instruction it does not see (found as misc.prev_vlner of lanes 12-15 of every 16 holding the NEXT store's word)
    asm volatile("global_store_dwordx4 %0, %1, off " SF_SC_ASM "\n\ts_nop 1" ::"v"(p), "v"(v) : "memory");
  } else {
    *p = v;
  }
}

// The projectile slots, the lane's chunks and the counters go through `buffer_*` instructions on a per-wave descriptor of the
// tile.  The slot's chunk offset (a compile-time constant too big for the 12-bit immediate) rides in
// the scalar offset instead of costing two 64-bit VALU adds per access, and a lane that has nothing in
// the slot gets an out-of-range offset: the hardware range check returns 0 for its load and drops its
// store, so there is no exec-mask branch around each access.
#define SF_GOFF(group, s) \
  ((unsigned)sfl::chunk_offset(SF_G_##group, 0) + (unsigned)(s) * (unsigned)(sfl::kGroups[SF_G_##group].chunk * sfl::kTileLanes))
#define SF_OOB 0x80000000u /* beyond any tile: the lane's access does not happen */

typedef double d2_t __attribute__((ext_vector_type(2)));
typedef int i4_t __attribute__((ext_vector_type(4)));
typedef int i2_t __attribute__((ext_vector_type(2)));
typedef unsigned int u4_t __attribute__((ext_vector_type(4)));

// A 128-bit buffer store with the wait state its data registers need ATTACHED.  A store of more than 64 bits reads its data
// VGPRs over several cycles, and a VALU write of one of them in the next issue slot changes what lanes 12-15 of every 16
// store.  The compiler inserts the s_nop for global / flat stores and for buffer stores with an immediate soffset, but takes a
// buffer store whose soffset is an SGPR to be safe (LLVM GCNHazardRecognizer::createsVALUHazard).  On MI355X that holds
// while the wave is alone on its SIMD -- every batch up to 65 536 envs, every test of rounds 1-3 -- and does not with two or
// more: a batch of 262 144 envs played different games than the same envs in four batches, in exactly those lanes (round 4;
// tests/test_gpu_parity.py::test_batches_beyond_one_wave_per_simd).  So the store goes out as inline assembly with its s_nop
// (the compiler cannot place anything in between), like sf_store's global one; tools/store_hazard_scan.py checks a build's
// assembly for wide buffer stores the compiler emitted bare.  AUX as the builtin's: 0 plain, 16 write-through (sc1).
template <int AUX>
__device__ __forceinline__ void sf_buf_st128(u4_t v, __amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff) {
  static_assert(AUX == 0 || AUX == 16, "cache bits of the store");
  if constexpr (AUX == 16)
    asm volatile("buffer_store_dwordx4 %0, %1, %2, %3 offen sc1\n\ts_nop 1" ::"v"(v), "v"(voff), "s"(rs), "s"(soff) : "memory");
  else
    asm volatile("buffer_store_dwordx4 %0, %1, %2, %3 offen\n\ts_nop 1" ::"v"(v), "v"(voff), "s"(rs), "s"(soff) : "memory");
}

namespace {

struct Lane {
  double sx, sy, vx, vy;
  int angle;
  unsigned fl;
  int death_t, fire_t, thrust_t, left_t, right_t;
  int fort_t, fort_death_t, fort_vuln_t;
  int fort_angle, fort_last;
  float points, raw;
  int vlner, time;
  int prev_vlner;
  unsigned cursor, mmask, smask;
  unsigned kc0, kc1;  // key-press counters: shots | thrusts << 16, lefts | rights << 16 (sf_layout.h: SF_KEYCOUNT_BYTE)
  // the per-episode counters that ride above the timers, vlner, time and the cursor (sf_layout.h: SF_W_*)
  int ep_return;
  unsigned c_resets, c_missed, c_incs, c_maxv, c_big, c_small, c_shell, c_destroyed;
  unsigned mpool;     // live entries of the tile's missile pool (wave-uniform; rides above the missile mask)
  unsigned ep_kills;  // sum of info over the episode (rides above the shell mask)
};

struct Off {  // 32-bit byte offsets of this lane into rows of 16-, 8-, 4-, 2- and 1-byte chunks
  unsigned o16, o8, o4, o2, o1;
};

// a / C for a compile-time constant C, bit-identical to the IEEE division it replaces, in three dependent
// operations instead of the eleven of the general v_div_* sequence (v_rcp_f64 included): with rc = RN(1/C),
// q = RN(a * rc) is within an ulp of a / C, rem = a - C * q is exact in an FMA, and RN(q + rem * rc) is the
// correctly rounded quotient (Markstein's theorem).  Checked exhaustively enough on the host for every C used
// here -- pi, 10, 20, 80, 90, 92, 180, 360, 5294: 4e8 operands each, none differ (tests/test_div_const.py keeps a
// smaller run of the same check).  Only the sign of a zero quotient can differ (-0.0 / C gives +0.0 here); nothing
// downstream looks at it.  The operands are angles, pixels and tick counts: no overflow, underflow or NaN.
__device__ __forceinline__ double sf_div_const(double a, double c, double rc) {
  const double q = a * rc;
  const double rem = __builtin_fma(-c, q, a);
  return __builtin_fma(rem, rc, q);
}
#define SF_DIV(a, C) sf_div_const((a), (double)(C), 1.0 / (double)(C))
__device__ __forceinline__ double rad2deg(double a) { return SF_DIV(a, M_PI) * 180; }  // SRC/vector.cpp:38-40

// atan2 as the reference's libm rounds it where it matters.  The device libm (ocml) is faithful, glibc is correctly
// rounded, and for nearly every argument the last-bit difference is invisible: the results only feed ceil-to-10
// degrees (fortress sector), ceil-to-1 degree (autoturn heading) and observations.  Ships move on near-lattices,
// though (integer spawns, velocities that are sums of 0.3 * cos(6k degrees)), and do cross x = 355 or y = 315 within
// 1e-13: the bearing is then a whisker off +-90 or +-180 degrees -- multiples of 10 -- and which side of the
// boundary the ROUNDED value falls on is decided by that last bit (found by a 3e8-step soak: sector 280 against the
// reference's 270).  Next to the y axis and to the negative x axis the result is therefore formed as
// +-pi/2 - x/y and +-pi + y/x with pi in two doubles: one rounding, the correctly rounded value, bit for bit what
// glibc returns there (4e7 such arguments checked on the host, tests/native/atan2_axis.c).  A wave-wide test skips
// the block on all but a handful of ticks.
//
// The same last bit decides whenever the bearing is within rounding noise of ANY integer degree, and in autoturn games
// that is a regime, not an accident: a ship that thrusts at the fortress flies along an exact-degree ray.  RAZOR = 1:
// within 1e-9 degrees of k degrees the result is formed as phi_k + N / D, N = |y| cos k - x sin k in double-double
// (products exact by FMA; phi, cos, sin of k = 0..180 as (hi, lo) pairs, sf_deg_dd.h), D = x cos k + |y| sin k: the
// correctly rounded value.  glibc's own atan2 is not correctly rounded in 0.08 % of such arguments (0.503-ulp errors,
// tools/atan2_razor), so agreement there is 99.9 %, not 100 % -- against a coin toss per tick for the plain device libm.
// atan2 for the step kernel's hot path, half the instructions of the device libm's: no special cases (the arguments are
// finite coordinate / velocity differences), the quotient q = min / max in [0, 1] by a reciprocal and Newton steps, then
// one table step atan(q) = atan(k / 16) + atan(t), t = (q - k/16) / (1 + q k/16), |t| <= 1/32, where five terms of the
// series leave 3e-18.  `atab` = atan(k / 16), k = 0..16, in LDS (host libm, sf_host_fill_consts).  Within 1e-15 rad of
// the host libm's atan2 (a few ulps; tests/native/atan2_core.c restates it on the host); everything that needs MORE than
// that -- the axes, the integer degrees -- is decided by sf_atan2's exact forms below, which do not look at this value's
// last bits.  (0, 0) gives a NaN: the only caller that can pass it, the velocity bearing, discards the value for a ship
// at rest.
__device__ __forceinline__ double sf_recip(double d) {  // 1 / d to an ulp or so, d in the normal range
  double r = __builtin_amdgcn_rcp(d);
  r = __builtin_fma(__builtin_fma(-d, r, 1.0), r, r);
  return __builtin_fma(__builtin_fma(-d, r, 1.0), r, r);
}
__device__ __forceinline__ double sf_atan2_core(double y, double x, const double* atab) {
  const double ax = fabs(x), ay = fabs(y);
  const double u = __builtin_fmax(ax, ay), v = __builtin_fmin(ax, ay);
  const double ru = sf_recip(u);
  double q = v * ru;
  q = __builtin_fma(__builtin_fma(-u, q, v), ru, q);
  const double k = rint(q * 16.0), c = k * 0.0625;
  const double den = __builtin_fma(q, c, 1.0), num = q - c;
  const double rd = sf_recip(den);
  double t = num * rd;
  t = __builtin_fma(__builtin_fma(-den, t, num), rd, t);
  const double s = t * t;
  double p = __builtin_fma(s, 1.0 / 9.0, -1.0 / 7.0);
  p = __builtin_fma(s, p, 0.2);
  p = __builtin_fma(s, p, -1.0 / 3.0);
  double a = atab[(int)k] + __builtin_fma(t, p * s, t);
  a = ay > ax ? 1.5707963267948966 - a : a;
  a = x < 0 ? 3.141592653589793 - a : a;
  return copysign(a, y);
}

template <bool RAZOR>
__device__ __forceinline__ double sf_atan2(double y, double x, const double* atab = nullptr) {
  double r = atab ? sf_atan2_core(y, x, atab) : atan2(y, x);
  const double ax = fabs(x), ay = fabs(y);
  const bool ny = ax * 0x1p27 < ay;              // next to the y axis (x == 0 included)
  const bool nx = (x < 0) & (ay * 0x1p27 < ax);  // next to the negative x axis (y == 0 included)
  if (__ballot(ny | nx) != 0ull) {
    if (ny | nx) {
      const double t = ny ? x / y : y / x;
      const double hi = ny ? 1.5707963267948966 : 3.141592653589793;          // pi/2, pi
      const double lo = ny ? 6.123233995736766e-17 : 1.2246467991473532e-16;  // their low parts
      r = copysign(hi, y) + (ny ? copysign(lo, y) - t : copysign(lo, y) + t);
    }
  }
  if (RAZOR) {
    const double deg = SF_DIV(fabs(r), M_PI) * 180, kd = rint(deg);
    const bool rz = !(ny | nx) & (fabs(deg - kd) < 1e-9) & (y != 0.0);
    if (__ballot(rz) != 0ull) {
      if (rz) {
        const double* e = kDegDD[(int)kd];  // (phi_hi, phi_lo, cos_hi, cos_lo, sin_hi, sin_lo) of kd degrees
        const double ph = e[0], pl = e[1], ch = e[2], cl = e[3], sh = e[4], sl = e[5];
        const double p1 = ay * ch, e1 = __builtin_fma(ay, ch, -p1);
        const double p2 = x * sh, e2 = __builtin_fma(x, sh, -p2);
        const double d = p1 - p2;  // nearly cancels
        const double bb = d - p1, err = (p1 - (d - bb)) + (-p2 - bb);  // two-sum error term of p1 + (-p2)
        const double lo = err + (e1 - e2) + (ay * cl - x * sl);
        const double N = d + lo, D = x * ch + ay * sh;
        r = copysign(ph + (pl + N / D), y);
      }
    }
  }
  return r;
}

// Hexagon::isInside (SRC/hexagon.cpp:36-48).  The edges (nx, ny, px, py) are compile-time
// constants (sf_layout.h: both radii are the same in every preset), so they are immediates.
// For the two horizontal edges of each hexagon nx is -0.0, so  nx*dx + ny*dy < 0  is exactly
// ny*dy < 0 (adding a zero changes nothing, a zero product is not < 0), i.e. a plain comparison
// of y against the edge: y < py for ny > 0, y > py for ny < 0 (the sign of a difference of two
// doubles is exact, and scaling by |ny| >= 1 cannot flush it to zero).  Eight multiplies, eight
// subtractions and four additions less per ship and tick, same truth value for every finite y.
// The six truth values are folded arithmetically: "no edge value is < 0" is "the smallest edge value is not < 0"
// (for the horizontal edges the value is the difference y - py or py - y; -0.0 is not < 0 either way; no NaN
// here), one comparison per hexagon instead of six whose results meet in scalar registers.
#define SF_EDGE_TEST(nx, ny, px, py)                                                                  \
  m = __builtin_fmin(m, (nx) == 0.0 ? ((ny) > 0 ? y - (py) : (py) - y) : (nx) * (x - (px)) + (ny) * (y - (py)));
__device__ __forceinline__ bool inside_big_hex(double x, double y) {
  double m = 1.0;
  SF_BIG_HEX_EDGES(SF_EDGE_TEST)
  return !(m < 0);
}
__device__ __forceinline__ bool inside_small_hex(double x, double y) {
  double m = 1.0;
  SF_SMALL_HEX_EDGES(SF_EDGE_TEST)
  return !(m < 0);
}
#undef SF_EDGE_TEST

// Game::isOutsideGameArea (SRC/game.cpp:129-131)
__device__ __forceinline__ bool outside_area(const SfKernelArgs& a, double x, double y) {
  return (x < 0) | (x > sfc::width_d) | (y > sfc::height_d) | (y < 0);
}

// Game::resetShip (SRC/game.cpp:133-149).  The accepted (x, y, angle) of the rejection loop over
// libc rand() is a fixed sequence per seed: the host precomputed it (sf_spawn_table) and each
// lane walks it with its own cursor.
// `e` = the lane's next table entry, packed (x, y, angle, 0) as four int16
__device__ __forceinline__ void spawn_ship_from(const SfKernelArgs& a, Lane& L, unsigned long long e) {
  L.cursor += 1;
  L.sx = (double)(int16_t)(e & 0xFFFFu);
  L.sy = (double)(int16_t)((e >> 16) & 0xFFFFu);
  L.angle = (int16_t)((e >> 32) & 0xFFFFu);
  L.vx = a.start_vx;
  L.vy = a.start_vy;
  L.fl |= SF_FL_SHIP_ALIVE;
}
__device__ __forceinline__ void spawn_ship(const SfKernelArgs& a, Lane& L) {
  spawn_ship_from(a, L, *reinterpret_cast<const unsigned long long*>(a.spawn + 4 * (size_t)(L.cursor & a.spawn_mask)));
}

// Game::Game (SRC/game.cpp:18-82); statistics and episode sums are zeroed by the caller
__device__ __forceinline__ void new_game(const SfKernelArgs& a, Lane& L) {
  L.fl = 0;
  spawn_ship(a, L);
  L.fl |= SF_FL_FORT_ALIVE;
  L.fort_angle = 180;  // :40
  L.fort_last = 0;     // :41
  L.points = 0;
  L.raw = 0;
  L.vlner = 0;
  L.time = 0;
  L.death_t = L.fire_t = L.thrust_t = L.left_t = L.right_t = 0;
  L.fort_t = L.fort_death_t = 0;
  L.fort_vuln_t = sfc::vuln_time;  // :78 adds to a never-initialised member; defined as 0 + 250
  L.mmask = L.smask = 0;
  L.kc0 = L.kc1 = 0;  // statistics start over with the game (SRC/game.cpp:18-82)
  L.ep_return = 0;
  L.c_resets = L.c_missed = L.c_incs = L.c_maxv = L.c_big = L.c_small = L.c_shell = L.c_destroyed = 0;
  L.ep_kills = 0;
  // (L.mpool belongs to the tile, not to the game: the caller maintains it)
}

// The fixed part of a lane: eight 16-byte chunks (sf_layout.h), in two sets.  The start of a launch is a chip-wide burst --
// every wave of every CU pulls its state at once and the fabric delivers about 12 bytes per cycle and CU -- so what the
// first phases of the tick need (keys, respawn, ship, fortress: flags and angles, masks, the timers, position and
// velocity) is issued FIRST and waited for alone; the two chunks that are first read at the shells or later (score,
// counts) and the missile pool rows are issued behind the dependent loads of round trip 2 and arrive under the
// key / ship / fortress arithmetic.
struct LaneLate {
  i4_t ta, sc;
};
__device__ __forceinline__ void load_lane_early(const unsigned char* tb, const Off& o, Lane& L) {
  const i4_t mi = SF_LD(i4_t, SF_CHUNK(misc, 0), o.o16);  // first: the projectile prefetch waits on the masks
  const i4_t sm = SF_LD(i4_t, SF_CHUNK(small, 0), o.o16);
  const d2_t p = SF_LD(d2_t, SF_CHUNK(ship_pos, 0), o.o16);
  const d2_t v = SF_LD(d2_t, SF_CHUNK(ship_vel, 0), o.o16);
  const i4_t tc = SF_LD(i4_t, SF_CHUNK(timers_b, 0), o.o16);
  L.right_t = (int)(int16_t)(tc.x & 0xFFFF);
  L.ep_return = (int)((unsigned)tc.x & 0xFFFF0000u);  // bits 16..31; the low half comes with the late set
  L.fort_t = tc.y;
  L.fort_death_t = tc.z;
  L.fort_vuln_t = tc.w;
  L.death_t = mi.x;
  L.cursor = (unsigned)mi.y & 0xFFFFFFu;
  L.c_destroyed = (unsigned)mi.y >> 24;
  L.mmask = (unsigned)mi.z & SF_MASK_LOW;
  L.mpool = (unsigned)mi.z >> SF_MPOOL_SHIFT;
  L.smask = (unsigned)mi.w & SF_MASK_LOW;
  L.ep_kills = (unsigned)mi.w >> SF_KILLS_SHIFT;
  L.sx = p.x;
  L.sy = p.y;
  L.vx = v.x;
  L.vy = v.y;
  L.angle = (int16_t)(sm.x & 0xFFFF);
  L.fort_angle = (int16_t)((unsigned)sm.x >> 16);
  L.fort_last = (int16_t)(sm.y & 0xFFFF);
  L.fl = ((unsigned)sm.y >> 16) & 0xFFu;
  L.kc0 = (unsigned)sm.z;
  L.kc1 = (unsigned)sm.w;
}
__device__ __forceinline__ LaneLate load_lane_late(const unsigned char* tb, const Off& o) {
  LaneLate t;
  t.ta = SF_LD(i4_t, SF_CHUNK(timers_a, 0), o.o16);
  t.sc = SF_LD(i4_t, SF_CHUNK(score, 0), o.o16);
  return t;
}
__device__ __forceinline__ void unpack_lane_late(const LaneLate& t, Lane& L) {
  const unsigned w_pvl = (unsigned)t.ta.x, w_fire = (unsigned)t.ta.y, w_thr = (unsigned)t.ta.z, w_left = (unsigned)t.ta.w;
  const unsigned w_vl = (unsigned)t.sc.z, w_time = (unsigned)t.sc.w;
  L.prev_vlner = (int)(w_pvl & 0xFFFu);
  L.c_incs = (w_pvl >> 12) & 0xFFFu;
  L.c_big = w_pvl >> 24;
  L.fire_t = (int)(int16_t)(w_fire & 0xFFFFu);
  L.c_resets = w_fire >> 16;
  L.thrust_t = (int)(int16_t)(w_thr & 0xFFFFu);
  L.c_missed = w_thr >> 16;
  L.left_t = (int)(int16_t)(w_left & 0xFFFFu);
  L.ep_return = (int)((unsigned)L.ep_return | (w_left >> 16));  // the high half came with timers_b
  L.points = __int_as_float(t.sc.x);
  L.raw = __int_as_float(t.sc.y);
  L.vlner = (int)(w_vl & 0xFFFu);
  L.c_maxv = (w_vl >> 12) & 0xFFFu;
  L.c_small = w_vl >> 24;
  L.time = (int)(w_time & 0xFFFFFFu);
  L.c_shell = w_time >> 24;
}

// The lane's seven chunks back to the tile, through the wave's descriptor: the chunk offsets ride in the scalar
// offset, no 64-bit address per store; write-through (SF_SC_AUX).  Four pieces, so that a launch of one tick can issue a piece
// as soon as its last writer has run (sf_step_kernel, kEarlySt: the ship behind the shells' walk, the score chunk behind the
// missile events, the rest behind the timers and the reward); store_lane_buf is the four in the order the chunks always
// had.  The pieces are macros over (rs, o, L): as functions inside store_lane_buf they gave the launches that keep the one
// store other instruction orders around it; as text, none (tools/device_code_id.py --kernels, profiles/step_wave_ends.md).
#define SF_BST16(group, v) sf_buf_st128<SF_SC_AUX>(__builtin_bit_cast(u4_t, v), rs, o.o16, SF_GOFF(group, 0))
#define SF_ST_LANE_SHIP                    \
  SF_BST16(ship_pos, (d2_t{L.sx, L.sy})); \
  SF_BST16(ship_vel, (d2_t{L.vx, L.vy}));
// the packed words of sf_layout.h (SF_W_*): a value below, a per-episode counter above (`er`: the episode's return)
#define SF_ST_LANE_TIMERS                                                                                                       \
  SF_BST16(timers_a, (i4_t{(int)(((unsigned)L.prev_vlner & 0xFFFu) | ((L.c_incs & 0xFFFu) << 12) | (L.c_big << 24)),           \
                           (int)(((unsigned)L.fire_t & 0xFFFFu) | (L.c_resets << 16)),                                         \
                           (int)(((unsigned)L.thrust_t & 0xFFFFu) | (L.c_missed << 16)),                                       \
                           (int)(((unsigned)L.left_t & 0xFFFFu) | (er << 16))}));                                              \
  SF_BST16(timers_b, (i4_t{(int)(((unsigned)L.right_t & 0xFFFFu) | (er & 0xFFFF0000u)), L.fort_t, L.fort_death_t, L.fort_vuln_t}));
#define SF_ST_LANE_SCORE                                                                                             \
  SF_BST16(score, (i4_t{__float_as_int(L.points), __float_as_int(L.raw),                                            \
                        (int)(((unsigned)L.vlner & 0xFFFu) | ((L.c_maxv & 0xFFFu) << 12) | (L.c_small << 24)),      \
                        (int)(((unsigned)L.time & 0xFFFFFFu) | (L.c_shell << 24))}));
#define SF_ST_LANE_MISC_SMALL                                                                                                               \
  SF_BST16(misc, (i4_t{L.death_t, (int)((L.cursor & 0xFFFFFFu) | (L.c_destroyed << 24)), (int)(L.mmask | (L.mpool << SF_MPOOL_SHIFT)),     \
                       (int)(L.smask | (L.ep_kills << SF_KILLS_SHIFT))}));                                                                 \
  sf_buf_st128<SF_SC_AUX>(                                                                                                                  \
      u4_t{(unsigned)(L.angle & 0xFFFF) | ((unsigned)(L.fort_angle & 0xFFFF) << 16),                                                       \
           (unsigned)(L.fort_last & 0xFFFF) | ((L.fl & 0xFFFFu) << 16), L.kc0, L.kc1},                                                     \
      rs, o.o16, SF_GOFF(small, 0));
__device__ __forceinline__ void store_lane_buf(__amdgpu_buffer_rsrc_t rs, const Off& o, const Lane& L) {
  SF_ST_LANE_SHIP
  const unsigned er = (unsigned)L.ep_return;
  SF_ST_LANE_TIMERS
  SF_ST_LANE_SCORE
  SF_ST_LANE_MISC_SMALL
}
__device__ __forceinline__ void store_lane_ship(__amdgpu_buffer_rsrc_t rs, const Off& o, const Lane& L) { SF_ST_LANE_SHIP }
__device__ __forceinline__ void store_lane_score(__amdgpu_buffer_rsrc_t rs, const Off& o, const Lane& L) { SF_ST_LANE_SCORE }
// timers_a, timers_b, misc and small: what every tick writes last -- the timers, the reward byte, the counters the reward feeds
__device__ __forceinline__ void store_lane_rest(__amdgpu_buffer_rsrc_t rs, const Off& o, const Lane& L) {
  const unsigned er = (unsigned)L.ep_return;
  SF_ST_LANE_TIMERS
  SF_ST_LANE_MISC_SMALL
}
#undef SF_ST_LANE_SHIP
#undef SF_ST_LANE_TIMERS
#undef SF_ST_LANE_SCORE
#undef SF_ST_LANE_MISC_SMALL
#undef SF_BST16

__device__ __forceinline__ void store_lane(unsigned char* tb, const Off& o, const Lane& L) {
  store_lane_buf(__builtin_amdgcn_make_buffer_rsrc(tb, 0, (int)sfl::kTileBytes, 0x00020000), o, L);
}

// ExtraGameValues of Game::computeExtra (SRC/game.cpp:282-312).  They are a pure function of the
// ship state (frozen while the ship is dead), so they are derived for the observation instead of
// being stored.  a_pos = atan2(sy - fy, sx - fx) is shared with updateFortress, a_vel =
// atan2(vy, vx); both are evaluated side by side so the two dependency chains interleave.
struct Extras {
  double aim, vdir, ndist;
};

__device__ __forceinline__ Extras compute_extras(const SfKernelArgs& a, const Lane& L, double a_pos, double a_vel) {
  Extras e;
  // aim (SRC/game.cpp:299-305)
  double o = rad2deg(a_pos) - (double)L.angle + 180;
  if (o < -180) o = o + 360;
  e.aim = o;
  // vdir (SRC/game.cpp:286-297).  norm()==0 iff vx*vx+vy*vy==0.  The reference's first atan2 is
  // atan2(-(fy-sy), fx-sx) = atan2(dy, -dx) = +-pi - a_pos: derived from a_pos (observation-only
  // value, differs from a second libm call by <= 1 ulp of pi).
  {
    const double dy = L.sy - sfc::fort_y;
    double ov;
    if (dy == 0)  // on the fortress row the two calls sit on different branch cuts: call it
      ov = sf_atan2<false>(-(sfc::fort_y - L.sy), sfc::fort_x - L.sx);
    else
      ov = dy < 0 ? (-M_PI - a_pos) : (M_PI - a_pos);
    double diff = a_vel - ov;
    if (diff > M_PI) diff -= M_PI * 2;
    if (diff < -M_PI) diff += M_PI * 2;
    e.vdir = (L.vx * L.vx + L.vy * L.vy == 0.0) ? 0.0 : rad2deg(diff);
  }
  // fdist, ndist (SRC/game.cpp:310-311): the y term of the reference subtracts the ship from
  // itself, so fdist = sqrt(dx^2 + 0) = |dx|.
  const double fdist = fabs(L.sx - sfc::fort_x);
  e.ndist = -1 + SF_DIV(fdist - sfc::ndist_a, sfc::ndist_b);
  return e;
}

// ---- the same bearings, sector arithmetic and extras with their fp64 constants as DATA (a split launch's games' wave) ----
// The instruction set has no 64-bit literals: a double compiled in is a pair of scalar moves, and with every SGPR in use the
// compiler builds the pair again in front of each use.  A wave alone on its SIMD pays an issue turn for each of them --
// some 40 per tick in the two atan2s, rad2deg, the sector and computeExtra.  SfKRow holds those constants in VGPRs, filled
// by eight broadcast LDS reads from the constants row the workgroup staged (sf_layout.h: SF_KROW_LIST, written by
// sf_host_fill_consts from the same expressions); measured at 65 536 envs: -0.10 us per launch (profiles/step_constants.md).
// The functions below restate rad2deg, sf_atan2_core, sf_atan2 and compute_extras operation for operation, in the same
// order, on the same values -- with -ffp-contract=off the same bits (tests/test_gpu_step_constants.py plays both for 300
// ticks and compares every bit).  They are separate functions, not a template over the originals: the kernels that keep
// the immediates (no registers to spare: 176 VGPRs at two waves per SIMD) must stay what they were instruction for
// instruction, and with the originals written over a constants type six of them came out of the compiler with other registers.
struct SfKRow {
#define SF_K(name, value) double name;
  SF_KROW_LIST(SF_K)
#undef SF_K
};
static_assert(sizeof(SfKRow) == SF_KROW_DOUBLES * sizeof(double) && SF_CONST_KROW % 2 == 0 && SF_KROW_DOUBLES % 2 == 0, "SF_KROW_LIST");
namespace sfkrow {  // the row's values against what the originals compile in
#define SF_K(name, value) constexpr double name = (value);
SF_KROW_LIST(SF_K)
#undef SF_K
static_assert(pi == M_PI && half_pi == 1.5707963267948966 && inv_pi == 1.0 / (double)(M_PI) && d10 == (double)sfc::sector_size &&
              inv10 == 1.0 / (double)sfc::sector_size && ndist_a == sfc::ndist_a && ndist_b == sfc::ndist_b &&
              inv_ndist_b == 1.0 / (double)sfc::ndist_b, "SF_KROW_LIST");
}  // namespace sfkrow
__device__ __forceinline__ SfKRow sf_load_krow(const double* row) {  // `row`: 16-byte aligned, in LDS, the same for every lane
  d2_t v[SF_KROW_DOUBLES / 2];
#pragma unroll
  for (int k = 0; k < SF_KROW_DOUBLES / 2; k++) v[k] = reinterpret_cast<const d2_t*>(row)[k];
  SfKRow K;
  int k = 0;
#define SF_K(name, value) K.name = (k & 1) ? v[k / 2].y : v[k / 2].x; k++;
  SF_KROW_LIST(SF_K)
#undef SF_K
  return K;
}
__device__ __forceinline__ double rad2deg(double a, const SfKRow& kc) { return sf_div_const(a, kc.pi, kc.inv_pi) * kc.d180; }
__device__ __forceinline__ double sf_atan2_core(double y, double x, const double* atab, const SfKRow& kc) {
  const double ax = fabs(x), ay = fabs(y);
  const double u = __builtin_fmax(ax, ay), v = __builtin_fmin(ax, ay);
  const double ru = sf_recip(u);
  double q = v * ru;
  q = __builtin_fma(__builtin_fma(-u, q, v), ru, q);
  const double k = rint(q * kc.d16), c = k * kc.inv16;
  const double den = __builtin_fma(q, c, 1.0), num = q - c;
  const double rd = sf_recip(den);
  double t = num * rd;
  t = __builtin_fma(__builtin_fma(-den, t, num), rd, t);
  const double s = t * t;
  double p = __builtin_fma(s, kc.c9, kc.c7);
  p = __builtin_fma(s, p, kc.c5);
  p = __builtin_fma(s, p, kc.c3);
  double a = atab[(int)k] + __builtin_fma(t, p * s, t);
  a = ay > ax ? kc.half_pi - a : a;
  a = x < 0 ? kc.pi - a : a;
  return copysign(a, y);
}
__device__ __forceinline__ double sf_atan2_razor(double y, double x, const double* atab, const SfKRow& kc) {  // sf_atan2<true>
  double r = sf_atan2_core(y, x, atab, kc);
  const double ax = fabs(x), ay = fabs(y);
  const bool ny = ax * 0x1p27 < ay;
  const bool nx = (x < 0) & (ay * 0x1p27 < ax);
  if (__ballot(ny | nx) != 0ull) {
    if (ny | nx) {
      const double t = ny ? x / y : y / x;
      const double hi = ny ? 1.5707963267948966 : 3.141592653589793;
      const double lo = ny ? 6.123233995736766e-17 : 1.2246467991473532e-16;
      r = copysign(hi, y) + (ny ? copysign(lo, y) - t : copysign(lo, y) + t);
    }
  }
  const double deg = sf_div_const(fabs(r), kc.pi, kc.inv_pi) * kc.d180, kd = rint(deg);
  const bool rz = !(ny | nx) & (fabs(deg - kd) < 1e-9) & (y != 0.0);
  if (__ballot(rz) != 0ull) {
    if (rz) {
      const double* e = kDegDD[(int)kd];
      const double ph = e[0], pl = e[1], ch = e[2], cl = e[3], sh = e[4], sl = e[5];
      const double p1 = ay * ch, e1 = __builtin_fma(ay, ch, -p1);
      const double p2 = x * sh, e2 = __builtin_fma(x, sh, -p2);
      const double d = p1 - p2;
      const double bb = d - p1, err = (p1 - (d - bb)) + (-p2 - bb);
      const double lo = err + (e1 - e2) + (ay * cl - x * sl);
      const double N = d + lo, D = x * ch + ay * sh;
      r = copysign(ph + (pl + N / D), y);
    }
  }
  return r;
}
__device__ __forceinline__ Extras compute_extras(const SfKernelArgs& a, const Lane& L, double a_pos, double a_vel, const SfKRow& kc) {
  Extras e;
  double o = rad2deg(a_pos, kc) - (double)L.angle + kc.d180;
  if (o < -kc.d180) o = o + kc.d360;
  e.aim = o;
  {
    const double dy = L.sy - sfc::fort_y;
    double ov;
    if (dy == 0)
      ov = sf_atan2<false>(-(sfc::fort_y - L.sy), sfc::fort_x - L.sx);
    else
      ov = dy < 0 ? (-kc.pi - a_pos) : (kc.pi - a_pos);
    double diff = a_vel - ov;
    if (diff > kc.pi) diff -= M_PI * 2;
    if (diff < -kc.pi) diff += M_PI * 2;
    e.vdir = (L.vx * L.vx + L.vy * L.vy == 0.0) ? 0.0 : rad2deg(diff, kc);
  }
  const double fdist = fabs(L.sx - sfc::fort_x);
  e.ndist = -1 + sf_div_const(fdist - kc.ndist_a, kc.ndist_b, kc.inv_ndist_b);
  return e;
}

// One observation row (ENV:95-157) written to `o` (an LDS staging row or global memory).
template <typename T>
__device__ __forceinline__ void write_obs(const SfKernelArgs& a, T* o, const Lane& L, const Extras& e) {
  const int n_missiles = __popc(L.mmask);
  const int n_shells = a.real_shell_count ? __popc(L.smask) : n_missiles;  // SRC/pymodule.cpp:131-134
  // ENV:148 reads the vulnerability timer through a getter with undefined behaviour
  // (SRC/pymodule.cpp:44-45); the intended predicate is used.
  const int kill_ready = (L.vlner > 10 && L.fort_vuln_t < sfc::vuln_time) ? 1 : 0;
  const int n_keys_t = a.obs_dim - 15;
  const int timers[4] = {L.fire_t, L.thrust_t, L.left_t, L.right_t};  // SRC/pymodule.cpp:98-105
  const bool ship_alive = L.fl & SF_FL_SHIP_ALIVE, fort_alive = L.fl & SF_FL_FORT_ALIVE;
  if (a.obs_type == 2) {  // monitors, ENV:96-108
    o[0] = (T)(n_missiles > 0 ? 0.5 : -0.5);
    o[1] = (T)(fort_alive ? 0.5 : -0.5);
    o[2] = (T)(L.vlner > 10 ? 0.5 : -0.5);
    o[3] = (T)(kill_ready ? 0.5 : -0.5);
    o[4] = (T)(e.aim < 3 ? 0.5 : -0.5);
    o[5] = (T)(e.aim > 3 ? 0.5 : -0.5);
    o[6] = (T)(e.ndist > .75 ? 0.5 : -0.5);
    o[7] = (T)(e.ndist > .25 ? 0.5 : -0.5);
    o[8] = (T)(e.ndist < -.25 ? 0.5 : -0.5);
    o[9] = (T)(e.ndist < -.75 ? 0.5 : -0.5);
  } else if (a.obs_type == 1) {  // normalized-features, ENV:109-133
    double f[19];
    f[0] = ship_alive ? 1 : 0;
    f[1] = SF_DIV(L.sx, sfc::pb_width);
    f[2] = SF_DIV(L.sy, sfc::pb_height);
    f[3] = SF_DIV(L.vx, 10);
    f[4] = SF_DIV(L.vy, 10);
    f[5] = SF_DIV((double)L.angle, 360);
    f[6] = SF_DIV(e.aim, 180);
    {
      double m = fmod(e.vdir, 360.0);  // Python float %: result takes the divisor's sign
      if (m != 0) {
        if (m < 0) m += 360.0;
      } else {
        m = 0.0;
      }
      f[7] = SF_DIV(m, 360);
    }
    f[8] = e.ndist;
    f[9] = fort_alive ? 1 : 0;
    f[10] = SF_DIV((double)L.fort_angle, 360);
    f[11] = SF_DIV((double)(L.vlner > 10 ? L.vlner : 10), 10);  // ENV:122 max(), as written
    f[12] = kill_ready;
    f[13] = SF_DIV((double)n_missiles, SF_MAX_MISSILES_D);
    f[14] = SF_DIV((double)n_shells, SF_MAX_MISSILES_D);
#pragma unroll
    for (int k = 0; k < 4; k++) f[15 + k] = SF_DIV((double)timers[k], sfc::max_ticks);
#pragma unroll
    for (int k = 0; k < 19; k++) {
      if (k < 15 + n_keys_t) {
        double v = f[k];
        v = v < -1 ? -1 : (v > 1 ? 1 : v);
        o[k] = (T)v;
      }
    }
  } else {  // features, ENV:134-157
    o[0] = (T)(ship_alive ? 1 : 0);
    o[1] = (T)L.sx;
    o[2] = (T)L.sy;
    o[3] = (T)L.vx;
    o[4] = (T)L.vy;
    o[5] = (T)L.angle;
    o[6] = (T)e.aim;
    o[7] = (T)e.vdir;
    o[8] = (T)e.ndist;
    o[9] = (T)(fort_alive ? 1 : 0);
    o[10] = (T)L.fort_angle;
    o[11] = (T)L.vlner;
    o[12] = (T)kill_ready;
    o[13] = (T)n_missiles;
    o[14] = (T)n_shells;
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (k < n_keys_t) o[15 + k] = (T)timers[k];
  }
}

// A new game's extras: the reference's are stale heap until the first tick; defined as computeExtra(spawn) -- or, by flag, as
// the zeros a fresh process's heap holds there (SF_FLAG_REF_RESET_OBS)
__device__ __forceinline__ Extras new_game_extras(const SfKernelArgs& a, const Lane& L) {
  Extras e = compute_extras(a, L, sf_atan2<true>(L.sy - sfc::fort_y, L.sx - sfc::fort_x), sf_atan2<false>(L.vy, L.vx));
  if (a.ref_reset_obs) e = Extras{0.0, 0.0, 0.0};
  return e;
}

// env e's row of the observation array `obs`, in the batch's element type
__device__ __forceinline__ void write_obs_row(const SfKernelArgs& a, void* obs, size_t e, const Lane& L, const Extras& x) {
  if (a.obs_f64)
    write_obs<double>(a, (double*)obs + e * a.obs_dim, L, x);
  else
    write_obs<float>(a, (float*)obs + e * a.obs_dim, L, x);
}

}  // namespace
