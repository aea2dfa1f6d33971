// sf_state_ops.hip -- the state tools: kernels that read or rewrite the tiled state off the hot path -- the masked reset, the
// draw records from the state, sf_get_field / sf_set_field, the slot view of the missile pools, the lane states, the two
// launches around a masked step (sf_step_where).  They share
// sf_lane_dev.h with sf_kernels.hip and nothing else: a change here leaves the step kernel's code object alone.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sf_drawrec.h"
#include "sf_lane_dev.h"  // (with sf_internal.h and sf_layout.h)

namespace {

constexpr int kBlock = 256;  // threads per workgroup of the per-env copy kernels

// A tile's missile pool (sf_layout.h): `count` entries -- the count rides above the missile mask in every lane's missile word
// -- of (x, y) in missile_pos and a meta word (SF_MM_*: heading, owner lane, slot) in missile_meta.

// The walk: f(k, meta) for the entries k = lane, lane + 64, ... of the pool whose missile word is `count_word`.  Bounded by
// what a pool and an env can hold whatever the words say: k < 64 * SF_NSLOT, and an entry whose 5-bit slot tag is not below
// SF_NSLOT is passed over (the callers index [SF_NSLOT] arrays with it; the 6-bit owner is always a lane).  The entry's
// position is the caller's to load (missile_pos, 16 * k): not every caller wants every one.
template <typename F>
__device__ __forceinline__ void pool_for_each(const unsigned char* tb, unsigned count_word, unsigned lane, F f) {
  const unsigned count = count_word >> SF_MPOOL_SHIFT, n = count < 64u * SF_NSLOT ? count : 64u * SF_NSLOT;
  for (unsigned k = lane; k < n; k += 64) {
    const unsigned m = SF_LD(unsigned, SF_CHUNK(missile_meta, 0), k * 4u);
    if (SF_MM_SLOT(m) < (unsigned)SF_NSLOT) f(k, m);
  }
}

// The rebuild, by the whole wave: `mask` = this lane's alive slots, pos_of_slot(s) / ang_of_slot(s) its missile in slot s (asked
// only for slots of the mask).  The entries' ORDER is the contract: slot-major, lanes ascending inside a slot (ballot + prefix
// count, the step kernel's compaction).  Returns the count; mask | count << SF_MPOOL_SHIFT into the missile words is the caller's.
template <typename P, typename A>
__device__ __forceinline__ unsigned pool_rebuild(unsigned char* tb, unsigned mask, unsigned lane, P pos_of_slot, A ang_of_slot) {
  unsigned wp = 0;
  for (int s = 0; s < SF_NSLOT; s++) {
    const bool live = (mask >> s) & 1u;
    const unsigned long long b = __ballot(live);
    const unsigned idx = wp + __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, 0u));
    wp += (unsigned)__popcll(b);
    if (live) {
      *reinterpret_cast<d2_t*>(SF_CHUNK(missile_pos, 0) + (size_t)idx * 16) = pos_of_slot(s);
      *reinterpret_cast<unsigned*>(SF_CHUNK(missile_meta, 0) + (size_t)idx * 4) = SF_MM_PACK((unsigned)ang_of_slot(s) & 511u, lane, s);
    }
  }
  return wp;
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// sf_reset_lanes: env.reset() in the envs the caller marks (ENV:163-178), the others play on.  One wave per tile, a lane
// per env; mask = uint8 [n_envs], any non-zero byte marks its env (no byte at or beyond n_envs is read).  A tile without a
// marked env returns before it writes anything.  Otherwise the marked lanes start a new game exactly as sf_reset_kernel's
// re-reset does -- prev_vlner and the spawn cursor are the lane's own --, and their missiles leave the tile's pool: the
// kept lanes' entries go through LDS by (owner, slot) and the pool is rebuilt from them (pool_rebuild); the new count goes
// into every lane's missile word.  A kept lane's chunks, shells and slots are as before (only WHERE its entries sit in the
// pool may differ, which no row and no tick can tell); the lanes behind the batch in a partial last tile count as kept.
// obs (may be null): the marked lanes' rows as sf_reset_kernel writes them; no other row is touched.  hint (image batches):
// the marked lanes' bits are cleared -- a new game's ship did not die in the last tick.
// FINISH (sf_finish_lanes_kernel, sfmi_final.h): the marked lanes are games that ENDED in the step launch in front, which ran
// with auto_reset off -- before the new game their episode totals go into a.acc, from the lane's counters as that launch left
// them, exactly as the step kernel's own auto-reset adds them (sf_kernels.hip: "episode totals")
template <bool FINISH>
__device__ __forceinline__ void reset_lanes_tile(const SfKernelArgs& a, const uint8_t* mask, void* obs, d2_t (*spos)[SF_NSLOT],
                                                 unsigned short (*sang)[SF_NSLOT]) {
  const unsigned lane = threadIdx.x;
  const long tile_i = blockIdx.x;
  const long e = tile_i * 64 + lane;
  const bool marked = e < a.n_envs && mask[e] != 0;
  const unsigned long long rmask = __ballot(marked);
  if (rmask == 0ull) return;  // (uniform)
  unsigned char* const tb = a.state + (size_t)tile_i * sfl::kTileBytes;
  const Off o = {lane * 16u, lane * 8u, lane * 4u, lane * 2u, lane};
  // everything that is read from the tile, first
  const i4_t mi = SF_LD(i4_t, SF_CHUNK(misc, 0), o.o16);
  const unsigned pvl_w = SF_LD(unsigned, SF_CHUNK(timers_a, 0), o.o16);
  if constexpr (FINISH) {
    if (marked) {
      Lane F;
      load_lane_early(tb, o, F);
      unpack_lane_late(load_lane_late(tb, o), F);
      const int ep_ret = F.ep_return, ep_kil = (int)F.ep_kills;
      const int deaths = (int)(F.c_big + F.c_small + F.c_shell);
      const int shots = (int)(F.kc0 & 0xFFFFu);
      atomicAdd(&a.acc[0], 1ull);
      atomicAdd(&a.acc[1], (unsigned long long)(long long)ep_ret);
      atomicAdd(&a.acc[2], (unsigned long long)((long long)ep_ret * ep_ret));
      atomicAdd(&a.acc[3], (unsigned long long)(long long)ep_kil);
      atomicAdd(&a.acc[4], (unsigned long long)deaths);
      atomicAdd(&a.acc[5], (unsigned long long)shots);
      atomicMin((long long*)&a.acc[6], (long long)ep_ret);
      atomicMax((long long*)&a.acc[7], (long long)ep_ret);
    }
  }
  pool_for_each(tb, (unsigned)__builtin_amdgcn_readfirstlane(mi.z), lane, [&](unsigned i, unsigned m) {  // (the same word's count in every lane)
    const unsigned ow = SF_MM_OWNER(m);
    if (!((rmask >> ow) & 1ull)) {
      spos[ow][SF_MM_SLOT(m)] = SF_LD(d2_t, SF_CHUNK(missile_pos, 0), i * 16u);
      sang[ow][SF_MM_SLOT(m)] = (unsigned short)SF_MM_ANGLE(m);
    }
  });
  const unsigned kept = marked ? 0u : ((unsigned)mi.z & SF_MASK_LOW);
  __syncthreads();
  const unsigned wp = pool_rebuild(tb, kept, lane, [&](int s) { return spos[lane][s]; }, [&](int s) { return sang[lane][s]; });
  if (!marked) {
    *reinterpret_cast<unsigned*>(SF_CHUNK(misc, 0) + o.o16 + 8u) = kept | (wp << SF_MPOOL_SHIFT);
  } else {
    Lane L;
    L.prev_vlner = (int)(pvl_w & 0xFFFu);
    L.cursor = (unsigned)mi.y;
    new_game(a, L);
    L.mpool = wp;
    store_lane(tb, o, L);
    if (obs != nullptr && a.obs_type != 3) write_obs_row(a, obs, (size_t)e, L, new_game_extras(a, L));  // (as sf_reset_kernel)
  }
  if (a.hint && lane == 0) a.hint[tile_i] &= ~rmask;
}

__global__ __launch_bounds__(64) void sf_reset_lanes_kernel(SfKernelArgs a, const uint8_t* mask, void* obs) {
  __shared__ d2_t spos[64][SF_NSLOT];
  __shared__ unsigned short sang[64][SF_NSLOT];
  reset_lanes_tile<false>(a, mask, obs, spos, sang);
}

__global__ __launch_bounds__(64) void sf_finish_lanes_kernel(SfKernelArgs a, const uint8_t* done) {
  __shared__ d2_t spos[64][SF_NSLOT];
  __shared__ unsigned short sang[64][SF_NSLOT];
  reset_lanes_tile<true>(a, done, nullptr, spos, sang);
}

hipError_t sf_launch_reset_lanes(const SfKernelArgs& a, const uint8_t* mask, void* obs, hipStream_t stream) {
  hipLaunchKernelGGL(sf_reset_lanes_kernel, dim3((unsigned)((a.n_envs + 63) / 64)), dim3(64), 0, stream, a, mask, obs);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// The envs' draw records (sf_drawrec.h) from the state as it is in HBM: what the image instantiations of the step kernel
// leave behind themselves, for a state that got there any other way -- a reset, sf_set_field, a batch that steps with a
// symbolic observation and renders now and then.  One wave per tile, a lane per env; the pool's entries file their
// transforms at [owner][slot] and tell their owners through LDS where they come near the score / the bar, exactly like the
// step kernel's m_row.  Same functions, same values: tests/test_gpu_image.py compares the two byte for byte.
// `take`: the lanes whose records are written (wave-uniform; all of them for sf_drawrec_kernel, the held ones behind a masked step).
__device__ __forceinline__ void drawrec_tile(const unsigned char* state, int n_envs, unsigned char* draw, int pics, unsigned long long take,
                                             unsigned* near) {
  const unsigned lane = threadIdx.x;
  const long tile_i = blockIdx.x;
  const unsigned char* tb = state + tile_i * sfl::kTileBytes;
  unsigned char* const dr = draw + tile_i * (long)SF_DR_TILE_BYTES;
  const unsigned o16 = lane * 16u;
  const d2_t sp = SF_LD(d2_t, SF_CHUNK(ship_pos, 0), o16);
  const i4_t tc = SF_LD(i4_t, SF_CHUNK(timers_b, 0), o16);
  const i4_t sc = SF_LD(i4_t, SF_CHUNK(score, 0), o16);
  const i4_t mi = SF_LD(i4_t, SF_CHUNK(misc, 0), o16);
  const i4_t sm = SF_LD(i4_t, SF_CHUNK(small, 0), o16);
  near[lane] = 0u;
  __syncthreads();
  pool_for_each(tb, (unsigned)__builtin_amdgcn_readfirstlane(mi.z), lane, [&](unsigned i, unsigned m) {  // (the same word's count in every lane)
    if (!((take >> SF_MM_OWNER(m)) & 1ull)) return;
    const d2_t p = SF_LD(d2_t, SF_CHUNK(missile_pos, 0), i * 16u);
    *reinterpret_cast<d2_t*>(dr + (SF_DR_PIECE_OBJ0 + SF_DR_OBJ_MISSILE0 + SF_MM_SLOT(m)) * SF_DR_PIECE_STRIDE + SF_MM_OWNER(m) * SF_DR_LANE_STRIDE) = p;
    *reinterpret_cast<int16_t*>(dr + SF_DR_ANGLES_OFF + 2 * SF_MM_SLOT(m) + SF_MM_OWNER(m) * SF_DR_LANE_STRIDE) = (int16_t)SF_MM_ANGLE(m);
    const unsigned f = sfd::hud_flags_near((float)p.x, (float)p.y, sfd::kMissileExt);
    if (f) atomicOr(&near[SF_MM_OWNER(m)], f);
  });
  const unsigned smask = (unsigned)mi.w & SF_MASK_LOW, mmask = (unsigned)mi.z & SF_MASK_LOW;
  unsigned proj = 0u;
  for (unsigned rest = smask; rest; rest &= rest - 1u) {
    const int s = __ffs(rest) - 1;
    const d2_t q = SF_LD(d2_t, SF_CHUNK(shell_pos, s), o16);
    proj |= sfd::hud_flags_near((float)q.x, (float)q.y, sfd::kShellExt);
  }
  __syncthreads();
  proj |= near[lane];
  if (tile_i * 64 + lane >= n_envs || !((take >> lane) & 1ull)) return;
  const int ship_angle = (int16_t)(sm.x & 0xFFFF), fort_angle = (int16_t)((unsigned)sm.x >> 16);
  const unsigned fl = ((unsigned)sm.y >> 16) & 0xFFu;
  const sfd::Header h = sfd::make_header(sp.x, sp.y, ship_angle, (fl & SF_FL_SHIP_ALIVE) != 0u, (fl & SF_FL_FORT_ALIVE) != 0u, fort_angle,
                                         __int_as_float(sc.x), sc.z & 0xFFF, tc.w, mmask, smask, proj, pics != 0,
                                         (int)((unsigned)sc.w & 0xFFFFFFu));
  unsigned char* const me = dr + lane * SF_DR_LANE_STRIDE;
  *reinterpret_cast<u4_t*>(me) = u4_t{h.w[0], h.w[1], h.w[2], h.w[3]};
  *reinterpret_cast<u4_t*>(me + SF_DR_PIECE_STRIDE) = u4_t{h.w[4], h.w[5], h.w[6], h.w[7]};
  *reinterpret_cast<d2_t*>(me + (SF_DR_PIECE_OBJ0 + SF_DR_OBJ_SHIP) * SF_DR_PIECE_STRIDE) = sp;
}

__global__ __launch_bounds__(64) void sf_drawrec_kernel(const unsigned char* state, int n_envs, unsigned char* draw, int pics) {
  __shared__ unsigned near[64];
  drawrec_tile(state, n_envs, draw, pics, ~0ull, near);
}

hipError_t sf_launch_drawrec(const SfKernelArgs& a, hipStream_t stream) {
  if (!a.draw) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sf_drawrec_kernel, dim3((unsigned)(a.lanes / 64)), dim3(64), 0, stream, a.state, a.n_envs, a.draw, a.draw_pics);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// sf_get_field / sf_set_field: one field between the tiled state and a linear [count][n_envs]
// buffer (not on the hot path).
template <typename T>
__global__ __launch_bounds__(kBlock) void sf_field_copy_kernel(unsigned char* state, int n_envs, long tile_off,
                                                                int lane_stride, int slot_stride, int count,
                                                                T* linear, int to_linear) {
  const long e = (long)blockIdx.x * kBlock + threadIdx.x;
  if (e >= n_envs) return;
  unsigned char* lane0 = state + (e >> 6) * sfl::kTileBytes + tile_off + (e & 63) * lane_stride;
  for (int c = 0; c < count; c++) {
    T* p = reinterpret_cast<T*>(lane0 + (long)c * slot_stride);
    if (to_linear)
      linear[(long)c * n_envs + e] = *p;
    else
      *p = linear[(long)c * n_envs + e];
  }
}

// sf_get_field / sf_set_field for the fields that are not one element at a fixed place of a chunk (sf_layout.h: SF_FK_*).

// "stats": the reference's 13 ints (SRC/game.hh:29-43) from / to their bit fields (sf_layout.h: SF_W_*); ship deaths
// (row 3) is the sum of rows 0-2 and is not stored (a value written to it is ignored).
__global__ __launch_bounds__(kBlock) void sf_stats_copy_kernel(unsigned char* state, int n_envs, int32_t* linear,
                                                                int to_linear) {
  const long e = (long)blockIdx.x * kBlock + threadIdx.x;
  if (e >= n_envs) return;
  unsigned char* tile = state + (e >> 6) * sfl::kTileBytes;
  const long lo = (e & 63) * 16;
  uint16_t* kc = reinterpret_cast<uint16_t*>(tile + sfl::chunk_offset(SF_G_small, 0) + lo + SF_KEYCOUNT_BYTE);
  uint32_t* ta = reinterpret_cast<uint32_t*>(tile + sfl::chunk_offset(SF_G_timers_a, 0) + lo);  // pvl, fire, thrust, left
  uint32_t* sc = reinterpret_cast<uint32_t*>(tile + sfl::chunk_offset(SF_G_score, 0) + lo);     // .., .., vlner, time
  uint32_t* mi = reinterpret_cast<uint32_t*>(tile + sfl::chunk_offset(SF_G_misc, 0) + lo);      // .., cursor, .., ..
#define SF_ROW(k) linear[(long)(k) * n_envs + e]
#define SF_PUT(word, shift, bits, k) word = (word & ~((((1u << (bits)) - 1u)) << (shift))) | (((uint32_t)SF_ROW(k) & ((1u << (bits)) - 1u)) << (shift))
  if (to_linear) {
    const int big = (int)(ta[0] >> 24), sml = (int)(sc[2] >> 24), shl = (int)(sc[3] >> 24);
    SF_ROW(SF_ST_BIG_HEX_DEATHS) = big;
    SF_ROW(SF_ST_SMALL_HEX_DEATHS) = sml;
    SF_ROW(SF_ST_SHELL_DEATHS) = shl;
    SF_ROW(SF_ST_SHIP_DEATHS) = big + sml + shl;
    SF_ROW(SF_ST_RESETS) = (int)(ta[1] >> 16);
    SF_ROW(SF_ST_DESTROYED) = (int)(mi[1] >> 24);
    SF_ROW(SF_ST_MISSED) = (int)(ta[2] >> 16);
    for (int c = 0; c < SF_ST_KEY_COUNT; c++) SF_ROW(SF_ST_KEY_FIRST + c) = kc[c];
    SF_ROW(SF_ST_VLNER_INCS) = (int)((ta[0] >> 12) & 0xFFFu);
    SF_ROW(SF_ST_MAX_VLNER) = (int)((sc[2] >> 12) & 0xFFFu);
  } else {
    SF_PUT(ta[0], 24, 8, SF_ST_BIG_HEX_DEATHS);
    SF_PUT(sc[2], 24, 8, SF_ST_SMALL_HEX_DEATHS);
    SF_PUT(sc[3], 24, 8, SF_ST_SHELL_DEATHS);
    SF_PUT(ta[1], 16, 16, SF_ST_RESETS);
    SF_PUT(mi[1], 24, 8, SF_ST_DESTROYED);
    SF_PUT(ta[2], 16, 16, SF_ST_MISSED);
    for (int c = 0; c < SF_ST_KEY_COUNT; c++) kc[c] = (uint16_t)SF_ROW(SF_ST_KEY_FIRST + c);
    SF_PUT(ta[0], 12, 12, SF_ST_VLNER_INCS);
    SF_PUT(sc[2], 12, 12, SF_ST_MAX_VLNER);
  }
#undef SF_PUT
#undef SF_ROW
}

// a bit field of a 32-bit word of the lane's chunk (sf_layout.h: SF_BITFIELDS) from / to a linear int32 buffer
__global__ __launch_bounds__(kBlock) void sf_bits_copy_kernel(unsigned char* state, int n_envs, long tile_off, int shift,
                                                               int bits, int is_signed, uint32_t* linear, int to_linear) {
  const long e = (long)blockIdx.x * kBlock + threadIdx.x;
  if (e >= n_envs) return;
  uint32_t* w = reinterpret_cast<uint32_t*>(state + (e >> 6) * sfl::kTileBytes + tile_off + (e & 63) * 16);
  const uint32_t mask = bits >= 32 ? ~0u : ((1u << bits) - 1u);
  if (to_linear) {
    uint32_t v = (*w >> shift) & mask;
    if (is_signed && bits < 32 && (v >> (bits - 1))) v |= ~mask;
    linear[e] = v;
  } else {
    *w = (*w & ~(mask << shift)) | ((linear[e] & mask) << shift);
  }
}
// "ep_return": int32, bits 0..15 above the left timer, bits 16..31 above the right timer
__global__ __launch_bounds__(kBlock) void sf_epret_copy_kernel(unsigned char* state, int n_envs, int32_t* linear, int to_linear) {
  const long e = (long)blockIdx.x * kBlock + threadIdx.x;
  if (e >= n_envs) return;
  unsigned char* tile = state + (e >> 6) * sfl::kTileBytes;
  uint32_t* wl = reinterpret_cast<uint32_t*>(tile + sfl::chunk_offset(SF_G_timers_a, 0) + (e & 63) * 16 + 12);
  uint32_t* wr = reinterpret_cast<uint32_t*>(tile + sfl::chunk_offset(SF_G_timers_b, 0) + (e & 63) * 16);
  if (to_linear) {
    linear[e] = (int32_t)((*wl >> 16) | (*wr & 0xFFFF0000u));
  } else {
    const uint32_t v = (uint32_t)linear[e];
    *wl = (*wl & 0xFFFFu) | (v << 16);
    *wr = (*wr & 0xFFFFu) | (v & 0xFFFF0000u);
  }
}

// The missile fields, per env and slot as the reference has them (mMissiles[i], SRC/game.hh:90), from / to the tile's pool.
// `slots` is the batch's slot-major view [SF_NSLOT][n_envs] of (x, y) as d2_t and of the heading as int32.
// Pool -> slots: every live entry goes to (slot, owner); slots without a missile read 0.
__global__ __launch_bounds__(64) void sf_mpool_to_slots_kernel(const unsigned char* state, int n_envs, d2_t* sl_pos,
                                                              int32_t* sl_ang) {
  const long tile_i = blockIdx.x;
  const unsigned lane = threadIdx.x;
  const unsigned char* tb = state + tile_i * sfl::kTileBytes;
  const long e = tile_i * 64 + lane;
  if (e < n_envs)
    for (int s = 0; s < SF_NSLOT; s++) {
      sl_pos[(long)s * n_envs + e] = d2_t{0, 0};
      sl_ang[(long)s * n_envs + e] = 0;
    }
  __syncthreads();
  pool_for_each(tb, SF_LD(unsigned, SF_CHUNK(misc, 0), 8u), lane, [&](unsigned i, unsigned m) {  // (lane 0's missile word)
    const long oe = tile_i * 64 + SF_MM_OWNER(m);
    if (oe < n_envs) {
      sl_pos[(long)SF_MM_SLOT(m) * n_envs + oe] = SF_LD(d2_t, SF_CHUNK(missile_pos, 0), i * 16u);
      sl_ang[(long)SF_MM_SLOT(m) * n_envs + oe] = (int)SF_MM_ANGLE(m);
    }
  });
}
// Slots -> pool: the tile's pool is rebuilt from the alive masks (pool_rebuild) and the count written into every lane's
// missile word; the lanes behind the batch have no missiles.
__global__ __launch_bounds__(64) void sf_slots_to_mpool_kernel(unsigned char* state, int n_envs, const d2_t* sl_pos,
                                                              const int32_t* sl_ang) {
  const long tile_i = blockIdx.x;
  const unsigned lane = threadIdx.x;
  unsigned char* const tb = state + tile_i * sfl::kTileBytes;
  const long e = tile_i * 64 + lane;
  unsigned* const mw = reinterpret_cast<unsigned*>(SF_CHUNK(misc, 0) + lane * 16u + 8u);
  const unsigned mask = e < n_envs ? (*mw & SF_MASK_LOW) : 0u;
  const unsigned wp = pool_rebuild(tb, mask, lane, [&](int s) { return sl_pos[(long)s * n_envs + e]; },
                                   [&](int s) { return sl_ang[(long)s * n_envs + e]; });
  *mw = mask | (wp << SF_MPOOL_SHIFT);
}

hipError_t sf_launch_mpool_to_slots(const unsigned char* state, int n_envs, void* sl_pos, int32_t* sl_ang, hipStream_t stream) {
  hipLaunchKernelGGL(sf_mpool_to_slots_kernel, dim3((unsigned)((n_envs + 63) / 64)), dim3(64), 0, stream, state, n_envs,
                     (d2_t*)sl_pos, sl_ang);
  return hipGetLastError();
}
hipError_t sf_launch_slots_to_mpool(unsigned char* state, long lanes, int n_envs, const void* sl_pos, const int32_t* sl_ang,
                                    hipStream_t stream) {
  hipLaunchKernelGGL(sf_slots_to_mpool_kernel, dim3((unsigned)(lanes / 64)), dim3(64), 0, stream, state, n_envs,
                     (const d2_t*)sl_pos, sl_ang);
  return hipGetLastError();
}

// one component of the slot-major missile view <-> the caller's linear [SF_NSLOT][n_envs] buffer
// which: 0 = x, 1 = y (double), 2 = heading (int16)
__global__ __launch_bounds__(kBlock) void sf_mslot_component_kernel(d2_t* sl_pos, int32_t* sl_ang, long total, int which,
                                                                     void* linear, int to_linear) {
  const long k = (long)blockIdx.x * kBlock + threadIdx.x;
  if (k >= total) return;
  if (which == 2) {
    if (to_linear) ((int16_t*)linear)[k] = (int16_t)sl_ang[k];
    else sl_ang[k] = ((const int16_t*)linear)[k];
  } else {
    double* comp = reinterpret_cast<double*>(sl_pos + k) + which;
    if (to_linear) ((double*)linear)[k] = *comp;
    else *comp = ((const double*)linear)[k];
  }
}
hipError_t sf_launch_mslot_component(void* sl_pos, int32_t* sl_ang, long total, int which, void* linear, int to_linear,
                                     hipStream_t stream) {
  hipLaunchKernelGGL(sf_mslot_component_kernel, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream,
                     (d2_t*)sl_pos, sl_ang, total, which, linear, to_linear);
  return hipGetLastError();
}

// PMC calibration (sf_calibration_copy): copy whole 16-byte chunks of one group to the linear
// buffer -- 16 B per lane, 1 KiB per wave-instruction, exactly the step kernel's access pattern.
__global__ __launch_bounds__(kBlock) void sf_group_copy_kernel(const unsigned char* state, int n_envs, long tile_off,
                                                                int slots, i4_t* linear) {
  const long e = (long)blockIdx.x * kBlock + threadIdx.x;
  if (e >= n_envs) return;
  const unsigned char* lane0 = state + (e >> 6) * sfl::kTileBytes + tile_off + (e & 63) * 16;
  for (int c = 0; c < slots; c++)
    linear[(long)c * n_envs + e] = *reinterpret_cast<const i4_t*>(lane0 + (long)c * 16 * sfl::kTileLanes);
}

hipError_t sf_launch_group_copy(const unsigned char* state, int n_envs, int group, unsigned char* linear,
                                hipStream_t stream) {
  const unsigned grid = (unsigned)((n_envs + kBlock - 1) / kBlock);
  hipLaunchKernelGGL(sf_group_copy_kernel, dim3(grid), dim3(kBlock), 0, stream, state, n_envs,
                     sfl::group_offset(group), sfl::kGroups[group].slots, (i4_t*)linear);
  return hipGetLastError();
}

hipError_t sf_launch_field_copy(unsigned char* state, int n_envs, int field, unsigned char* linear, int to_linear,
                                hipStream_t stream) {
  const sfl::FieldMeta& m = sfl::kFields[field];
  const unsigned grid = (unsigned)((n_envs + kBlock - 1) / kBlock);
  if (m.kind == SF_FK_STATS) {
    hipLaunchKernelGGL(sf_stats_copy_kernel, dim3(grid), dim3(kBlock), 0, stream, state, n_envs, (int32_t*)linear, to_linear);
    return hipGetLastError();
  }
  if (m.kind == SF_FK_BITS) {
    const sfl::BitField bf = sfl::bit_field(field);
    hipLaunchKernelGGL(sf_bits_copy_kernel, dim3(grid), dim3(kBlock), 0, stream, state, n_envs,
                       sfl::group_offset(m.group) + m.byte_in_chunk, bf.shift, bf.bits, bf.is_signed, (uint32_t*)linear, to_linear);
    return hipGetLastError();
  }
  if (m.kind == SF_FK_EPRET) {
    hipLaunchKernelGGL(sf_epret_copy_kernel, dim3(grid), dim3(kBlock), 0, stream, state, n_envs, (int32_t*)linear, to_linear);
    return hipGetLastError();
  }
  if (m.kind == SF_FK_MPOOL) return hipErrorInvalidValue;  // sf_capi.cpp goes through the slot view (sf_launch_mslot_component)
  const int lane_stride = sfl::kGroups[m.group].chunk, slot_stride = lane_stride * sfl::kTileLanes;
  const long off = sfl::group_offset(m.group) + m.byte_in_chunk;
#define SF_COPY(T)                                                                                                      \
  hipLaunchKernelGGL(sf_field_copy_kernel<T>, dim3(grid), dim3(kBlock), 0, stream, state, n_envs, off, lane_stride, \
                     slot_stride, m.count, (T*)linear, to_linear)
  switch (m.elem_size) {
    case 1: SF_COPY(uint8_t); break;
    case 2: SF_COPY(uint16_t); break;
    case 4: SF_COPY(uint32_t); break;
    default: SF_COPY(uint64_t); break;
  }
#undef SF_COPY
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Lane states (sfmi.h: sf_save_lanes / sf_load_lanes / sf_copy_lanes): one env's whole game state as a row of
// SF_LANE_STATE_BYTES, independent of the lane and the tile it came from.  A row is 71 pieces of 16 bytes:
//   0        header (SF_LANE_STATE_MAGIC | version, preset, seed, spawn table length) -- sfmi.h
//   1 .. 7   the lane's chunks of ship_pos, ship_vel, timers_a, timers_b, score, misc, small (the tile's pool count that rides
//            above the missile mask is cleared: it belongs to the tile)
//   8 .. 47  its shell_pos / shell_vel chunks, slots 0 .. 19 each
//   48 .. 67 its missiles by SLOT, (x, y) -- out of the tile's pool by owner and slot as sf_mpool_to_slots_kernel takes them;
//            a slot without a missile is zero
//   68 .. 70 their headings as uint16, slots 0 .. 19, then zeros
// Save: one wave per row; the row's 71 pieces leave as one 1136-byte run of consecutive 16-byte stores.  Load: one wave
// per destination tile the call touches, which rebuilds the tile's pool from the lanes it keeps and the rows it takes.
static_assert(SF_LANE_STATE_BYTES == 16 * 71, "sfmi.h: the row's pieces");
constexpr int kLsPieces = 71, kLsBase = 1, kLsShell = 8, kLsMis = 48, kLsAng = 68;
static_assert(SF_G_ship_pos == 0 && SF_G_small == 6 && sfl::chunk_offset(SF_G_small) == 6 * 1024 &&
                  sfl::chunk_offset(SF_G_shell_vel) == sfl::chunk_offset(SF_G_shell_pos, SF_NSLOT),
              "the row copies the seven one-slot groups, then the shell groups, as runs of 1 KiB rows");

__device__ __forceinline__ long sf_lane_index(const void* idx, int idx64, long k) {
  return idx64 ? (long)reinterpret_cast<const long long*>(idx)[k] : (long)reinterpret_cast<const int*>(idx)[k];
}

// piece p (1 .. 47) of lane l: its byte offset inside the tile
__device__ __forceinline__ unsigned sf_ls_chunk_off(int p, unsigned l) {
  return (p < kLsShell ? (unsigned)(p - kLsBase) * 1024u : (unsigned)sfl::chunk_offset(SF_G_shell_pos) + (unsigned)(p - kLsShell) * 1024u) +
         16u * l;
}

// The observation rows of the lanes a state tool has just put into a tile (sf_lanes_load_kernel, sf_hold_end_kernel), by the
// whole wave: `stage` = the tile's seven one-slot chunks in tile layout, in LDS (defined values in every lane), `write` = this
// lane's row is wanted.  The step kernel's unpackers and write_obs; the bearings as the tick that made the state computed
// them: a new game's (time 0: sf_reset, an auto-reset) with the reset's atan2 and its SF_FLAG_REF_RESET_OBS, any other with
// the step's table form.
__device__ __forceinline__ void obs_rows_from_stage(const SfKernelArgs& a, const unsigned char* stage, unsigned lane, bool write, void* obs,
                                                    size_t e) {
  Lane L;
  const Off o = {lane * 16u, lane * 8u, lane * 4u, lane * 2u, lane};
  load_lane_early(stage, o, L);
  unpack_lane_late(load_lane_late(stage, o), L);
  const bool fresh = L.time == 0;
  const double* atab = a.consts + SF_CONST_ATAB;
  const Extras x = fresh ? new_game_extras(a, L)
                         : compute_extras(a, L, sf_atan2<true>(L.sy - sfc::fort_y, L.sx - sfc::fort_x, atab), sf_atan2_core(L.vy, L.vx, atab));
  if (write) write_obs_row(a, obs, e, L, x);
}

__global__ __launch_bounds__(64) void sf_lanes_save_kernel(const unsigned char* state, int n_envs, const void* lanes, int idx64,
                                                          unsigned char* rows, u4_t header, unsigned long long* refused) {
  __shared__ d2_t mpos[SF_NSLOT];
  __shared__ unsigned mang[SF_NSLOT];
  const long k = blockIdx.x;
  const unsigned lane = threadIdx.x;
  const long e = lanes ? sf_lane_index(lanes, idx64, k) : k;
  unsigned char* const row = rows + k * (long)SF_LANE_STATE_BYTES;
  if (e < 0 || e >= n_envs) {  // (uniform) no such lane: a row no batch takes
    if (lane == 0) {
      *reinterpret_cast<u4_t*>(row) = u4_t{0u, 0u, 0u, 0u};
      atomicAdd(refused, 1ull);
    }
    return;
  }
  const unsigned char* const tb = state + (e >> 6) * sfl::kTileBytes;
  const unsigned l = (unsigned)(e & 63);
  if (lane < SF_NSLOT) {
    mpos[lane] = d2_t{0.0, 0.0};
    mang[lane] = 0u;
  }
  __syncthreads();
  pool_for_each(tb, SF_LD(unsigned, SF_CHUNK(misc, 0), 16u * l + 8u), lane, [&](unsigned i, unsigned m) {
    if (SF_MM_OWNER(m) == l) {
      mpos[SF_MM_SLOT(m)] = SF_LD(d2_t, SF_CHUNK(missile_pos, 0), i * 16u);
      mang[SF_MM_SLOT(m)] = SF_MM_ANGLE(m);
    }
  });
  __syncthreads();
  for (int p = (int)lane; p < kLsPieces; p += 64) {
    u4_t v;
    if (p == 0) {
      v = header;
    } else if (p < kLsMis) {
      v = SF_LD(u4_t, tb, sf_ls_chunk_off(p, l));
      if (p == kLsBase + SF_G_misc) v.z &= SF_MASK_LOW;  // (the tile's pool count: not the lane's)
    } else if (p < kLsAng) {
      v = __builtin_bit_cast(u4_t, mpos[p - kLsMis]);
    } else {
      unsigned w[4];
#pragma unroll
      for (int j = 0; j < 4; j++) {
        const int s = 8 * (p - kLsAng) + 2 * j;
        w[j] = (s < SF_NSLOT ? mang[s] : 0u) | ((s + 1 < SF_NSLOT ? mang[s + 1] : 0u) << 16);
      }
      v = u4_t{w[0], w[1], w[2], w[3]};
    }
    *reinterpret_cast<u4_t*>(row + 16 * p) = v;
  }
}

// Load, pass 1: every (lane, row) pair of the call is checked -- lane inside the batch, row index inside the rows, the row's
// header the batch's -- and counted where it is not; the accepted ones file k into map[lane] with atomicMax (the LAST
// occurrence of a lane wins) and their tile into the list of tiles pass 2 visits (once each: the tile's flag).
__global__ __launch_bounds__(kBlock) void sf_lanes_mark_kernel(int n_envs, const void* lanes, int idx64, int n,
                                                                const unsigned char* rows, const void* row_idx, long n_rows, u4_t header,
                                                                int* map, unsigned* tflag, unsigned* tlist, unsigned* tcount,
                                                                unsigned long long* refused) {
  const long k = (long)blockIdx.x * kBlock + threadIdx.x;
  if (k >= n) return;
  const long e = lanes ? sf_lane_index(lanes, idx64, k) : k;
  const long r = row_idx ? sf_lane_index(row_idx, idx64, k) : k;
  bool ok = e >= 0 && e < n_envs && r >= 0 && r < n_rows;
  if (ok) {
    const u4_t h = *reinterpret_cast<const u4_t*>(rows + r * (long)SF_LANE_STATE_BYTES);
    ok = h.x == header.x && h.y == header.y && h.z == header.z && h.w == header.w;
  }
  if (!ok) {
    atomicAdd(refused, 1ull);
    return;
  }
  atomicMax(&map[e], (int)k);
  if (atomicExch(&tflag[e >> 6], 1u) == 0u) tlist[atomicAdd(tcount, 1u)] = (unsigned)(e >> 6);
}

// Load, pass 2: one wave per listed tile (a grid-stride loop over the list).  The lanes that take a row get its chunks; the
// tile's missile pool is rebuilt from the kept lanes' entries and the rows' slots (pool_rebuild) and its count goes into
// every lane's missile word.  map / flags are left as pass 1 found them (-1 / 0) for the next call.  obs (may be null): the
// restored lanes' observation rows, computed from the restored state by the step kernel's functions (compute_extras with
// the bearings as the step computes them, write_obs).
__global__ __launch_bounds__(64) void sf_lanes_load_kernel(SfKernelArgs a, const unsigned char* rows, const void* row_idx, int idx64,
                                                          int* map, unsigned* tflag, const unsigned* tlist, const unsigned* tcount,
                                                          void* obs) {
  __shared__ d2_t spos[64][SF_NSLOT];
  __shared__ unsigned short sang[64][SF_NSLOT];
  __shared__ __attribute__((aligned(16))) unsigned char stage[7 * 1024];  // restored lanes' seven chunks, tile layout (obs)
  const unsigned lane = threadIdx.x;
  const unsigned n_tiles = *tcount;
  for (unsigned ti = blockIdx.x; ti < n_tiles; ti += gridDim.x) {
    const unsigned t = tlist[ti];
    unsigned char* const tb = a.state + (size_t)t * sfl::kTileBytes;
    const long e = (long)t * 64 + lane;
    const int k = map[e];
    const bool restored = k >= 0;
    const unsigned char* const row =
        restored ? rows + (row_idx ? sf_lane_index(row_idx, idx64, k) : (long)k) * (long)SF_LANE_STATE_BYTES : nullptr;
    const unsigned long long rmask = __ballot(restored);
    // everything that is read from the tile, first
    const unsigned kept_mw = SF_LD(unsigned, SF_CHUNK(misc, 0), 16u * lane + 8u);
    pool_for_each(tb, (unsigned)__builtin_amdgcn_readfirstlane(kept_mw), lane, [&](unsigned i, unsigned m) {
      const unsigned ow = SF_MM_OWNER(m);
      if (!((rmask >> ow) & 1ull)) {
        spos[ow][SF_MM_SLOT(m)] = SF_LD(d2_t, SF_CHUNK(missile_pos, 0), i * 16u);
        sang[ow][SF_MM_SLOT(m)] = (unsigned short)SF_MM_ANGLE(m);
      }
    });
    unsigned mask = e < a.n_envs ? (kept_mw & SF_MASK_LOW) : 0u;
    if (restored) {
#pragma unroll 4
      for (int s = 0; s < SF_NSLOT; s++) spos[lane][s] = SF_LD(d2_t, row, 16 * (kLsMis + s));
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const u4_t w = SF_LD(u4_t, row, 16 * (kLsAng + j));
        const unsigned ww[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int q = 0; q < 8; q++)
          if (8 * j + q < SF_NSLOT) sang[lane][8 * j + q] = (unsigned short)(ww[q >> 1] >> (16 * (q & 1)));
      }
      mask = SF_LD(unsigned, row, 16 * (kLsBase + SF_G_misc) + 8) & SF_MASK_LOW;
    }
    __syncthreads();
    const unsigned wp = pool_rebuild(tb, mask, lane, [&](int s) { return spos[lane][s]; }, [&](int s) { return sang[lane][s]; });
    if (restored) {
      // eight pieces in flight at a time: (the row and the tile might alias as far as the compiler knows -- one piece per
      // round trip otherwise)
      for (int p0 = kLsBase; p0 < kLsMis; p0 += 8) {
        u4_t v[8];
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = p0 + j < kLsMis ? SF_LD(u4_t, row, 16 * (p0 + j)) : u4_t{0u, 0u, 0u, 0u};
#pragma unroll
        for (int j = 0; j < 8; j++) {
          const int p = p0 + j;
          if (p >= kLsMis) break;
          if (p == kLsBase + SF_G_misc) v[j].z = mask | (wp << SF_MPOOL_SHIFT);
          if (p < kLsShell) *reinterpret_cast<u4_t*>(stage + (p - kLsBase) * 1024 + 16 * lane) = v[j];
          *reinterpret_cast<u4_t*>(tb + sf_ls_chunk_off(p, lane)) = v[j];
        }
      }
    } else {
      *reinterpret_cast<unsigned*>(SF_CHUNK(misc, 0) + 16u * lane + 8u) = mask | (wp << SF_MPOOL_SHIFT);
      for (int g = 0; g < 7; g++) *reinterpret_cast<u4_t*>(stage + g * 1024 + 16 * lane) = u4_t{0u, 0u, 0u, 0u};  // (defined values below)
    }
    map[e] = -1;
    if (lane == 0) tflag[t] = 0u;
    if (obs != nullptr && a.obs_type != 3 && rmask != 0ull) obs_rows_from_stage(a, stage, lane, restored, obs, (size_t)e);  // (uniform)
    __syncthreads();  // (the LDS rows are the next tile's)
  }
}

hipError_t sf_launch_lanes_save(const unsigned char* state, int n_envs, const void* lanes, int idx64, int n, unsigned char* rows,
                                const uint32_t header[4], unsigned long long* refused, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(sf_lanes_save_kernel, dim3((unsigned)n), dim3(64), 0, stream, state, n_envs, lanes, idx64, rows,
                     u4_t{header[0], header[1], header[2], header[3]}, refused);
  return hipGetLastError();
}

hipError_t sf_launch_lanes_load(const SfKernelArgs& a, const void* lanes, int idx64, int n, const unsigned char* rows, const void* row_idx,
                                long n_rows, const uint32_t header[4], int* map, unsigned* tflag, unsigned* tlist, unsigned* tcount,
                                unsigned long long* refused, void* obs, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipError_t e = hipMemsetAsync(tcount, 0, sizeof(unsigned), stream);
  if (e != hipSuccess) return e;
  const u4_t h{header[0], header[1], header[2], header[3]};
  hipLaunchKernelGGL(sf_lanes_mark_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, a.n_envs, lanes,
                     idx64, n, rows, row_idx, n_rows, h, map, tflag, tlist, tcount, refused);
  const long tiles = a.lanes / 64;
  const unsigned grid = (unsigned)(n < tiles ? n : tiles);
  hipLaunchKernelGGL(sf_lanes_load_kernel, dim3(grid), dim3(64), 0, stream, a, rows, row_idx, idx64, map, tflag, tlist, tcount, obs);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// sf_step_where (sfmi_hold.h): the envs whose byte of active [n_envs] is zero are HELD while the others tick.  The tick is
// straight-line code with wave-wide ballots over a pool the tile shares, so a held lane cannot sit a launch out; instead
// sf_hold_begin_kernel swaps it for a game in which nothing can happen -- the state a REPEAT launch parks a finished env in
// (sf_kernels.hip, "PARKED") --, the unchanged step launch ticks that, and sf_hold_end_kernel swaps the lane back and rewrites
// its outputs.  One wave per tile, a lane per env; both kernels return before they write anything in a tile without a held
// env, and read no mask byte at or beyond n_envs: the lanes behind the batch in a partial last tile count as active.
//
// The stash is one more buffer in the tile layout.  A held lane's 47 chunks go to their own place in the stash's tile, its
// missiles -- out of the pool by owner and slot -- to row `slot`, lane `owner` of the stash's missile_pos / missile_meta
// rows (64 x SF_NSLOT entries: exactly the room), only the live ones.  Per held env and call 752 B read + 752 B written
// twice, 20 B more per live missile, 112 B of inert chunks; every access is a 16-byte piece of a 1 KiB row the wave moves
// whole.  Lane rows (sf_lanes_save_kernel's format) would move 1 136 B per copy, a third more, in 71-piece runs of one lane each.
//
// The inert game: ship dead with death_t = -(1 << 24) (no respawn: 255 ticks add 8 670), no missile, no shell (a dead ship
// does not fire, the fortress fires at a live ship only), time 0 (no game over for 5 295 ticks), vlner = prev_vlner = 0 and every
// per-episode counter and key timer zero (no reward, nothing that could leave its packed width: the overflow count of a
// batch without auto-reset stays).  Position, velocity, headings, the fortress's timers, the score and the spawn cursor stay
// the lane's own: nothing reads them to any effect.  tests/test_hold_model.py plays this recipe on the CPU oracle.
namespace {
constexpr int kInertDeath = -(1 << 24);

__device__ __forceinline__ u4_t* hold_chunk(unsigned char* tile, int p, unsigned lane) {  // piece p (1 .. 47) as a row has it
  return reinterpret_cast<u4_t*>(tile + sf_ls_chunk_off(p, lane));
}
}  // namespace

__global__ __launch_bounds__(64) void sf_hold_begin_kernel(SfKernelArgs a, const uint8_t* active, unsigned char* stash) {
  __shared__ d2_t spos[64][SF_NSLOT];
  __shared__ unsigned short sang[64][SF_NSLOT];
  const unsigned lane = threadIdx.x;
  const long tile_i = blockIdx.x;
  const long e = tile_i * 64 + lane;
  const bool held = e < a.n_envs && active[e] == 0;
  const unsigned long long hmask = __ballot(held);
  if (hmask == 0ull) return;  // (uniform)
  unsigned char* const tb = a.state + (size_t)tile_i * sfl::kTileBytes;
  unsigned char* const sb = stash + (size_t)tile_i * sfl::kTileBytes;
  // everything that is read from the tile's pool, first: the held lanes' entries into the stash, the others' through LDS
  const unsigned mw = SF_LD(unsigned, SF_CHUNK(misc, 0), 16u * lane + 8u);
  pool_for_each(tb, (unsigned)__builtin_amdgcn_readfirstlane(mw), lane, [&](unsigned i, unsigned m) {  // (the same word's count in every lane)
    const unsigned ow = SF_MM_OWNER(m), s = SF_MM_SLOT(m);
    const d2_t p = SF_LD(d2_t, SF_CHUNK(missile_pos, 0), i * 16u);
    if ((hmask >> ow) & 1ull) {
      *reinterpret_cast<d2_t*>(sb + sfl::chunk_offset(SF_G_missile_pos, 0) + (size_t)(s * 64u + ow) * 16) = p;
      *reinterpret_cast<unsigned*>(sb + sfl::chunk_offset(SF_G_missile_meta, 0) + (size_t)(s * 64u + ow) * 4) = SF_MM_ANGLE(m);
    } else {
      spos[ow][s] = p;
      sang[ow][s] = (unsigned short)SF_MM_ANGLE(m);
    }
  });
  const unsigned kept = held ? 0u : (mw & SF_MASK_LOW);
  __syncthreads();
  const unsigned wp = pool_rebuild(tb, kept, lane, [&](int s) { return spos[lane][s]; }, [&](int s) { return sang[lane][s]; });
  if (!held) {
    *reinterpret_cast<unsigned*>(SF_CHUNK(misc, 0) + 16u * lane + 8u) = kept | (wp << SF_MPOOL_SHIFT);
    return;
  }
  // the held lane's chunks into the stash, eight pieces in flight at a time (as sf_lanes_load_kernel moves them)
  u4_t base[kLsShell];
#pragma unroll
  for (int p = kLsBase; p < kLsShell; p++) base[p] = *hold_chunk(tb, p, lane);
#pragma unroll
  for (int p = kLsBase; p < kLsShell; p++) *hold_chunk(sb, p, lane) = base[p];
  for (int p0 = kLsShell; p0 < kLsMis; p0 += 8) {
    u4_t v[8];
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = *hold_chunk(tb, p0 + j, lane);
#pragma unroll
    for (int j = 0; j < 8; j++) *hold_chunk(sb, p0 + j, lane) = v[j];
  }
  // ... and the inert game in its place (ship_pos and ship_vel stay)
  const u4_t tb4 = base[kLsBase + SF_G_timers_b], sc = base[kLsBase + SF_G_score], mi = base[kLsBase + SF_G_misc], sm = base[kLsBase + SF_G_small];
  *hold_chunk(tb, kLsBase + SF_G_timers_a, lane) = u4_t{0u, 0u, 0u, 0u};
  *hold_chunk(tb, kLsBase + SF_G_timers_b, lane) = u4_t{0u, tb4.y, tb4.z, tb4.w};
  *hold_chunk(tb, kLsBase + SF_G_score, lane) = u4_t{sc.x, sc.y, 0u, 0u};
  *hold_chunk(tb, kLsBase + SF_G_misc, lane) = u4_t{(unsigned)kInertDeath, mi.y & 0xFFFFFFu, wp << SF_MPOOL_SHIFT, 0u};
  *hold_chunk(tb, kLsBase + SF_G_small, lane) = u4_t{sm.x, sm.y & ~(SF_FL_SHIP_ALIVE << 16), 0u, 0u};
}
static_assert((kLsMis - kLsShell) % 8 == 0, "the shell pieces move in rounds of eight");

// Behind the step launch.  The held lanes' chunks come back from the stash; the pool is rebuilt from the active lanes' entries
// as the tick left them and the held lanes' stashed slots, and its count goes into every lane's missile word.  The held
// lanes' outputs (each may be null): reward 0, done 0, info 0, ticks 0, event word 0, and the observation row of the
// restored state (obs_rows_from_stage: sf_lanes_load_kernel's writer; a batch without observation rows gets none).  Their
// render-hint bits are cleared: a held ship did not die in this call.  No row of a.final_obs is touched.
__global__ __launch_bounds__(64) void sf_hold_end_kernel(SfKernelArgs a, const uint8_t* active, const unsigned char* stash, void* obs,
                                                        int32_t* reward, uint8_t* done, uint8_t* info, uint8_t* ticks) {
  __shared__ d2_t spos[64][SF_NSLOT];
  __shared__ unsigned short sang[64][SF_NSLOT];
  __shared__ __attribute__((aligned(16))) unsigned char stage[7 * 1024];  // the held lanes' seven chunks, tile layout (obs)
  const unsigned lane = threadIdx.x;
  const long tile_i = blockIdx.x;
  const long e = tile_i * 64 + lane;
  const bool held = e < a.n_envs && active[e] == 0;
  const unsigned long long hmask = __ballot(held);
  if (hmask == 0ull) return;  // (uniform)
  unsigned char* const tb = a.state + (size_t)tile_i * sfl::kTileBytes;
  unsigned char* const sb = const_cast<unsigned char*>(stash) + (size_t)tile_i * sfl::kTileBytes;
  const unsigned mw = SF_LD(unsigned, SF_CHUNK(misc, 0), 16u * lane + 8u);
  pool_for_each(tb, (unsigned)__builtin_amdgcn_readfirstlane(mw), lane, [&](unsigned i, unsigned m) {
    const unsigned ow = SF_MM_OWNER(m);
    if (!((hmask >> ow) & 1ull)) {  // (an inert lane owns nothing)
      spos[ow][SF_MM_SLOT(m)] = SF_LD(d2_t, SF_CHUNK(missile_pos, 0), i * 16u);
      sang[ow][SF_MM_SLOT(m)] = (unsigned short)SF_MM_ANGLE(m);
    }
  });
  unsigned mask = mw & SF_MASK_LOW;
  if (held) {
    mask = SF_LD(unsigned, sb, sf_ls_chunk_off(kLsBase + SF_G_misc, lane) + 8u) & SF_MASK_LOW;
    for (unsigned rest = mask; rest; rest &= rest - 1u) {
      const unsigned s = (unsigned)__ffs(rest) - 1u;
      spos[lane][s] = SF_LD(d2_t, sb, sfl::chunk_offset(SF_G_missile_pos, 0) + (size_t)(s * 64u + lane) * 16);
      sang[lane][s] = (unsigned short)SF_LD(unsigned, sb, sfl::chunk_offset(SF_G_missile_meta, 0) + (size_t)(s * 64u + lane) * 4);
    }
  }
  __syncthreads();
  const unsigned wp = pool_rebuild(tb, mask, lane, [&](int s) { return spos[lane][s]; }, [&](int s) { return sang[lane][s]; });
  if (held) {
    for (int p0 = kLsBase; p0 < kLsMis; p0 += 8) {
      u4_t v[8];
#pragma unroll
      for (int j = 0; j < 8; j++) v[j] = p0 + j < kLsMis ? *hold_chunk(sb, p0 + j, lane) : u4_t{0u, 0u, 0u, 0u};
#pragma unroll
      for (int j = 0; j < 8; j++) {
        const int p = p0 + j;
        if (p >= kLsMis) break;
        if (p == kLsBase + SF_G_misc) v[j].z = mask | (wp << SF_MPOOL_SHIFT);
        if (p < kLsShell) *reinterpret_cast<u4_t*>(stage + (p - kLsBase) * 1024 + 16 * lane) = v[j];
        *hold_chunk(tb, p, lane) = v[j];
      }
    }
    if (reward) reward[e] = 0;
    if (done) done[e] = 0;
    if (info) info[e] = 0;
    if (ticks) ticks[e] = 0;
    if (a.events) a.events[e] = 0u;
  } else {
    *reinterpret_cast<unsigned*>(SF_CHUNK(misc, 0) + 16u * lane + 8u) = mask | (wp << SF_MPOOL_SHIFT);
    for (int g = 0; g < 7; g++) *reinterpret_cast<u4_t*>(stage + g * 1024 + 16 * lane) = u4_t{0u, 0u, 0u, 0u};  // (defined values below)
  }
  if (a.hint && lane == 0) a.hint[tile_i] &= ~hmask;
  if (obs != nullptr && a.obs_type != 3) obs_rows_from_stage(a, stage, lane, held, obs, (size_t)e);  // (uniform)
}

// The held lanes' draw records (image batches) from their restored state, behind sf_hold_end_kernel: sf_drawrec_kernel's
// code for the lanes of the mask's zeros; the active lanes' records are the step launch's own and stay.
__global__ __launch_bounds__(64) void sf_hold_drawrec_kernel(const unsigned char* state, int n_envs, const uint8_t* active, unsigned char* draw,
                                                            int pics) {
  __shared__ unsigned near[64];
  const long e = (long)blockIdx.x * 64 + threadIdx.x;
  const unsigned long long hmask = __ballot(e < n_envs && active[e] == 0);
  if (hmask == 0ull) return;  // (uniform)
  drawrec_tile(state, n_envs, draw, pics, hmask, near);
}

// The finished lanes' draw records from their new games, behind sf_finish_lanes_kernel: sf_drawrec_kernel's code for the lanes of
// the done bytes' non-zeros; the others' records are the step launch's own and stay.
__global__ __launch_bounds__(64) void sf_finish_drawrec_kernel(const unsigned char* state, int n_envs, const uint8_t* done, unsigned char* draw,
                                                              int pics) {
  __shared__ unsigned near[64];
  const long e = (long)blockIdx.x * 64 + threadIdx.x;
  const unsigned long long fmask = __ballot(e < n_envs && done[e] != 0);
  if (fmask == 0ull) return;  // (uniform)
  drawrec_tile(state, n_envs, draw, pics, fmask, near);
}

hipError_t sf_launch_finish_lanes(const SfKernelArgs& a, const uint8_t* done, hipStream_t stream) {
  const dim3 grid((unsigned)((a.n_envs + 63) / 64));
  hipLaunchKernelGGL(sf_finish_lanes_kernel, grid, dim3(64), 0, stream, a, done);
  if (a.draw) hipLaunchKernelGGL(sf_finish_drawrec_kernel, grid, dim3(64), 0, stream, a.state, a.n_envs, done, a.draw, a.draw_pics);
  return hipGetLastError();
}

hipError_t sf_launch_hold_begin(const SfKernelArgs& a, const uint8_t* active, unsigned char* stash, hipStream_t stream) {
  hipLaunchKernelGGL(sf_hold_begin_kernel, dim3((unsigned)((a.n_envs + 63) / 64)), dim3(64), 0, stream, a, active, stash);
  return hipGetLastError();
}

// ticks [n] = 1: what a plain step launch, which has no ticks output, says of every env in front of sf_hold_end_kernel.  (A
// kernel, not hipMemsetAsync: as a node of a captured graph the byte memset left other values behind on replay.)
__global__ __launch_bounds__(kBlock) void sf_hold_one_tick_kernel(uint8_t* ticks, int n) {
  const long e = (long)blockIdx.x * kBlock + threadIdx.x;
  if (e < n) ticks[e] = 1;
}

hipError_t sf_launch_hold_end(const SfKernelArgs& a, const uint8_t* active, const unsigned char* stash, void* obs, int32_t* reward,
                              uint8_t* done, uint8_t* info, uint8_t* ticks, int one_tick, hipStream_t stream) {
  const dim3 grid((unsigned)((a.n_envs + 63) / 64));
  if (one_tick && ticks)
    hipLaunchKernelGGL(sf_hold_one_tick_kernel, dim3((unsigned)((a.n_envs + kBlock - 1) / kBlock)), dim3(kBlock), 0, stream, ticks, a.n_envs);
  hipLaunchKernelGGL(sf_hold_end_kernel, grid, dim3(64), 0, stream, a, active, stash, obs, reward, done, info, ticks);
  if (a.draw) hipLaunchKernelGGL(sf_hold_drawrec_kernel, grid, dim3(64), 0, stream, a.state, a.n_envs, active, a.draw, a.draw_pics);
  return hipGetLastError();
}
