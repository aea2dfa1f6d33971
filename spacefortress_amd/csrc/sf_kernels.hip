// sf_kernels.hip -- the env.step() hot path as HIP kernels for gfx950 (MI355X, CDNA4): sf_reset_kernel, sf_step_kernel, their
// launchers.  The state tools are in sf_state_ops.hip, what both share in sf_lane_dev.h.
//
// One lane per environment.  A launch of sf_step_kernel advances every env of the
// batch by one 34 ms tick and does, fused, what the reference spreads over three
// layers and N processes:
//   SSF_Env.step          ENV:208-253   action -> key events, reward shaping, obs
//   Game::stepOneTick     SRC/game.cpp:473-485 and everything it calls
//   vec-env worker loop   rl/train.py:80 (auto-reset on done)
// (SRC = python/spacefortress/src, ENV = python/spacefortress.gym/.../ssf_env.py of
// the reference.)  The step order, the float32 score adds and the double position
// arithmetic follow the reference operation by operation; the file is compiled
// with -ffp-contract=off so that a*b+c rounds twice, as it does in the reference
// build (baseline x86-64, no FMA).
//
// Hardware mapping:
//  * state is struct-of-arrays per 64-env wave tile in HBM (sf_layout.h): a wave's 64
//    lanes read 64 consecutive elements of each field -- every access is a full
//    coalesced row -- and the whole state of the wave hangs off ONE scalar base with
//    compile-time field offsets (the batch-wide SoA first tried spent a quarter of its
//    instructions on per-field 64-bit address arithmetic and SGPR spills);
//  * at 65 536 envs a launch is 1024 waves = ONE wave per SIMD of the chip, so the
//    kernel is a latency chain, not a throughput problem.  It is organised so that a
//    wave makes two memory round trips, not twenty: (1) every unconditional load is
//    issued up front; (2) as soon as the two alive-bitmasks arrive, the live
//    projectile slots are prefetched -- a wave ballot skips slots no lane uses --
//    and their latency hides under the key / ship / fortress arithmetic;
//  * projectile ballistics run as straight-line code over the prefetched slots (the
//    slots are independent until a hit), so their f64 chains interleave; only the
//    rare hit / miss events walk the fortress state machine, in slot order;
//  * the 360-entry cos/sin table (indexed per lane) is staged into LDS once per workgroup (6 KB),
//    BEFORE the predicated loads are issued (any wait behind them is a vmcnt(0)); the hexagon
//    edges and the scalar presets are immediates, what round trip 1 needs of the kernel arguments
//    is preloaded into SGPRs by the command processor;
//  * a lone wave waits out every hand-off between units, so truth values stay in the vector ALU
//    (integer masks, min / max folds, selects instead of small exec-mask branches), constants
//    used per slot live in VGPRs, divisions by constants are three operations;
//  * the four waves of a CU share one address unit: projectile slots, lane chunks and counters go
//    through buffer instructions on a per-wave descriptor (constant part of the address in the
//    scalar offset, idle lanes out of range instead of branched around), what is written once
//    per projectile is one store with the slot in the lane offset;
//  * the per-episode statistics ride in spare bits of words the lane loads and stores anyway (sf_layout.h: SF_W_*): no
//    counter rows, no atomics on the tick; only an episode's END adds its totals to the batch's accumulators with atomics
//    (once per env and 5 295 ticks);
//  * image batches: the tick also leaves the env's draw record for the frame kernel (sf_drawrec.h);
//  * observations are transposed through LDS and leave as 16-byte coalesced stores; every 16-byte
//    store is write-through (sc1), so the end-of-kernel write-back has little left to flush;
//  * no dense contraction anywhere on this path: no MFMA.  The bound is HBM traffic.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <stdint.h>

#include "sf_drawrec.h"
#include "sf_lane_dev.h"  // (with sf_internal.h and sf_layout.h)
#define SF_EVENTS_FN static __device__ __forceinline__
#include "sf_events.h"

// ---- the build's switches: numeric tunables that name a real quantity, and one instrument (SF_STAMPS) ----
// Four waves per workgroup share one LDS copy of the cos/sin table (one barrier, early, while the
// waves are still in step; a copy per wave was tried: 1024 waves pulling the same 45 cache lines
// out of L2 at once made the load phase 3x longer).  Everything after that is wave-private.
#ifndef SF_BLOCK
#define SF_BLOCK 256
#endif
#ifndef SF_SPLIT
#define SF_SPLIT 1 /* 1: batches up to 65 536 envs (at most one games' wave per SIMD) step by split launches (sf_step_kernel, BLKP = 1000 + BLK): A/B 4 096 envs 5.48 -> 5.29 us, 32 768: 6.11 -> 5.89, 65 536: 6.51 -> 6.39; 0: never; 2: every batch the instantiation can serve (tests) */
#endif
#ifndef SF_MROWS
#define SF_MROWS 3 /* rows of the tile's missile pool (64 entries each) loaded up front with the lane's chunks (a split launch's
                      missile wave: those of them the pool reaches); more live missiles than that (> 192 in 64 envs; random
                      play averages 104) take the dependent-load loop */
#endif
#ifndef SF_SPF
#define SF_SPF 6 /* shell slots prefetched, one at a time (A/B at 65 536 envs with the missile pool: pairs 6.82 us per launch, singles 6.75) */
#endif
#ifndef SF_STAGGER
#define SF_STAGGER 12 /* x 64 cycles (sf_step_kernel's staggered start); A/B at 65 536 envs: 0: 7.02 us per launch, 8: 6.84, 16: 6.84, 24: 6.89, 40: 7.36 */
#endif

// LDS map (doubles): [0, SF_LDS_DOUBLES) the cos/sin table; then one (hit, out) pair of 32-bit event words per lane,
// through which the missile pool's entries tell their owner lanes what happened to them; then the observation staging
#define SF_LDS_EV SF_LDS_DOUBLES
/* then (sf_step_kernel: kLdsAtab, kLdsStage) behind the BLK event words: atan(k / 16), k = 0..16 (sf_atan2_core), and the staging rows */
// A split launch stages the WHOLE constants block, [0, SF_LDS_SPLIT_DOUBLES): the cos/sin table, the hexagon edges, the atan
// table and the kernel constants row in one pass; its event words, hand-over words and staging rows follow that (kLdsEv ...).

// Diagnostic build only (-DSF_STAMPS, tools/stamps.py): shader-clock stamps at phase boundaries,
// with forced waits so each phase owns its memory latency.  The product build has none of it.
#if defined(SF_STAMPS) && !defined(SF_STAMPS_LITE)
#define SF_STAMP(k, drain)                                                 \
  do {                                                                     \
    __builtin_amdgcn_sched_barrier(0);                                     \
    if (drain) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); \
    stamp_[k] = __builtin_amdgcn_s_memtime();                              \
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                     \
    __builtin_amdgcn_sched_barrier(0);                                     \
  } while (0)
#else
#define SF_STAMP(k, drain)
#endif

#define SF_COS(ang) trig[2 * (ang)]
#define SF_SIN(ang) trig[2 * (ang) + 1]
#define SF_ST(T, base, off, v) sf_store<T>(reinterpret_cast<T*>((base) + (off)), (T)(v))

// ---- three pieces of sf_step_kernel's tick that a REPEAT launch runs once, behind its tick loop: macros over the kernel's own
//      names, so that the tick of every other instantiation is the text it was (as always_inline lambdas in front of the loop
//      they gave all 108 other instantiations other instructions; as macros none: profiles/frame_skip.md)
// A lane that started a new game while others of its tile play on (only possible when episodes are out of step:
// sf_set_field, a reset of part of a tile; a REPEAT launch: the lanes parked in the window) must take its entries out of the
// shared pool: DN = the ballot of those lanes.  With every lane of the tile done in the same tick -- the regular case -- the
// pool is simply emptied.  (a split launch first waits for the missile wave's acknowledgement of this tick's rows)
#define SF_PURGE_POOL(DN) \
  { \
    const unsigned long long dn_ = (DN); \
    if (dn_ != 0ull) { \
      if (dn_ == ~0ull) { \
        L.mpool = 0; \
      } else { \
        const unsigned n_before = (unsigned)__builtin_amdgcn_readfirstlane((int)L.mpool); \
        unsigned wp = 0; \
        if constexpr (SPLIT) { \
          unsigned spins = 0u; \
          while (__builtin_amdgcn_readfirstlane((int)hflags[2]) == 0 && ++spins < kSpinLimit) __builtin_amdgcn_s_sleep(1); \
          if (spins >= kSpinLimit && lane == 0u) atomicAdd(&a.acc[SF_ACC_HANDOVER], 1ull); \
          asm volatile("" ::: "memory"); \
        } \
_Pragma("unroll 1") \
        for (unsigned r = 0; 64u * r < n_before; r++) { \
          const u4_t pr = __builtin_amdgcn_raw_buffer_load_b128(rs, o.o16 + r * 1024u, SF_GOFF(missile_pos, 0), 16); \
          const unsigned pm = __builtin_amdgcn_raw_buffer_load_b32(rs, o.o4 + r * 256u, SF_GOFF(missile_meta, 0), 16); \
          const bool keep = (64u * r + lane < n_before) && !((dn_ >> SF_MM_OWNER(pm)) & 1ull); \
          const unsigned long long kb = __ballot(keep); \
          const unsigned idx = wp + __builtin_amdgcn_mbcnt_hi((unsigned)(kb >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)kb, 0u)); \
          wp += (unsigned)__popcll(kb); \
          sf_buf_st128<kStAux>(pr, rs, keep ? idx * 16u : SF_OOB, SF_GOFF(missile_pos, 0)); \
          __builtin_amdgcn_raw_buffer_store_b32(pm, rs, keep ? idx * 4u : SF_OOB, SF_GOFF(missile_meta, 0), kStAux); \
        } \
        L.mpool = wp; \
      } \
    } \
  }
// the env's draw record (sf_drawrec.h) -- header, ship, fortress; the missiles' entries go out as the pool is walked.
// NEWGAME: the env starts a new game here (it has no projectiles); PROJ: sfd::hud_flags_near of its projectiles
#define SF_DRAW_HEADER(NEWGAME, PROJ) \
  { \
    typedef float f4_t __attribute__((ext_vector_type(4))); \
    const sfd::Header h = sfd::make_header(L.sx, L.sy, L.angle, (L.fl & SF_FL_SHIP_ALIVE) != 0u, (L.fl & SF_FL_FORT_ALIVE) != 0u, L.fort_angle, \
                                           L.points, L.vlner, L.fort_vuln_t, L.mmask, L.smask, \
                                           (NEWGAME) ? 0u : (PROJ) /* a new game has no projectiles */, a.draw_pics != 0, L.time); \
    const __amdgpu_buffer_rsrc_t rs_dr = __builtin_amdgcn_make_buffer_rsrc( \
        a.draw + (size_t)__builtin_amdgcn_readfirstlane(i >> 6) * (size_t)SF_DR_TILE_BYTES, 0, SF_DR_TILE_BYTES, 0x00020000); \
    const unsigned d0 = real ? lane * (unsigned)SF_DR_LANE_STRIDE : SF_OOB; \
    sf_buf_st128<0>(u4_t{h.w[0], h.w[1], h.w[2], h.w[3]}, rs_dr, d0, 0); \
    sf_buf_st128<0>(u4_t{h.w[4], h.w[5], h.w[6], h.w[7]}, rs_dr, d0, SF_DR_PIECE_STRIDE); \
    sf_buf_st128<0>(__builtin_bit_cast(u4_t, (d2_t{L.sx, L.sy})), rs_dr, d0, (SF_DR_PIECE_OBJ0 + SF_DR_OBJ_SHIP) * SF_DR_PIECE_STRIDE); \
  }
// the lane's observation row, by way of the wave's staging rows, into row ROW (in units of n_envs rows) of the output; BPOS,
// BVEL: the two bearings of the state.  OBSK == 1: the host guarantees features, float32, n_envs % 64 == 0, an aligned output
// (sf_launch_step); the padding waves behind the batch write nothing.  NEWGAME && a.ref_reset_obs: a new game's observation
// as the reference returns it (sf_launch_step keeps such batches out of OBSK == 1)
#define SF_WRITE_OBSERVATION(ROW, BPOS, BVEL, NEWGAME) \
  { \
    if constexpr (OBSK == 1) { \
      constexpr int DIM = AUTOTURN ? 17 : 19; \
      float* stage = reinterpret_cast<float*>(lds + kLdsStage); \
      const Extras e = SPLIT ? compute_extras(a, L, BPOS, BVEL, kc) : compute_extras(a, L, BPOS, BVEL); \
      write_features_f32<DIM>(stage + tid * DIM, L, e, a.real_shell_count); \
      if ((i & ~63u) < (unsigned)n_envs_p) \
        flush_features_f32<DIM>(stage + (tid & ~63u) * DIM, (float*)obs + (ROW + (i & ~63u)) * DIM, lane); \
    } else if (obs != nullptr && a.obs_type != 3) { \
      Extras e = compute_extras(a, L, BPOS, BVEL); \
      if (a.ref_reset_obs && NEWGAME) e = Extras{0.0, 0.0, 0.0}; \
      if (a.obs_f64) { \
        double* stage = lds + kLdsStage; \
        write_obs<double>(a, stage + tid * a.obs_dim, L, e); \
        flush_obs_wave<double>(a, stage + (tid & ~63u) * a.obs_dim, (double*)obs + ROW * a.obs_dim, i & ~63u, lane, \
                               obs_vec_ok); \
      } else { \
        float* stage = reinterpret_cast<float*>(lds + kLdsStage); \
        write_obs<float>(a, stage + tid * a.obs_dim, L, e); \
        flush_obs_wave<float>(a, stage + (tid & ~63u) * a.obs_dim, (float*)obs + ROW * a.obs_dim, i & ~63u, lane, \
                              obs_vec_ok); \
      } \
    } \
  }

namespace {

// What one tick adds to the statistics (SRC/game.hh:29-43); flushed with atomics.
// (Named scalars, not an array: the compiler merges `if (c) d[5]++; else d[4]++;` into a
// dynamically indexed update, which would push an array into scratch memory.)
struct StatDelta {
  int big_hex_deaths = 0, small_hex_deaths = 0, shell_deaths = 0, ship_deaths = 0, resets = 0, destroyed = 0,
      missed = 0, shots = 0, thrusts = 0, lefts = 0, rights = 0, vlner_incs = 0;
  int max_vlner = 0;  // candidate for counter 12 (a running maximum)
};

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the Random123 constants): counter
// (c0, c1, 0, 0), key (k0, k1); the first output word.  The reference's rollout gets its actions from the policy
// (rl/train.py:76-80); the random-action benchmark draws them here: action = floor(x * n_actions / 2^32).
__device__ __forceinline__ unsigned sf_philox4x32_10(unsigned c0, unsigned c1, unsigned k0, unsigned k1) {
  unsigned c2 = 0u, c3 = 0u;
#pragma unroll
  for (int r = 0; r < 10; r++) {
    const unsigned lo0 = 0xD2511F53u * c0, hi0 = __umulhi(0xD2511F53u, c0);
    const unsigned lo1 = 0xCD9E8D57u * c2, hi1 = __umulhi(0xCD9E8D57u, c2);
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c0;
}

// Game::reward (SRC/game.cpp:97-102): three float32 adds in this order, points clamped at 0.
__device__ __forceinline__ void score(float amount, float& rew, Lane& L) {
  rew += amount;
  L.raw += amount;
  L.points += amount;
  if (L.points < 0) L.points = 0;
}

__device__ __forceinline__ void kill_ship(Lane& L, StatDelta& S) {  // SRC/game.cpp:274-280
  if (L.fl & SF_FL_SHIP_ALIVE) {
    L.fl &= ~SF_FL_SHIP_ALIVE;
    L.death_t = 0;
    S.ship_deaths += 1;
  }
}

// Agent-scope (L2-coherent, L1-bypassing) accesses for the few places where one launch may read
// back what it wrote earlier or mixes plain stores with atomics on the same word: the counter
// rows (atomics + the zeroing at a new game) and the dependent-load slow path of the projectile
// slots beyond the prefetched groups (a fused launch reads in tick k+1 what tick k stored).
__device__ __forceinline__ int ld_coherent_i32(const unsigned char* p) {
  return __hip_atomic_load(reinterpret_cast<const int*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ int ld_coherent_i16(const unsigned char* p) {
  return (int16_t)__hip_atomic_load(reinterpret_cast<const unsigned short*>(p), __ATOMIC_RELAXED,
                                    __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ d2_t ld_coherent_d2(const unsigned char* p) {
  const unsigned long long* q = reinterpret_cast<const unsigned long long*>(p);
  const unsigned long long x = __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned long long y = __hip_atomic_load(q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return d2_t{__longlong_as_double((long long)x), __longlong_as_double((long long)y)};
}
__device__ __forceinline__ void st_coherent_i32(unsigned char* p, int v) {
  __hip_atomic_store(reinterpret_cast<int*>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The default observation -- obs_type 'features', float32, full waves, 16-byte aligned output -- with everything
// the generic path decides at run time fixed at compile time (OBSK = 1 instantiations of the step kernel): DIM
// stores into the wave's staging rows at constant offsets, then the wave's 64 rows (one contiguous span of
// 64 * DIM floats, in LDS and in global memory alike) leave as 16-byte pieces: all LDS reads issued, then all stores.
template <int DIM>
__device__ __forceinline__ void write_features_f32(float* o, const Lane& L, const Extras& e, int real_shell_count) {
  const int n_missiles = __popc(L.mmask);
  const int n_shells = real_shell_count ? __popc(L.smask) : n_missiles;  // SRC/pymodule.cpp:131-134
  const int kill_ready = (L.vlner > 10 && L.fort_vuln_t < sfc::vuln_time) ? 1 : 0;
  const int timers[4] = {L.fire_t, L.thrust_t, L.left_t, L.right_t};
  o[0] = (L.fl & SF_FL_SHIP_ALIVE) ? 1.0f : 0.0f;  // ENV:134-157, as in write_obs
  o[1] = (float)L.sx;
  o[2] = (float)L.sy;
  o[3] = (float)L.vx;
  o[4] = (float)L.vy;
  o[5] = (float)L.angle;
  o[6] = (float)e.aim;
  o[7] = (float)e.vdir;
  o[8] = (float)e.ndist;
  o[9] = (L.fl & SF_FL_FORT_ALIVE) ? 1.0f : 0.0f;
  o[10] = (float)L.fort_angle;
  o[11] = (float)L.vlner;
  o[12] = (float)kill_ready;
  o[13] = (float)n_missiles;
  o[14] = (float)n_shells;
#pragma unroll
  for (int k = 0; k < DIM - 15; k++) o[15 + k] = (float)timers[k];
}
template <int DIM>
__device__ __forceinline__ void flush_features_f32(const float* stage_w, float* dst_w, unsigned lane) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  typedef float f4_t __attribute__((ext_vector_type(4)));
  constexpr int NV = 64 * DIM / 4, IT = (NV + 63) / 64;  // 304 pieces of 16 bytes (DIM 19), 272 (DIM 17)
  f4_t v[IT];
#pragma unroll
  for (int k = 0; k < IT; k++)
    if (k * 64 + 63 < NV || (int)lane + k * 64 < NV) v[k] = reinterpret_cast<const f4_t*>(stage_w)[lane + k * 64];
#pragma unroll
  for (int k = 0; k < IT; k++)
    if (k * 64 + 63 < NV || (int)lane + k * 64 < NV) {
      sf_store<f4_t>(reinterpret_cast<f4_t*>(dst_w) + lane + k * 64, v[k]);  // write-through, like the state chunks
    }
}

// A wave's 64 observation rows sit in ITS OWN piece of LDS as [lane][obs_dim]; global memory wants
// exactly the same order ([N, obs_dim] row-major), so the wave's rows form one contiguous span:
// copy it with 16-byte lanes-consecutive stores instead of obs_dim strided 4-byte stores per lane.
// Wave-private on purpose: no workgroup barrier, so a fast wave never waits for the divergence
// tail of a slower one (LDS is in-order per wave; the fence only pins the compiler).
template <typename T>
__device__ __forceinline__ void flush_obs_wave(const SfKernelArgs& a, const T* stage_w, T* obs, unsigned wave_env0,
                                               unsigned lane, bool vec_ok) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  long rows = (long)a.n_envs - (long)wave_env0;
  if (rows > 64) rows = 64;
  if (rows <= 0) return;
  const int total = (int)rows * a.obs_dim;
  T* dst = obs + (size_t)wave_env0 * a.obs_dim;
  constexpr int V = 16 / (int)sizeof(T);
  int done_elems = 0;
  if (vec_ok) {
    typedef T vec_t __attribute__((ext_vector_type(V)));
    const int nvec = total / V;
    for (int v = lane; v < nvec; v += 64) {
      sf_store<vec_t>(reinterpret_cast<vec_t*>(dst) + v, reinterpret_cast<const vec_t*>(stage_w)[v]);
    }
    done_elems = nvec * V;
  }
  for (int t = done_elems + lane; t < total; t += 64) dst[t] = stage_w[t];
}

// VecNormalize's batch sums for this wave's rows, from the observation tile the wave has just flushed (it is
// still in the wave's private piece of LDS): lanes [g*dim, (g+1)*dim) add every groups-th row of feature
// lane % dim and of its square; the tile is then reused to fold the groups.  One row of the column-major
// partial-sum array per wave (sf_normalize.hip adds the rows up); no workgroup barrier.
template <typename T>
__device__ __forceinline__ void norm_partials_wave(const SfKernelArgs& a, T* stage_w, unsigned wave_env0, unsigned lane,
                                                   double my_ret, bool has_obs) {
  const int dim = a.obs_dim, groups = 64 / dim;
  const size_t waves = (size_t)(a.lanes / 64), w = wave_env0 >> 6;
  long rows = (long)a.n_envs - (long)wave_env0;
  rows = rows > 64 ? 64 : (rows < 0 ? 0 : rows);
  double s = 0, q = 0;
  if (has_obs && (int)lane < groups * dim)
    for (int r = (int)lane / dim; r < rows; r += groups) {
      const double v = (double)stage_w[r * dim + (int)lane % dim];
      s += v;
      q += v * v;
    }
  __builtin_amdgcn_wave_barrier();
  double* fold = reinterpret_cast<double*>(stage_w);  // 2 x 64 doubles <= 64 rows x dim x sizeof(T) for dim >= 4
  if (has_obs) {
    fold[lane] = s;
    fold[64 + lane] = q;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  if ((int)lane < dim) {
    double ts = 0, tq = 0;
    if (has_obs)
      for (int g = 0; g < groups; g++) {
        ts += fold[g * dim + lane];
        tq += fold[64 + g * dim + lane];
      }
    a.n_partials[(size_t)lane * waves + w] = ts;
    a.n_partials[(size_t)(dim + 1 + lane) * waves + w] = tq;
  }
  double rs = (long)lane < rows ? my_ret : 0.0, rq = rs * rs;
  for (int o = 32; o > 0; o >>= 1) {
    rs += __shfl_xor(rs, o);
    rq += __shfl_xor(rq, o);
  }
  if (lane == 0) {
    a.n_partials[(size_t)dim * waves + w] = rs;
    a.n_partials[(size_t)(2 * dim + 1) * waves + w] = rq;
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// VecEnv.reset(): a brand-new Game in every lane (ENV:163-178).  first != 0 additionally
// initialises what SSF_Env.__init__ sets once (prev_vlner, ENV:92) and the spawn cursors.
__global__ __launch_bounds__(SF_BLOCK) void sf_reset_kernel(SfKernelArgs a, int first, unsigned cursor0,
                                                           unsigned cursor_stride, void* obs) {
  const unsigned i = blockIdx.x * SF_BLOCK + threadIdx.x;
  const unsigned lane = threadIdx.x & 63u;
  unsigned char* const tb = a.state + (size_t)__builtin_amdgcn_readfirstlane(i >> 6) * sfl::kTileBytes;
  const Off o = {lane * 16u, lane * 8u, lane * 4u, lane * 2u, lane};
  Lane L;
  if (first) {
    L.prev_vlner = 0;
    L.cursor = cursor0 + cursor_stride * i;
  } else {
    const i4_t mi = SF_LD(i4_t, SF_CHUNK(misc, 0), o.o16);
    L.prev_vlner = SF_LD(int, SF_CHUNK(timers_a, 0), o.o16) & 0xFFF;
    L.cursor = (unsigned)mi.y;
  }
  new_game(a, L);
  L.mpool = 0;  // every env of the tile starts over: the tile's missile pool is empty
  store_lane(tb, o, L);
  if (obs != nullptr && i < (unsigned)a.n_envs && a.obs_type != 3) {
    // new_game_extras (sf_lane_dev.h), spelled out: inlined as a function, this kernel's selects come out in another order
    // (profiles/state_ops_split.md).  A one-line clean-up for the change that next alters this kernel on purpose.
    Extras e = compute_extras(a, L, sf_atan2<true>(L.sy - sfc::fort_y, L.sx - sfc::fort_x), sf_atan2<false>(L.vy, L.vx));
    if (a.ref_reset_obs) e = Extras{0.0, 0.0, 0.0};
    write_obs_row(a, obs, i, L, e);
  }
}

// ---------------------------------------------------------------------------------------------
// FUSED = false: one tick per launch (sf_step, the VecEnv.step path).
// FUSED = true:  n_steps ticks per launch with the actions of all of them given up front
// (sf_rollout): the wave keeps its state in registers between ticks, so a tick costs neither the
// two memory round trips nor a kernel boundary.  Same body, bit-identical results.
// XTRA = the launch may need what the plain VecEnv.step never does -- actions drawn in the kernel (SF_ACT_SAMPLED), the
// played actions written out (a.act_out), the packed counters' overflow test of batches without auto-reset: three uniform
// tests and their code, 0.07 us of a 6.5 us launch when they sit in the one kernel everybody runs (A/B, tools/ab.py)
// FOBS = an XTRA launch that also writes the finished games' last observations (a.final_obs, sf_set_final_obs_output).  A flag
// of its own: inside the XTRA instantiations the row's code cost them 4 to 8 VGPRs, and the 64-thread ones of autoturn a wave
// of occupancy, with the output off (profiles/final_obs.md); so they stay what they were, instruction for instruction.
// BLK = threads per workgroup (64, 128 or 256: one to four tiles).  256 is what the metric's batch wants (65 536 envs = 256
// workgroups, one per CU, the cos/sin table staged once per four waves); a batch of 16 384 envs is 256 waves all the same, and
// as 64 workgroups of four it leaves three CUs in four idle while the four waves of a CU share its address unit and LDS:
// launched as 256 workgroups of ONE wave the same step takes 7.0 instead of 8.0 us (image batch, draw records included;
// sf_launch_step picks the smallest BLK that still fills every CU).
// BLKP = 1000 + BLK is a SPLIT launch: BLK envs per workgroup and a second wave per tile that moves the tile's missile pool
// while the first plays the 64 games (see "the tile's MISSILE wave" below); what sf_launch_step takes for the plain step of the
// default observation of batches up to 65 536 envs (beyond, a SIMD has several games' waves to interleave anyway).
// BLKP = 2000 + BLK is a REPEAT launch (sf_step_repeat: action repeat, frame skip): the fused tick loop on ONE action per env,
// one row of outputs behind it, an env whose game ends inside the window parked for the rest of it (see "a REPEAT launch" in
// front of the tick loop).  It rides on FUSED = XTRA = true at BLK 256 and tests a.final_obs at run time: AUTOTURN x SHAPED x
// OBSK instantiations of their own, spelled in BLKP and not as one more template flag so that every other instantiation keeps
// its symbol as well as its instructions (profiles/frame_skip.md).
template <bool AUTOTURN, bool SHAPED, bool FUSED, int OBSK, bool XTRA, int BLKP, bool FOBS = false>
__global__ __launch_bounds__(BLKP > 2000 ? BLKP - 2000 : (BLKP > 1000 ? 2 * (BLKP - 1000) : BLKP)) void sf_step_kernel(unsigned char* state_p, const double* consts_p,
                                                          const void* actions, int n_envs_p, int act_type,
                                                          int32_t* reward_out, uint8_t* done_out, uint8_t* info_out,
                                                          SfKernelArgs a, void* obs, int obs_vec_ok, int n_steps) {
  // The five leading parameters (= a.state, a.consts, the actions, a.n_envs, the action type) are what round trip 1
  // needs; the library is built with -amdgpu-kernarg-preload-count=8, so the command processor hands them over in
  // SGPRs at wave launch and the state loads issue without a scalar-load round trip to the kernel-argument
  // segment first (on a firmware without the feature the compiler's compatibility preamble loads them).  The
  // three output pointers ride along: the epilogue then stores without a scalar load and its wait.
  // BLKP = 1000 + BLK: a SPLIT launch -- BLK envs per workgroup and as many threads again, the tiles' MISSILE waves (below)
  // BLKP = 2000 + BLK: a REPEAT launch (sf_step_repeat) -- n_steps ticks of ONE action per env, one row of outputs (below)
  constexpr bool REPEAT = BLKP > 2000;
  constexpr bool SPLIT = BLKP > 1000 && !REPEAT;
  constexpr int BLK = REPEAT ? BLKP - 2000 : (SPLIT ? BLKP - 1000 : BLKP);  // envs per workgroup
  constexpr int NT = SPLIT ? 2 * BLK : BLK;        // threads per workgroup
  // A launch of one tick at the full workgroup size (batches beyond 32 768 envs: 4 or 4 + 4 waves on every CU) stores a chunk
  // of the lane when its last writer has run -- see the ship's stores below.  Smaller workgroups leave the CU's address
  // unit no burst to relieve; there the early stores measured level to +0.02 us per launch and the tick ends with
  // store_lane_buf as before (profiles/step_wave_ends.md).
  constexpr bool kEarlySt = !FUSED && BLK == SF_BLOCK;
  static_assert(!SPLIT || (!FUSED && OBSK == 1 && !XTRA), "the split launch exists for the plain step of the default observation");
  static_assert(!FOBS || XTRA, "the final-observation output rides on the XTRA instantiations");
  static_assert(!REPEAT || (FUSED && XTRA && !FOBS && BLK == SF_BLOCK), "the action repeat rides on the fused XTRA instantiations (a.final_obs: a run-time test)");
  // what the workgroup stages into LDS in its one table pass: the cos/sin table; a split launch: the whole constants block --
  // the hexagon edges, the atan table and the kernel constants row sit right behind the cos/sin table, and 401 pieces of 16
  // bytes fit the pass that moved 360 (512 threads: one piece each, as before; 256: two; 128: four instead of three plus the
  // games' wave's atan piece).  The games' wave's own load of the atan table and its LDS write are gone with it.
  constexpr int kStaged = SPLIT ? SF_LDS_SPLIT_DOUBLES : SF_LDS_DOUBLES;
  constexpr int kTrigPieces = (kStaged / 2 + NT - 1) / NT;
  // (the LDS map above, for BLK envs; a split launch's: the staged block with the atan table inside it, the event words, then
  //  the hand-over words in front of the staging rows: the new missiles' (x, y) [BLK d2_t] and meta words [BLK], the
  //  fortress's shots' (ship - fortress) [BLK d2_t] and slot words [BLK], then four words per tile: fired, pool done | count,
  //  stores done, shot.  sf_launch_step's lds_bytes is this map's end.)
  constexpr int kLdsEv = kStaged;
  constexpr int kLdsAtab = SPLIT ? SF_CONST_ATAB : kLdsEv + BLK, kLdsHand = SPLIT ? kLdsEv + BLK : kLdsAtab + SF_ATAB_DOUBLES,
                kLdsHandMeta = kLdsHand + 2 * BLK, kLdsShot = kLdsHandMeta + BLK / 2, kLdsShotSlot = kLdsShot + 2 * BLK,
                kLdsHandFlags = SPLIT ? kLdsShotSlot + BLK / 2 : kLdsHandMeta + BLK / 2, kLdsStage = SPLIT ? kLdsHandFlags + BLK / 32 : kLdsHand;
  static_assert(kLdsEv == SF_LDS_EV || SPLIT, "the other kernels' map is the one above");
  static_assert(kStaged % 2 == 0 && kLdsAtab % 2 == 0 && kLdsHand % 2 == 0 && kLdsShot % 2 == 0 && kLdsStage % 2 == 0, "16-byte LDS accesses");
  extern __shared__ double lds[];  // [SF_LDS_DOUBLES] cos/sin table, the event words, then the obs staging rows (SF_LDS_*)
  const unsigned tid_all = threadIdx.x;
  const unsigned tid = SPLIT ? (tid_all & (unsigned)(BLK - 1)) : tid_all;  // the env of the workgroup this thread works for
  const unsigned i = blockIdx.x * BLK + tid;  // env index: actions and outputs
  const unsigned lane = tid & 63u;
  // this wave's tile: wave-uniform by construction, made scalar for the compiler
  unsigned char* const tb = state_p + (size_t)__builtin_amdgcn_readfirstlane(i >> 6) * sfl::kTileBytes;
  const Off o = {lane * 16u, lane * 8u, lane * 4u, lane * 2u, lane};  // lane offsets inside the tile's rows
  const Off g = {i * 16u, i * 8u, i * 4u, i * 2u, i};     // env offsets into the caller's arrays
  const bool real = i < (unsigned)n_envs_p;  // lanes in [n_envs, lanes) are padding: they run NOOPs
  // predicated access to one projectile slot of the lane: `goff` = SF_GOFF(group, slot), wave-uniform
  const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(tb, 0, (int)sfl::kTileBytes, 0x00020000);
  constexpr int kStAux = SF_SC_AUX;
  auto pld16 = [&](unsigned goff, bool p) __attribute__((always_inline)) -> d2_t {
    return __builtin_bit_cast(d2_t, __builtin_amdgcn_raw_buffer_load_b128(rs, p ? o.o16 : SF_OOB, goff, 0));
  };
  auto pst16 = [&](unsigned goff, bool p, d2_t v) __attribute__((always_inline)) {
    sf_buf_st128<kStAux>(__builtin_bit_cast(u4_t, v), rs, p ? o.o16 : SF_OOB, goff);
  };
  // the same with a per-lane slot offset (`extra` = slot * row bytes)
  auto pst16_at = [&](unsigned goff, bool p, unsigned extra, d2_t v) __attribute__((always_inline)) {
    sf_buf_st128<kStAux>(__builtin_bit_cast(u4_t, v), rs, p ? o.o16 + extra : SF_OOB, goff);
  };
#ifdef SF_STAMPS
  unsigned long long stamp_[SF_STAMP_SLOTS] = {};
  stamp_[12] = __builtin_amdgcn_s_memrealtime();
#endif
  SF_STAMP(0, false);

#if SF_STAGGER
  // Half of the workgroups (every other one of an XCD's: workgroup i runs on XCD i % 8) start a third of a microsecond
  // late: a launch is a chip-wide load burst, then arithmetic with the fabric idle, then a store burst; staggered, one
  // half's bursts meet the other half's arithmetic.
  // (a batch that leaves CUs idle has no burst to split; the batch size is a preloaded kernel argument, gridDim is a load)
  if (n_envs_p > 65536 - 256 && ((blockIdx.x >> 3) & 1u)) __builtin_amdgcn_s_sleep(SF_STAGGER);
#endif
  // A poll of a hand-over word gives up after 2^18 rounds of 64+ cycles (10 ms; a launch lasts 6 us): a kernel must end
  // whatever happens to the other wave.  Giving up is counted (SF_ACC_HANDOVER -> sf_check_state fails: the step is wrong).
  constexpr unsigned kSpinLimit = 1u << 18;
  typedef volatile __attribute__((address_space(3))) unsigned lds_word_t;  // (named as LDS: a volatile access through a generic pointer is a flat_load)
  lds_word_t* const hflags = (lds_word_t*)(reinterpret_cast<unsigned*>(lds + kLdsHandFlags) + 4u * (tid >> 6));  // (split launches: this tile's hand-over words)
  if constexpr (SPLIT) {
    // ================= the tile's MISSILE wave =================
    // At the metric's batch a wave is alone on its SIMD and everything it does is one dependent chain; the missile pool --
    // move, test, compact 64 entries a row, whoever owns them -- depends on the 64 games only through the missiles fired
    // this tick, and the games depend on it only through the owners' event words.  A split launch gives every tile a
    // second wave (threads BLK .. 2 BLK - 1 of the workgroup: wave w + BLK / 64 works for wave w's tile; with 256 envs per
    // workgroup on the same SIMD, with fewer on one of the CU's idle ones) that does
    // exactly that part under the first wave's ship / fortress / shell arithmetic.  Hand-over through LDS, both ways by a
    // word the other side polls (a workgroup barrier would make the games wait for the pool's loads): the games' wave
    // files its new missiles and sets `fired`; the missile wave sets `done | entries kept` behind its last event word.
    // Both waves of a workgroup are resident before either starts, each sets its word on every path, the polls sleep.
    // What it buys is the first wave's issue bubbles, not the missiles' whole cost (removing them: -0.68 us; moving them
    // here: -0.12): in its arithmetic the first wave keeps the SIMD's one VALU busy most of the time, and the second wave's
    // instructions take the same issue slots.  Issue priority for the first wave and a later start for the pool's loads
    // changed nothing measurable; starting them 1 500 cycles later made the games wait; asked for without waiting for the
    // pool's count: nothing either (tools/ab.py, NOTES.md, profiles/r04_split_ab.txt, profiles/closed_switches.md).
    // It also fires the fortress's shell: the games' wave keeps the decision (updateFortress) and files the ship's offset
    // from the fortress and the slot, word `shot`; the sqrt, the two divisions and the shell's two stores happen here, behind
    // the `done` word, in issue slots the games' wave leaves free (profiles/step_shell_fire.md).
    // With the word already set, the games' wave's poll of `done` (stamps 16 -> 17 of the instrument build) costs 280
    // cycles: one LDS read and its hand-off to the scalar unit.  That was all it took while the missile events were replayed
    // in a loop (profiles/step_handover_fill.md: the tick's independent tail in front of the poll had nothing to hide in,
    // +0.09 us per launch); since the closed form the two waves reach the hand-over neck and neck
    // (profiles/step_outcomes.md, profiles/step_shell_fire.md).
    if (tid_all >= (unsigned)BLK) {  // wave-uniform
      // the pool's count rides in every lane's misc chunk: lane 0's word, by a scalar load
      const unsigned n_word = *reinterpret_cast<const __attribute__((address_space(4))) unsigned*>(
          reinterpret_cast<const __attribute__((address_space(4))) void*>(
              (unsigned long long)(tb + (unsigned)sfl::chunk_offset(SF_G_misc, 0) + 8u)));
      unsigned cpi0[kTrigPieces];  // (this wave's share of the cos/sin table's pieces: one with 512 threads, up to three)
      d2_t cst0[kTrigPieces];
#pragma unroll
      for (int k = 0; k < kTrigPieces; k++) {
        cpi0[k] = min(tid_all + k * NT, (unsigned)(kStaged / 2 - 1));
        cst0[k] = SF_LD(d2_t, (const unsigned char*)consts_p, cpi0[k] * 16u);
      }
      const unsigned m_live = n_word >> SF_MPOOL_SHIFT;
      d2_t prow[SF_MROWS];
      unsigned pmeta[SF_MROWS];
#pragma unroll
      for (int k = 0; k < kTrigPieces; k++) reinterpret_cast<d2_t*>(lds)[cpi0[k]] = cst0[k];
      if (lane < 4u) hflags[lane] = 0u;
      asm volatile("" ::: "memory");
      // A row the pool does not reach is not asked for at all: the count is scalar, the test a scalar branch (no exec
      // mask), and an instruction that moves no bytes still takes its turn at the CU's one address unit (random play keeps
      // 2 rows of the 3 in use: 8 instructions less per CU and tick; A/B at 65 536 envs 6.40 -> 6.28 us per launch,
      // profiles/step_handover_fill.md).  Behind the table's LDS write, as before: the compiler cannot count loads it does
      // not see issued, so a wait for the table placed behind them would be a wait for them too, in front of the barrier.
      // (a skipped row's position registers are never used: m_row runs behind the same test; its meta word is 0, so the
      //  heading looked up for it below is entry 0 of the table)
#pragma unroll
      for (int r = 0; r < SF_MROWS; r++) {
        asm volatile("" : "=v"(prow[r].x), "=v"(prow[r].y));
        pmeta[r] = 0u;
        if (m_live > 64u * r) {
          const bool in_ = 64u * r + lane < m_live;
          prow[r] = __builtin_bit_cast(d2_t, __builtin_amdgcn_raw_buffer_load_b128(rs, in_ ? o.o16 : SF_OOB, SF_GOFF(missile_pos, r), 0));
          pmeta[r] = __builtin_amdgcn_raw_buffer_load_b32(rs, in_ ? o.o4 : SF_OOB, SF_GOFF(missile_meta, r), 0);
        }
      }
      __syncthreads();  // (the workgroup's one barrier: the cos/sin table is in LDS, the hand-over words are zero)
      // (the rows' first use stays behind the barrier: moved in front of it, it is the wait for them the line above avoids)
#pragma unroll
      for (int r = 0; r < SF_MROWS; r++) asm volatile("" : "+v"(pmeta[r]));
      const double* trig = lds;
      d2_t pcs[SF_MROWS];
#pragma unroll
      for (int r = 0; r < SF_MROWS; r++) pcs[r] = *reinterpret_cast<const d2_t*>(&trig[2 * SF_MM_ANGLE(pmeta[r])]);
      double kv_speed = sfc::missile_speed, kv_fx = sfc::fort_x, kv_fy = sfc::fort_y, kv_w = sfc::width_d, kv_h = sfc::height_d,
             kv_mr2 = sfc::missile_hit_r2;
      asm volatile("" : "+v"(kv_speed), "+v"(kv_fx), "+v"(kv_fy), "+v"(kv_w), "+v"(kv_h), "+v"(kv_mr2));
      unsigned wp = 0;
      unsigned* const evw32 = reinterpret_cast<unsigned*>(lds + kLdsEv) + 2u * (tid & ~63u);
      auto m_row = [&](double x, double y, unsigned meta, d2_t cs, bool valid) __attribute__((always_inline)) {  // (as below)
        const double nx = x + kv_speed * cs.x, ny = y + kv_speed * cs.y;
        const double dx = nx - kv_fx, dy = ny - kv_fy;
        const bool hit = valid & (dx * dx + dy * dy <= kv_mr2);
        const bool gone = valid & (hit | (__builtin_fmax(__builtin_fmax(-nx, nx - kv_w), __builtin_fmax(-ny, ny - kv_h)) > 0));
        if (__ballot(gone) != 0ull) {
          if (gone)
            __hip_atomic_fetch_or(evw32 + 2 * SF_MM_OWNER(meta) + (hit ? 0 : 1), 1u << SF_MM_SLOT(meta), __ATOMIC_RELAXED,
                                  __HIP_MEMORY_SCOPE_WORKGROUP);
        }
        const bool keep = valid & !gone;
        const unsigned long long kb = __ballot(keep);
        const unsigned idx = wp + __builtin_amdgcn_mbcnt_hi((unsigned)(kb >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)kb, 0u));
        wp += (unsigned)__popcll(kb);
        sf_buf_st128<kStAux>(__builtin_bit_cast(u4_t, (d2_t{nx, ny})), rs, keep ? idx * 16u : SF_OOB,
                                               SF_GOFF(missile_pos, 0));
        __builtin_amdgcn_raw_buffer_store_b32(meta, rs, keep ? idx * 4u : SF_OOB, SF_GOFF(missile_meta, 0), kStAux);
      };
#pragma unroll
      for (int r = 0; r < SF_MROWS; r++)
        if (m_live > 64u * r) m_row(prow[r].x, prow[r].y, pmeta[r], pcs[r], 64u * r + lane < m_live);
      if (m_live > 64u * SF_MROWS) {
#pragma unroll 1
        for (unsigned r = SF_MROWS; 64u * r < m_live; r++) {
          const d2_t pr = __builtin_bit_cast(d2_t, __builtin_amdgcn_raw_buffer_load_b128(rs, o.o16 + r * 1024u, SF_GOFF(missile_pos, 0), 16));
          const unsigned pm = __builtin_amdgcn_raw_buffer_load_b32(rs, o.o4 + r * 256u, SF_GOFF(missile_meta, 0), 16);
          m_row(pr.x, pr.y, pm, *reinterpret_cast<const d2_t*>(&trig[2 * SF_MM_ANGLE(pm)]), 64u * r + lane < m_live);
        }
      }
      // the missiles fired this tick (SRC/game.cpp:237-238), one more row, lane = owner
      unsigned fired, spins = 0u;
      while ((fired = (unsigned)__builtin_amdgcn_readfirstlane((int)hflags[0])) == 0u && ++spins < kSpinLimit) __builtin_amdgcn_s_sleep(1);
      if (spins >= kSpinLimit && lane == 0u) atomicAdd(&a.acc[SF_ACC_HANDOVER], 1ull);  // (never seen; see kSpinLimit)
      asm volatile("" ::: "memory");
      if (fired == 2u) {
        const d2_t nxy = reinterpret_cast<const d2_t*>(lds + kLdsHand)[tid];
        const unsigned nm = reinterpret_cast<const unsigned*>(lds + kLdsHandMeta)[tid];
        m_row(nxy.x, nxy.y, nm & 0x7FFFFFFFu, *reinterpret_cast<const d2_t*>(&trig[2 * SF_MM_ANGLE(nm)]), !(nm >> 31));
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the event words are in
      if (lane == 0u) hflags[1] = 0x80000000u | wp;
      // the shell the fortress fires this tick (fireShell, SRC/game.cpp:159-173), BEHIND the `done` word, so that the games
      // never wait for it: the games' wave decides (updateFortress below) and files (ship - fortress) and the slot per lane,
      // then sets `shot`, usually long before this poll; the arithmetic -- one sqrt, two fp64 divisions -- and the shell's two
      // stores are done here.  vel = shellSpeed * d / |d|, pos = fortress + vel: the same operations on the same values in the
      // same order as the games' wave of the other launches performs them, so the same bits.
      static_assert(sfl::kGroups[SF_G_shell_vel].chunk * sfl::kTileLanes == 1024 && sfl::kGroups[SF_G_shell_pos].chunk * sfl::kTileLanes == 1024,
                    "slot stride of the two stores below");
      unsigned shot;
      spins = 0u;
      while ((shot = (unsigned)__builtin_amdgcn_readfirstlane((int)hflags[3])) == 0u && ++spins < kSpinLimit) __builtin_amdgcn_s_sleep(1);
      if (spins >= kSpinLimit && lane == 0u) atomicAdd(&a.acc[SF_ACC_HANDOVER], 1ull);  // (never seen; see kSpinLimit)
      asm volatile("" ::: "memory");
      if (shot == 2u) {
        const d2_t dd = reinterpret_cast<const d2_t*>(lds + kLdsShot)[tid];
        const unsigned sl = reinterpret_cast<const unsigned*>(lds + kLdsShotSlot)[tid];  // the slot (< SF_NSLOT), or bit 31: no shot
        const double nrm = sqrt(dd.x * dd.x + dd.y * dd.y);
        const double svx = sfc::shell_speed * (dd.x / nrm), svy = sfc::shell_speed * (dd.y / nrm);
        const unsigned so = !(sl >> 31) ? o.o16 + sl * 1024u : SF_OOB;
        sf_buf_st128<kStAux>(__builtin_bit_cast(u4_t, (d2_t{svx, svy})), rs, so, SF_GOFF(shell_vel, 0));
        sf_buf_st128<kStAux>(__builtin_bit_cast(u4_t, (d2_t{kv_fx + svx, kv_fy + svy})), rs, so, SF_GOFF(shell_pos, 0));
      }
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the pool's rows and the new shell are written (the rare purge below re-reads the rows)
      if (lane == 0u) hflags[2] = 1u;
      return;
    }
  }
  // ================= round trip 1: every unconditional load =================
  // act_type SF_ACT_SAMPLED: no action array -- `actions` is this batch's sampler records (SfActRec, one per tile) and the
  // lane draws its action itself: Philox4x32-10 keyed by the seed, counter (lane of the whole job, tick).  The record is
  // ONE scalar load off a preloaded kernel argument, back long before the early set, and the ten rounds run while the
  // wave would otherwise sit in that wait.  (constant address space = s_load; the tile's tick is rewritten by lane 0 after
  // the last tick of the launch, nothing reads it again in between.)
  u4_t act_rec = {0u, 0u, 0u, 0u};
  if (XTRA && act_type == SF_ACT_SAMPLED)
    act_rec = *(reinterpret_cast<const __attribute__((address_space(4))) u4_t*>(
                    reinterpret_cast<const __attribute__((address_space(4))) void*>((unsigned long long)actions)) +
                __builtin_amdgcn_readfirstlane(i >> 6));
  // (its own variable, never the destination of a load: joined with the loaded action in one register, the compiler
  //  waits for every outstanding load -- vmcnt(0) -- in front of the ten rounds instead of running them under that wait)
  auto sample_action = [&](int step) __attribute__((always_inline)) -> int {
    const unsigned x = sf_philox4x32_10(act_rec.w + lane, act_rec.x + (unsigned)step, act_rec.y, act_rec.z);
    return real ? (int)__umulhi(x, (unsigned)a.n_actions) : 0;
  };
  auto load_action = [&](int step) __attribute__((always_inline)) -> int {  // ENV:211-212
    if (!real || (XTRA && act_type == SF_ACT_SAMPLED)) return 0;
    const unsigned char* ab = (const unsigned char*)actions;
    const unsigned e = (unsigned)step * (unsigned)n_envs_p + i;
    if (act_type == 8) return (int)SF_LD(long long, ab, e * 8u);
    if (act_type == 4) return SF_LD(int, ab, e * 4u);
    return SF_LD(unsigned char, ab, e);
  };
  // ---- the early set: what keys, respawn and ship need (load_lane_early), the action, the cos/sin table pieces
  Lane L;
  load_lane_early(tb, o, L);  // before the action: its address needs two more kernel arguments and a branch on the action type
  int act_next = load_action(0);
  // (the atan table: nine pieces of its own; a split launch has it in the block its threads stage below, and no load here)
  const unsigned atab_pi = min(tid, (unsigned)(SF_ATAB_DOUBLES / 2 - 1));
  const d2_t atab_piece = SPLIT ? d2_t{0, 0} : SF_LD(d2_t, (const unsigned char*)consts_p, (SF_CONST_ATAB / 2 + atab_pi) * 16u);
  // cos/sin table: 720 doubles = 360 16-byte pieces, six per lane (the last one partial)
  const unsigned char* cb = (const unsigned char*)consts_p;
  // (threads past the end re-load and re-store the last piece: straight-line code, no exec-masked
  // branches for the compiler's wait-count insertion to be conservative about)
  d2_t cst[kTrigPieces];
  unsigned cpi[kTrigPieces];
#pragma unroll
  for (int k = 0; k < kTrigPieces; k++) {
    cpi[k] = min(tid_all + k * NT, (unsigned)(kStaged / 2 - 1));
    cst[k] = SF_LD(d2_t, cb, cpi[k] * 16u);
  }
  // (behind the last load of the early set: the ten rounds run while those are in flight)
  int act_sampled = 0;
  if (XTRA && act_type == SF_ACT_SAMPLED) act_sampled = sample_action(0);  // uniform branch, VALU only
  // lane l takes entry 64 r + l if the pool has that many (`n_pool`: the tile's count, known once the early set is in):
  // the instructions are unconditional, the bytes are not
#define SF_LOAD_POOL_ROWS(aux, n_pool)                                                                                        \
  _Pragma("unroll") for (int r = 0; r < SF_MROWS; r++) {                                                                      \
    const bool in_ = 64u * r + lane < (n_pool);                                                                               \
    prow[r] = __builtin_bit_cast(d2_t, __builtin_amdgcn_raw_buffer_load_b128(rs, in_ ? o.o16 : SF_OOB, SF_GOFF(missile_pos, r), (aux)));   \
    pmeta[r] = __builtin_amdgcn_raw_buffer_load_b32(rs, in_ ? o.o4 : SF_OOB, SF_GOFF(missile_meta, r), (aux));               \
  }
  constexpr bool kPoolLoads = !SPLIT;
  d2_t prow[SF_MROWS];
  unsigned pmeta[SF_MROWS];
  LaneLate late;
  SF_STAMP(1, false);
  SF_STAMP(2, true);

  // cos/sin table -> LDS (the loads were issued in round trip 1).  BEFORE the projectile loads are issued:
  // memory returns in order and the number of predicated loads below is not known at compile time, so a
  // wait for the table placed after them is a wait for all of them (`s_waitcnt vmcnt(0)`) -- round trip 2
  // would be over before the workgroup barrier instead of running under the ship / fortress arithmetic.
  // For the same reason EVERY load issued so far is waited for here, explicitly (vmcnt(0), the other counters
  // untouched): a first use of, say, the flags after the predicated loads would otherwise be a vmcnt(0) too.
  __builtin_amdgcn_s_waitcnt(0x0F70);
#pragma unroll
  for (int k = 0; k < kTrigPieces; k++) reinterpret_cast<d2_t*>(lds)[cpi[k]] = cst[k];
  // this lane's (hit, out) event words start at zero; the missile pool's entries OR their slot bit into their
  // OWNER's words (wave-private: only lanes of this wave own entries of this tile; LDS is in order per wave)
  unsigned long long* const evw = reinterpret_cast<unsigned long long*>(lds + kLdsEv) + (tid & ~63u);
  evw[lane] = 0ull;
  if constexpr (!SPLIT) reinterpret_cast<d2_t*>(lds + kLdsAtab)[atab_pi] = atab_piece;  // (every lane the same nine pieces: no branch)

  // ================= round trip 2: live shell slots, predicated by the alive mask ======
  // Slot by slot: a wave ballot skips a slot no lane uses.  The kernel lasts as long as its slowest wave, so
  // the slots reach well past the common case: the dependent-load loop behind them is for slots hardly ever used.
  // (Missiles need no second round trip: the tile's pool rows came with the first.)
  double shx[SF_SPF], shy[SF_SPF], shvx[SF_SPF], shvy[SF_SPF];
#pragma unroll
  for (int s = 0; s < SF_SPF; s++) {
    if (FUSED) {
      shx[s] = shy[s] = shvx[s] = shvy[s] = 0;
    } else {
      // one tick per launch: a slot's registers are read only under the same wave-wide test that loaded them, and what a
      // lane without a shell in the slot computes from them is masked out (`live`): whatever the registers hold will do
      asm volatile("" : "=v"(shx[s]), "=v"(shy[s]), "=v"(shvx[s]), "=v"(shvy[s]));
    }
  }
  // a dead ship whose explosion is over respawns this tick (SRC/game.cpp:151-157): fetch its
  // entry of the spawn sequence now, not in the middle of the arithmetic
  bool will_respawn = !(L.fl & SF_FL_SHIP_ALIVE) && L.death_t >= sfc::explode_duration;
  unsigned long long spawn_e = 0;
  // The spawn entry FIRST and without a branch (a lane that does not respawn gets an out-of-range offset): memory
  // returns in order, so what is issued behind it -- shells, the late set -- is not waited for when the respawn reads it
  const __amdgpu_buffer_rsrc_t rs_spawn =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<int16_t*>(a.spawn), 0, (int)((a.spawn_mask + 1u) * 8u), 0x00020000);
  auto load_spawn = [&]() __attribute__((always_inline)) {
    const i2_t e = __builtin_bit_cast(i2_t, __builtin_amdgcn_raw_buffer_load_b64(rs_spawn, will_respawn ? (L.cursor & a.spawn_mask) * 8u : SF_OOB, 0, 0));
    spawn_e = (unsigned long long)(unsigned)e.x | ((unsigned long long)(unsigned)e.y << 32);
  };
  load_spawn();
  {
    // (the one-trip inner loops here and in updateShells are what is left of slot groups of two.  They stay in this change,
    //  whose check is that the device code is the parent's instruction for instruction: with the loops collapsed the
    //  compiler unrolls in another order and allocates registers differently.  profiles/closed_switches.md)
#pragma unroll
    for (int g = 0; g < SF_SPF; g++) {
      if (__ballot((L.smask & (1u << g)) != 0u) != 0ull) {
#pragma unroll
        for (int k = 0; k < 1; k++) {
          const int s = g + k;
          const bool live = (L.smask >> s) & 1u;
          const d2_t sp = pld16(SF_GOFF(shell_pos, s), live);
          const d2_t sv = pld16(SF_GOFF(shell_vel, s), live);
          shx[s] = sp.x;
          shy[s] = sp.y;
          shvx[s] = sv.x;
          shvy[s] = sv.y;
        }
      }
    }
  }
  // ---- the late set, 2 + 2 SF_MROWS unconditional memory instructions behind everything the first phases wait for: the
  //      score and counts chunks, then the first SF_MROWS rows of the tile's missile pool -- lane l takes entry 64 r + l,
  //      (x, y) and the meta word, if the pool has that many (the count came with the early set): unconditional
  //      instructions, so the compiler can count them when it waits for the spawn entry issued ahead of them
  late = load_lane_late(tb, o);
  if (kPoolLoads) { SF_LOAD_POOL_ROWS(0, L.mpool) }

  __syncthreads();  // the only workgroup barrier of the kernel
  const double* trig = lds;
  SF_STAMP(3, false);
  // A split launch's games' wave reads the fp64 constants of its bearings, sector and extras from the staged constants row
  // as DATA (sf_lane_dev.h: SfKRow): eight broadcast reads here, in front of the key processing and the hand-over's compiler
  // barrier, back long before the first bearing asks for them.  Compiled in they were some forty scalar moves per tick;
  // A/B at 65 536 envs against the build that only stages the row: 6.21 -> 6.11 us per launch in loop launches, 6.28 -> 6.19
  // in graph launches (profiles/step_constants.md; the hexagon edges read the same way measured +0.05 / +0.02 and stay
  // immediates).  The other instantiations keep the immediates: they have no 32 VGPRs to hold the row in.
  SfKRow kc;
  if constexpr (SPLIT) kc = sf_load_krow(lds + SF_CONST_KROW);

  // A fused launch unpacks the late set here, once, in front of its tick loop.  One tick per launch unpacks it behind the
  // two bearings (below): unpacked here, the sign extensions of the key timers -- pure ALU on the loaded words -- are
  // scheduled right behind the respawn, and the wait they bring (the whole late set's round trip but for the score chunk,
  // some eighty instructions after its issue) stands in front of the ship and both atan2s instead of under them.
  if (FUSED) unpack_lane_late(late, L);
  const int n_iter = FUSED ? n_steps : 1;
  // ---- a REPEAT launch (sf_step_repeat, sfmi_repeat.h): the n_steps ticks play ONE action per env and leave ONE row of outputs
  //      -- the summed reward, done, the OR of the ticks' info, events and render hints, the ticks played -- and the
  //      observation and draw record of the state the window ends in.  An env whose game ends inside the window is PARKED:
  //      the tick is straight-line code with wave-wide ballots and a pool the tile shares, so the lane ticks on, but as a game
  //      in which nothing can happen (ship dead and not due back within 255 ticks, no projectiles: no shot, no shell, no
  //      respawn, no event -- the spawn cursor and prev_vlner, which is all new_game reads, stay what the finishing tick left)
  //      and with every output masked; behind the loop it gets its new game, of which no tick has been played.
  //      rp_w: ticks played (bits 0..7), info (8), render hint (9), parked (10)
  constexpr unsigned kRpInfo = 1u << 8, kRpDied = 1u << 9, kRpParked = 1u << 10;
  unsigned rp_w = 0u, rp_events = 0u, rp_proj = 0u;
  int rp_reward = 0;
  double rp_apos = 0, rp_avel = 0;  // the last tick's bearings, for the observation behind the loop
  for (int step = 0; step < n_iter; step++) {
  int act = (XTRA && act_type == SF_ACT_SAMPLED) ? act_sampled : act_next;
  if (FUSED) {
    if (!REPEAT && step + 1 < n_iter) {
      act_next = load_action(step + 1);  // in flight while this tick computes
      if (XTRA && act_type == SF_ACT_SAMPLED) act_sampled = sample_action(step + 1);
    }
    if (step > 0) {
      // the pool rows the previous tick compacted in place: agent-scope loads (they bypass the wave's L1, where the rows
      // read a tick ago may still sit), in flight under the key / ship / fortress / shell arithmetic
      SF_LOAD_POOL_ROWS(16, L.mpool)
      will_respawn = !(L.fl & SF_FL_SHIP_ALIVE) && L.death_t >= sfc::explode_duration;
      load_spawn();
    }
  }
  const size_t so = REPEAT ? (size_t)0 : (size_t)step * (size_t)a.n_envs;  // this tick's row of the output arrays
  const bool rp_parked = REPEAT && (rp_w & kRpParked) != 0u;  // parked by an earlier tick of this window
  // image batches: this tick leaves the envs' draw records for the frame kernel (sf_drawrec.h) -- of a fused launch, the
  // last tick does.  `dr_proj`: where this env's projectiles come near the score / the bar (sfd::hud_flags_near)
  const bool draw_now = OBSK != 1 && a.draw != nullptr && (!FUSED || step + 1 == n_iter);  // uniform
  unsigned dr_proj = 0u;

  const int act_raw = act;  // what rollouts.actions[step] records
  if (act < 0 || act >= a.n_actions) {
    if (!rp_parked) atomicAdd(&a.acc[SF_ACC_BAD_ACTION], 1ull);  // reference: IndexError; here NOOP + counted (sf_check_actions)
    act = 0;
  }
  const unsigned keys = (unsigned)(a.action_keys >> (4 * act)) & 0xFu;

  StatDelta S;

  // ================= Game::stepOneTick (SRC/game.cpp:473-485) =================
  float rew = 0;        // mReward = 0 (updateTime: with the game-over test below, `time` is in a late chunk)

  // ---- processKeyState (SRC/game.cpp:218-272); the wrapper sends FIRE, THRUST, (LEFT, RIGHT)
  //      press-or-release every step (ENV:213-229), so each key is one edge test.  Branch-free:
  //      the flag bits of `fl` sit in key order (FIRE, THRUST, LEFT, RIGHT = bits 2..5), so the
  //      new flags are the key mask itself, an edge is key XOR flag, a press edge is key AND NOT
  //      flag; an edge zeroes that key's timer (:227,231,235,244,250,253,257,261), a press edge
  //      counts (:228,232,236,245).
  int new_m_slot = -1;
  unsigned key_edge_bits = 0;
  float amt_fire = 0.0f, amt_hex = 0.0f;  // this tick's first two score() amounts, applied in order once `points` is needed
  unsigned key_edges;  // SF_EV_PRESS_* | SF_EV_RELEASE_*: the key STATE changes of this tick
  {
    const unsigned kmask = AUTOTURN ? 0x3u : 0xFu;  // autoturn games send two keys (ENV:221)
    const unsigned old = (L.fl >> 2) & kmask, now = keys & kmask;
    const unsigned edge = old ^ now, press = now & ~old;
    key_edges = press | ((old & ~now) << 4);
    L.fl = (L.fl & ~(kmask << 2)) | (now << 2);
    key_edge_bits = edge;  // the key timers live in late chunks: an edge zeroes its timer at stepTimers below
    S.shots += (int)(press & 1u);
    S.thrusts += (int)((press >> 1) & 1u);
    L.kc0 += (press & 1u) | ((press & 2u) << 15);  // shots in the low half, thrusts in the high half
    if (!AUTOTURN) L.kc1 += ((press >> 2) & 1u) | ((press & 8u) << 13);  // lefts, rights
    if (!AUTOTURN) {
      S.lefts += (int)((press >> 2) & 1u);
      S.rights += (int)((press >> 3) & 1u);
    }
    // FIRE press edge: fireMissile (SRC/game.cpp:175-192,237-238) before this tick's turn and
    // move; the shot is counted and the timer zeroed even if nothing could be created
    // as selects: an exec-mask branch around a three-line body costs a lone wave more than the body (the
    // compare travels VALU -> SALU -> EXEC -> VALU).  score(+0.0f) changes nothing: x + 0.0f == x bit for bit for
    // every x these sums can hold (none of them is ever -0.0f), and the clamp does not move a non-negative total.
    {
      const int slot = __ffs(~L.mmask) - 1;
      const bool can = (press & 1u) && (L.fl & SF_FL_SHIP_ALIVE) && slot >= 0 && slot < SF_NSLOT;
      new_m_slot = can ? slot : -1;
      L.mmask |= can ? (1u << (slot & 31)) : 0u;
      amt_fire = can ? -sfc::Score<SHAPED>::missile_penalty : 0.0f;  // reward(-penalty), :187
    }
  }
  // the missile created above starts at the ship's pre-move position and heading
  const double new_m_x = L.sx, new_m_y = L.sy;
  const int new_m_angle = L.angle;
  if constexpr (SPLIT) {  // ... and goes to the tile's missile wave (LDS is in order per wave: the word last)
    reinterpret_cast<d2_t*>(lds + kLdsHand)[tid] = d2_t{new_m_x, new_m_y};
    reinterpret_cast<unsigned*>(lds + kLdsHandMeta)[tid] =
        new_m_slot >= 0 ? SF_MM_PACK(new_m_angle, lane, new_m_slot & 31) : 0x80000000u;
    asm volatile("" ::: "memory");
    const unsigned fired = __ballot(new_m_slot >= 0) != 0ull ? 2u : 1u;
    if (lane == 0u) hflags[0] = fired;
  }

  // ---- monitorShipRespawn (SRC/game.cpp:151-157)
  if (will_respawn) {  // !alive && deathTimer >= shipExplodeDuration, evaluated (and fetched) above
    spawn_ship_from(a, L, spawn_e);  // (mFortress.mTimer = 0, :155: at the fortress update below, a late chunk)
  }

  // ---- updateShip (SRC/game.cpp:314-351)
  if (L.fl & SF_FL_SHIP_ALIVE) {
    if (AUTOTURN) {
      // stdAngle(ceil(angleTo(ship, fortress)))  (SRC/vector.cpp:42-52)
      double t = SPLIT ? sf_atan2_razor(sfc::fort_y - L.sy, sfc::fort_x - L.sx, lds + kLdsAtab, kc)  // (see the bearings below)
                       : sf_atan2<true>(sfc::fort_y - L.sy, sfc::fort_x - L.sx, lds + kLdsAtab);
      if (t < 0) t += M_PI * 2;
      double c = ceil(SPLIT ? rad2deg(t, kc) : rad2deg(t));  // in [0, 360]
      int ia = (int)c;
      if (ia >= 360) ia -= 360;  // fmod(360, 360)
      L.angle = ia;
    } else {
      // TURN_LEFT / TURN_RIGHT / both or none (:317-325): right - left steps of turnSpeed, then stdAngle's wrap
      // (one of the two corrections can apply, and only on the side that was stepped towards)
      L.angle += sfc::turn_speed * ((int)((L.fl / SF_FL_RIGHT) & 1u) - (int)((L.fl / SF_FL_LEFT) & 1u));
      L.angle += L.angle < 0 ? 360 : 0;
      L.angle -= L.angle >= 360 ? 360 : 0;
    }
    {
      const bool th = L.fl & SF_FL_THRUST;
      const double tvx = L.vx + sfc::ship_accel * SF_COS(L.angle), tvy = L.vy + sfc::ship_accel * SF_SIN(L.angle);
      L.vx = th ? tvx : L.vx;
      L.vy = th ? tvy : L.vy;
    }
    L.sx += L.vx;
    L.sy += L.vy;
    // `if (!big.isInside) ... else if (small.isInside) ...` (:337-349), counters branch-free
    const int out_big = !inside_big_hex(L.sx, L.sy);
    const int in_small = !out_big & inside_small_hex(L.sx, L.sy);
    {
      const int dead_now = out_big | in_small;  // killShip (:274-280) on a live ship, as selects
      L.fl &= dead_now ? ~SF_FL_SHIP_ALIVE : ~0u;
      L.death_t = dead_now ? 0 : L.death_t;
      S.ship_deaths += dead_now;
      amt_hex = dead_now ? -sfc::Score<SHAPED>::death_penalty : 0.0f;  // penalize(shipDeathPenalty), :339,345
    }
    S.big_hex_deaths += out_big;
    S.small_hex_deaths += in_small;
  }

  // the two bearings the rest of the tick and the observation need, side by side (ILP)
  // (SPLIT is a constant: one arm of each `SPLIT ? ... : ...` here and below is compiled -- a split launch's takes the
  //  constants from `kc`, the same operations on the same values)
  double a_pos = SPLIT ? sf_atan2_razor(L.sy - sfc::fort_y, L.sx - sfc::fort_x, lds + kLdsAtab, kc)
                       : sf_atan2<true>(L.sy - sfc::fort_y, L.sx - sfc::fort_x, lds + kLdsAtab);
  double a_vel = SPLIT ? sf_atan2_core(L.vy, L.vx, lds + kLdsAtab, kc) : sf_atan2_core(L.vy, L.vx, lds + kLdsAtab);
  if (!FUSED) {
    // the late set's first use, pinned HERE: the timers' words pass through an empty asm together with the two bearings, so
    // nothing that reads them can be scheduled in front of the atan2s, and the set's wait (vmcnt counts only the score chunk
    // behind it) has the key / ship / bearing arithmetic to arrive under.  A/B at 65 536 envs: 6.38 -> 6.25 us per launch
    // in loop launches, 6.43 -> 6.32 in graph launches (profiles/step_first_burst.md)
    asm volatile("" : "+v"(a_pos), "+v"(a_vel), "+v"(late.ta.x), "+v"(late.ta.y), "+v"(late.ta.z), "+v"(late.ta.w));
    unpack_lane_late(late, L);
  }

  // ---- updateFortress (SRC/game.cpp:194-216)
  int new_s_slot = -1;
  unsigned new_s_bit = 0u;  // (a split launch: the new shell's bit of the mask, set behind the shells' walk)
  double new_s_vx = 0, new_s_vy = 0;
  bool fort_respawned = false;
  {
    double ats = SPLIT ? rad2deg(a_pos, kc) : rad2deg(a_pos);  // stdAngle: in [-180, 180], only the sign fix applies
    if (ats < 0) ats += SPLIT ? kc.d360 : 360;
    L.fort_t = will_respawn ? 0 : L.fort_t;  // monitorShipRespawn's mFortress.mTimer = 0 (SRC/game.cpp:155)
    fort_respawned = !(L.fl & SF_FL_FORT_ALIVE) && L.fort_death_t > sfc::fort_respawn;
    L.fort_t = fort_respawned ? 0 : L.fort_t;
    L.fl |= fort_respawned ? SF_FL_FORT_ALIVE : 0u;
    const bool ship_up = L.fl & SF_FL_SHIP_ALIVE;
    {
      double q = SPLIT ? ceil(sf_div_const(ats, kc.d10, kc.inv10)) * kc.d10  // (SF_DIV's form)
                       : ceil(SF_DIV(ats, sfc::sector_size)) * sfc::sector_size;  // in [0, 360]
      int fa = (int)q;
      fa -= fa >= 360 ? 360 : 0;
      L.fort_angle = ship_up ? fa : L.fort_angle;
      const bool moved = ship_up && fa != L.fort_last;
      L.fort_last = moved ? fa : L.fort_last;
      L.fort_t = moved ? 0 : L.fort_t;
    }
    if constexpr (SPLIT) {
      // fireShell (SRC/game.cpp:159-173), the DECISION only, as selects: the slot, the mask bit, the timer, the event.  The
      // shell's velocity -- one sqrt and two fp64 divisions, some fifty instructions behind an exec-mask branch that a wave
      // of 64 games takes on nine ticks in ten for a lane or two -- is not needed by anything this wave does in this tick:
      // the new shell takes no part in the walk below, because it cannot collide (the ship is alive behind updateShip, hence
      // not inside the small hexagon, hence farther than 34 from the fortress; the shell sits 6 from it; they meet at 13)
      // and cannot leave the area (tests/test_shell_fire_model.py holds the hexagon's constants to that).  The tile's missile
      // wave computes and stores it, from (ship - fortress) and the slot filed here, behind the `shot` word (written last;
      // LDS is in order per wave; 1: nobody fired, 2: somebody did).
      const int slot = __ffs(~L.smask) - 1;  // (bits 20..31 of the mask are clear: 0..20)
      const bool lock = ship_up && L.fort_t >= sfc::lock_time && (L.fl & SF_FL_FORT_ALIVE);
      const bool fire = lock && slot < SF_NSLOT;
      new_s_slot = fire ? slot : -1;
      new_s_bit = fire ? 1u << (slot & 31) : 0u;
      L.fort_t = lock ? 0 : L.fort_t;
      reinterpret_cast<d2_t*>(lds + kLdsShot)[tid] = d2_t{L.sx - sfc::fort_x, L.sy - sfc::fort_y};
      reinterpret_cast<unsigned*>(lds + kLdsShotSlot)[tid] = fire ? (unsigned)slot : 0x80000000u;
      asm volatile("" ::: "memory");
      const unsigned shot = __ballot(fire) != 0ull ? 2u : 1u;
      if (lane == 0u) hflags[3] = shot;
    } else if (ship_up) {
      if (L.fort_t >= sfc::lock_time && (L.fl & SF_FL_FORT_ALIVE)) {
        // fireShell (SRC/game.cpp:159-173): vel = shellSpeed * (cos, sin)(deg2rad(angle_to_ship)).
        // angle_to_ship is the bearing of d = ship - fortress, so (cos, sin) = d / |d|: one sqrt
        // and two divisions instead of a device sincos with argument reduction.  Shell velocity
        // was never bit-exact against glibc's sin/cos anyway; both forms sit within a few 1e-15
        // of the true direction (shell positions are tested to 1e-9).
        int slot = __ffs(~L.smask) - 1;
        if (slot < SF_NSLOT) {
          new_s_slot = slot;
          L.smask |= 1u << slot;
          const double ddx = L.sx - sfc::fort_x, ddy = L.sy - sfc::fort_y;
          const double nrm = sqrt(ddx * ddx + ddy * ddy);
          new_s_vx = sfc::shell_speed * (ddx / nrm);
          new_s_vy = sfc::shell_speed * (ddy / nrm);
        }
        L.fort_t = 0;
      }
    }
  }
  SF_STAMP(4, false);
  SF_STAMP(5, true);

  // keep the spawn entry's register allocated up to here: reused earlier, the compiler must first wait for the
  // (predicated, possibly outstanding) load into it -- a vmcnt(0), i.e. the whole of round trip 2, right
  // after the key processing
  asm volatile("" ::"v"(spawn_e));
  // the (cos, sin) of the pool rows' headings in ONE batch of LDS reads, here, so that their latency hides under the
  // shells (a wave alone on its SIMD hides nothing: looked up row by row below, each would pay its own LDS round trip)
  const unsigned m_live = (unsigned)__builtin_amdgcn_readfirstlane((int)L.mpool);  // entries in the pool before this tick
  d2_t pcs[SF_MROWS];
#pragma unroll
  for (int r = 0; r < SF_MROWS; r++)
    pcs[r] = SPLIT ? d2_t{0, 0} : *reinterpret_cast<const d2_t*>(&trig[2 * SF_MM_ANGLE(pmeta[r])]);

  // the tick's first two score() calls (fireMissile's penalty, then a hexagon death), in their order, now that the
  // score chunk is needed anyway (shell kills and missile events follow)
  score(amt_fire, rew, L);
  score(amt_hex, rew, L);

  // The constants of the projectile arithmetic, parked in VGPRs: none of them is an inline constant, SGPRs are
  // scarce (101 of 102 in use), and the compiler re-materialises each as an `s_mov_b32` pair in front of every slot
  // group -- about a hundred scalar moves per tick that a lone wave pays in full.  Opaque to the optimiser on
  // purpose; the values are the same doubles.
  double kv_speed = sfc::missile_speed, kv_fx = sfc::fort_x, kv_fy = sfc::fort_y, kv_w = sfc::width_d, kv_h = sfc::height_d,
         kv_mr2 = sfc::missile_hit_r2, kv_sr2 = sfc::shell_hit_r2;
  asm volatile("" : "+v"(kv_speed), "+v"(kv_fx), "+v"(kv_fy), "+v"(kv_w), "+v"(kv_h), "+v"(kv_mr2), "+v"(kv_sr2));
  // Game::isOutsideGameArea (SRC/game.cpp:129-131), (x < 0) | (x > W) | (y > H) | (y < 0), as ONE comparison:
  // the largest of -x, x - W, -y, y - H is positive exactly when one of the four holds (a difference of two
  // doubles has the exact sign; no NaN on this path).  Four compares OR-ed through scalar registers are a chain of
  // VALU -> SALU -> VALU hand-offs per slot, which a wave alone on its SIMD waits out every time.
  auto outside = [&](double x, double y) __attribute__((always_inline)) -> bool {
    return __builtin_fmax(__builtin_fmax(-x, x - kv_w), __builtin_fmax(-y, y - kv_h)) > 0;
  };

  // ---- updateShells (SRC/game.cpp:404-423).  Ballistics of the prefetched slots first, as
  //      straight-line code; then the (ship-alive dependent) outcome in slot order.
  // What is written ONCE per projectile -- a new shell's velocity -- is one store for the
  // wave with the slot in the lane's offset, not a predicated store per slot: every memory instruction of the four
  // waves of a CU goes through the one address unit they share, idle lanes or not.
  static_assert(sfl::kGroups[SF_G_shell_vel].chunk * sfl::kTileLanes == 1024, "slot stride of the row below");
  if (!SPLIT && __ballot(new_s_slot >= 0) != 0ull)  // (a split launch: the missile wave's store)
    pst16_at(SF_GOFF(shell_vel, 0), new_s_slot >= 0, (unsigned)new_s_slot * 1024u, d2_t{new_s_vx, new_s_vy});
  {
#pragma unroll
    for (int g = 0; g < SF_SPF; g++) {
      const unsigned gmask = 1u << g;
      if (__ballot((L.smask & gmask) != 0u) == 0ull) continue;
      unsigned col = 0, out = 0;
      double nx[1], ny[1];
#pragma unroll
      for (int k = 0; k < 1; k++) {
        const int s = g + k;
        const bool isnew = !SPLIT && (s == new_s_slot);
        const double vx = isnew ? new_s_vx : shvx[s], vy = isnew ? new_s_vy : shvy[s];
        nx[k] = (isnew ? kv_fx : shx[s]) + vx;
        ny[k] = (isnew ? kv_fy : shy[s]) + vy;
        // Object::collided (SRC/object.cpp:12-15): sqrt(dx^2+dy^2) <= r.  With a correctly
        // rounded sqrt and r an integer, RN(sqrt(s)) <= r  <=>  s <= r^2 (r^2 is exactly
        // representable and the next double above r^2 has a root that rounds above r).
        const double dx = nx[k] - L.sx, dy = ny[k] - L.sy;
        col |= (unsigned)(dx * dx + dy * dy <= kv_sr2) << s;
        out |= (unsigned)outside(nx[k], ny[k]) << s;
        if (FUSED) {  // the registers carry the shell into the next tick
          shx[s] = nx[k];
          shy[s] = ny[k];
          shvx[s] = vx;
          shvy[s] = vy;
        }
      }
      const unsigned live = L.smask & gmask;
      col &= live;
      // slot order: the first colliding shell kills a live ship; every other shell only
      // leaves by flying out (`if (alive && collided) ... else if (outside)`, :410-420)
      unsigned dead = out & live;
      {
        const int hitship = (L.fl & SF_FL_SHIP_ALIVE) && col;
        dead |= hitship ? (col & (0u - col)) : 0u;  // lowest colliding slot
        L.fl &= hitship ? ~SF_FL_SHIP_ALIVE : ~0u;  // killShip on a live ship, as selects
        L.death_t = hitship ? 0 : L.death_t;
        S.ship_deaths += hitship;
        S.shell_deaths += hitship;
        score(hitship ? -sfc::Score<SHAPED>::death_penalty : 0.0f, rew, L);
      }
      L.smask &= ~dead;
#pragma unroll
      for (int k = 0; k < 1; k++) {
        const int s = g + k;
        pst16(SF_GOFF(shell_pos, s), (L.smask >> s) & 1u, d2_t{nx[k], ny[k]});
        if (draw_now)
          if (((L.smask >> s) & 1u) && sfd::hud_rows_near((float)ny[k], sfd::kShellExt))  // (all but never)
            dr_proj |= sfd::hud_flags_near((float)nx[k], (float)ny[k], sfd::kShellExt);
      }
    }
    if (__ballot((L.smask >> SF_SPF) != 0u) != 0ull) {  // rare: more than SF_SPF shells in some lane
#pragma unroll 1
      for (int s = SF_SPF; s < SF_NSLOT; s++) {
        const bool live = (L.smask >> s) & 1u;
        if (__ballot(live) == 0ull) continue;
        if (live) {
          double x, y, vx, vy;
          if (!SPLIT && s == new_s_slot) {
            x = sfc::fort_x;
            y = sfc::fort_y;
            vx = new_s_vx;
            vy = new_s_vy;
          } else {
            const d2_t sp = ld_coherent_d2(SF_CHUNK(shell_pos, s) + o.o16);
            const d2_t sv = ld_coherent_d2(SF_CHUNK(shell_vel, s) + o.o16);
            x = sp.x;
            y = sp.y;
            vx = sv.x;
            vy = sv.y;
          }
          x += vx;
          y += vy;
          bool dead = false;
          if (L.fl & SF_FL_SHIP_ALIVE) {
            const double dx = x - L.sx, dy = y - L.sy;
            if (dx * dx + dy * dy <= sfc::shell_hit_r2) {
              dead = true;
              kill_ship(L, S);
              score(-sfc::Score<SHAPED>::death_penalty, rew, L);
              S.shell_deaths += 1;
            }
          }
          if (!dead && outside_area(a, x, y)) dead = true;
          if (dead) {
            L.smask &= ~(1u << s);
          } else {
            SF_ST(d2_t, SF_CHUNK(shell_pos, s), o.o16, (d2_t{x, y}));
            if (draw_now) dr_proj |= sfd::hud_flags_near((float)x, (float)y, sfd::kShellExt);
          }
        }
      }
    }
    if constexpr (SPLIT) L.smask |= new_s_bit;  // the shell fired this tick: in the count and the lane's stores, not in the walk
  }

  // ---- updateMissiles (SRC/game.cpp:353-402) over the tile's missile POOL.  The reference walks 20 slots per env; with
  //      one lane per env a wave would walk every slot ANY of its 64 envs uses with a couple of lanes busy.  The tile's
  //      live missiles are kept as one dense list instead: a row is 64 entries, one per lane, whoever owns them, every
  //      lane busy (random play: 104 missiles per tile = 2 rows instead of 8-9 slot passes).  An entry that hits the
  //      fortress or leaves the area ORs its slot bit into its OWNER lane's event words in LDS; the survivors are
  //      compacted IN PLACE (ballot + prefix count) as the rows go by -- a row is in registers before anything is
  //      written, and entries only move down.  What the hits and misses do to the fortress / score depends only on how
  //      many of each an env has (sf_events.h), so the owners count the collected masks afterwards: no replay in slot order.
  //      New missiles (fired this tick, SRC/game.cpp:237-238: before the move) are one more row, lane = owner.
  unsigned hit_count = 0;  // missiles that reached the fortress this tick (alive or not)
  {
    unsigned wp = 0;  // write pointer of the compaction = entries kept so far (wave-uniform)
    unsigned* const evw32 = reinterpret_cast<unsigned*>(evw);
    // (the draw records of this wave's 64 envs: one descriptor, like the tile's)
    const __amdgpu_buffer_rsrc_t rs_draw = __builtin_amdgcn_make_buffer_rsrc(
        draw_now ? a.draw + (size_t)__builtin_amdgcn_readfirstlane(i >> 6) * (size_t)SF_DR_TILE_BYTES : (unsigned char*)nullptr, 0,
        draw_now ? SF_DR_TILE_BYTES : 0, 0x00020000);
    auto m_row = [&](double x, double y, unsigned meta, d2_t cs, bool valid) __attribute__((always_inline)) {
      // velocity = missileSpeed * (cos, sin)(deg2rad(angle)) with an integer angle: table
      const double nx = x + kv_speed * cs.x, ny = y + kv_speed * cs.y;
      const double dx = nx - kv_fx, dy = ny - kv_fy;
      const bool hit = valid & (dx * dx + dy * dy <= kv_mr2);  // collided(mFortress), see shells
      const bool gone = valid & (hit | outside(nx, ny));       // `else if (isOutsideGameArea)`: hit wins
      if (__ballot(gone) != 0ull) {
        if (gone) {  // (slot bit) -> the owner's hit word or, for a missile that left the area, its out word
          __hip_atomic_fetch_or(evw32 + 2 * SF_MM_OWNER(meta) + (hit ? 0 : 1), 1u << SF_MM_SLOT(meta), __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      }
      const bool keep = valid & !gone;
      const unsigned long long kb = __ballot(keep);
      const unsigned idx = wp + __builtin_amdgcn_mbcnt_hi((unsigned)(kb >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)kb, 0u));
      wp += (unsigned)__popcll(kb);
      sf_buf_st128<kStAux>(__builtin_bit_cast(u4_t, (d2_t{nx, ny})), rs, keep ? idx * 16u : SF_OOB,
                                             SF_GOFF(missile_pos, 0));
      __builtin_amdgcn_raw_buffer_store_b32(meta, rs, keep ? idx * 4u : SF_OOB, SF_GOFF(missile_meta, 0), kStAux);
      if (draw_now) {  // uniform.  The survivor's transform goes to its OWNER's draw record, at its slot (sf_drawrec.h)
        typedef float f4_t __attribute__((ext_vector_type(4)));
        const unsigned doff = (SF_DR_PIECE_OBJ0 + SF_DR_OBJ_MISSILE0 + SF_MM_SLOT(meta)) * (unsigned)SF_DR_PIECE_STRIDE +
                              SF_MM_OWNER(meta) * (unsigned)SF_DR_LANE_STRIDE;
        sf_buf_st128<0>(__builtin_bit_cast(u4_t, (d2_t{nx, ny})), rs_draw, keep ? doff : SF_OOB, 0);
        __builtin_amdgcn_raw_buffer_store_b16((short)SF_MM_ANGLE(meta), rs_draw,
                                              keep ? SF_DR_ANGLES_OFF + 2u * SF_MM_SLOT(meta) + SF_MM_OWNER(meta) * (unsigned)SF_DR_LANE_STRIDE : SF_OOB,
                                              0, 0);
        const bool rows = keep & sfd::hud_rows_near((float)ny, sfd::kMissileExt);
        if (__ballot(rows) != 0ull) {  // (all but never) -> bits 24..27 of the owner's hit word
          if (rows)
            __hip_atomic_fetch_or(evw32 + 2 * SF_MM_OWNER(meta), sfd::hud_flags_near((float)nx, (float)ny, sfd::kMissileExt) << 24,
                                  __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
      }
    };
    if constexpr (SPLIT) {  // the tile's missile wave did all of that: wait for its word
      // A launch of one tick (kEarlySt) stores a chunk of the lane when its last writer has run, not with the others at the end, where
      // the 4 + 4 waves of a CU queue for its one address unit (19 cycles per memory instruction, NOTES.md).  The ship moves
      // for the last time in updateShip: its two chunks go out here, in the middle of the launch, while that unit has nothing
      // to do -- and behind the shells' walk, the last consumer of a load: a wait of the compiler's for a load (it does not
      // see these stores) would be a wait for their acknowledgement too.  A new game rewrites them: see the lane's stores
      // below.  A/B at 65 536 envs: 5.77 -> 5.63 us per launch in loop launches, 5.78 -> 5.71 in graph launches
      // (profiles/step_wave_ends.md)
      if (kEarlySt) store_lane_ship(rs, o, L);
      unsigned dw, spins = 0u;
      SF_STAMP(16, false);
      while (!((dw = (unsigned)__builtin_amdgcn_readfirstlane((int)hflags[1])) >> 31) && ++spins < kSpinLimit) __builtin_amdgcn_s_sleep(1);
      if (spins >= kSpinLimit && lane == 0u) atomicAdd(&a.acc[SF_ACC_HANDOVER], 1ull);
      asm volatile("" ::: "memory");
      SF_STAMP(17, false);
      wp = dw & 0x7FFFFFFFu;
    } else {
#pragma unroll
      for (int r = 0; r < SF_MROWS; r++)
        if (m_live > 64u * r) m_row(prow[r].x, prow[r].y, pmeta[r], pcs[r], 64u * r + lane < m_live);
      if (m_live > 64u * SF_MROWS) {  // rare: more than SF_MROWS rows of live missiles in this tile
#pragma unroll 1
        for (unsigned r = SF_MROWS; 64u * r < m_live; r++) {
          // agent-scope loads: in a fused launch the previous tick of this wave wrote these rows
          const d2_t pr = __builtin_bit_cast(d2_t, __builtin_amdgcn_raw_buffer_load_b128(rs, o.o16 + r * 1024u, SF_GOFF(missile_pos, 0), 16));
          const unsigned pm = __builtin_amdgcn_raw_buffer_load_b32(rs, o.o4 + r * 256u, SF_GOFF(missile_meta, 0), 16);
          m_row(pr.x, pr.y, pm, *reinterpret_cast<const d2_t*>(&trig[2 * SF_MM_ANGLE(pm)]), 64u * r + lane < m_live);
        }
      }
      if (__ballot(new_m_slot >= 0) != 0ull)
        m_row(new_m_x, new_m_y, SF_MM_PACK(new_m_angle, lane, new_m_slot & 31),
              *reinterpret_cast<const d2_t*>(&trig[2 * new_m_angle]), new_m_slot >= 0);
    }
    L.mpool = wp;
    if (kEarlySt && !SPLIT) store_lane_ship(rs, o, L);  // (as the split launch's above: behind the pool rows, the last loads)
    // the owners collect what happened to their missiles (LDS is in order per wave; the fences pin the compiler)
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const unsigned long long evp = evw[lane];
    if (FUSED) evw[lane] = 0ull;  // ready for the next tick
    unsigned ev_hit = (unsigned)evp, ev_out = (unsigned)(evp >> 32);
    dr_proj |= (ev_hit >> 24) & 0xFu;  // (draw records: this env's missiles near the score / the bar, sfd::hud_flags_near)
    ev_hit &= L.mmask;             // hit = live & collided
    ev_out &= L.mmask & ~ev_hit;   // out = live & !hit & outside
    const unsigned ev = ev_hit | ev_out;
    hit_count = __popc(ev_hit);
    L.mmask &= ~ev;
    // slot order (SRC/game.cpp:355) does not matter beyond the two counts: the fortress state machine of :357-399 in
    // closed form (sf_events.h: no loop, no wave-wide test), and the one amount it can score.  A miss only counts:
    static_assert(sfc::Score<false>::miss_penalty == 0.0f && sfc::Score<true>::miss_penalty == 0.0f,
                  "sf_missile_events scores no miss (:394-398)");
    {
      const SfMissileEvents e = sf_missile_events((int)hit_count, __popc(ev_out), (L.fl & SF_FL_FORT_ALIVE) != 0u, L.fort_vuln_t,
                                                  L.vlner, sfc::vuln_time, sfc::vuln_threshold, sfc::Score<SHAPED>::destroy_reward);
      L.vlner = e.vlner;
      L.fl &= e.fort_alive ? ~0u : ~SF_FL_FORT_ALIVE;
      L.fort_vuln_t = e.fort_vuln_t;
      L.fort_death_t = e.fort_death_reset ? 0 : L.fort_death_t;
      S.vlner_incs += e.incs;
      S.max_vlner = e.max_vlner > S.max_vlner ? e.max_vlner : S.max_vlner;
      S.destroyed += e.destroyed;
      S.resets += e.resets;
      S.missed += e.missed;
      score(e.amount, rew, L);
    }
  }
  // The score chunk is final here in a launch of one tick (kEarlySt): the tick's last score() is the one above, the vulnerability and
  // the three counters that ride in the chunk have their last writers behind them (updateShip, the shells, the events),
  // and `time` only counts the tick.  It goes out in front of the timers and the reward arithmetic, not behind them.  (The
  // four updates are the ones updateTime and the statistics make below, on a copy: the tick's text stays what it is for the
  // launches of several ticks, and the compiler computes each once.)
  if (kEarlySt) {
    Lane Ls = L;
    Ls.time += sfc::tick_ms;
    Ls.c_maxv = (unsigned)S.max_vlner > L.c_maxv ? (unsigned)S.max_vlner : L.c_maxv;
    Ls.c_small += (unsigned)S.small_hex_deaths;
    Ls.c_shell += (unsigned)S.shell_deaths;
    store_lane_score(rs, o, Ls);
  }
  SF_STAMP(6, false);

  // ---- stepTimers (SRC/game.cpp:425-451)
  L.fort_t += sfc::tick_ms;
  L.fort_death_t += sfc::tick_ms;
  L.fort_vuln_t += sfc::tick_ms;
  L.death_t += sfc::tick_ms;
  // (a key edge of processKeyState zeroes its timer, :227,231,235,244,250,253,257,261: applied here, nothing in between reads them)
  L.fire_t = ((key_edge_bits & 1u) ? 0 : L.fire_t) + ((L.fl & SF_FL_FIRE) ? 1 : -1);
  L.thrust_t = ((key_edge_bits & 2u) ? 0 : L.thrust_t) + ((L.fl & SF_FL_THRUST) ? 1 : -1);
  L.left_t = ((key_edge_bits & 4u) ? 0 : L.left_t) + ((L.fl & SF_FL_LEFT) ? 1 : -1);
  L.right_t = ((key_edge_bits & 8u) ? 0 : L.right_t) + ((L.fl & SF_FL_RIGHT) ? 1 : -1);

  int r = (int)rew;  // `return mReward` through `int stepOneTick` (SRC/game.hh:138): truncation
  // kept for `Game.step_one_tick`'s return value (field last_reward): the spare byte next to the flags
  L.fl = (L.fl & 0xFFu) | ((unsigned)(r & 0xFF) << 8);

  // ================= SSF_Env.step epilogue (ENV:233-253) =================
  const int fort_kill = r > 0;
  if (SHAPED) {
    const int vlner_change = L.vlner - L.prev_vlner;
    if (L.vlner <= 10 && !fort_kill) r += vlner_change;
    r = r > 1 ? 1 : (r < -1 ? -1 : r);
    r = r + 2 * fort_kill;
    L.prev_vlner = L.vlner;
  }
  L.time += sfc::tick_ms;                     // updateTime (SRC/game.cpp:475); nothing in between reads it
  const int done = L.time >= sfc::game_time;  // Game::isGameOver (SRC/game.cpp:487-489)

  // ---- optional telemetry: what happened this tick, as a bitmask (the reference's addEvent strings,
  //      SRC/game.cpp:124-127 and its call sites; include/sfmi.h SF_EV_*).  Everything it needs is already live.
  unsigned evmask = 0;
  if (a.events) {
    const int live_hits = S.vlner_incs + S.destroyed + S.resets;
    evmask = key_edges | (new_m_slot >= 0 ? SF_EV_MISSILE_FIRED : 0u) | (will_respawn ? SF_EV_SHIP_RESPAWN : 0u) |
             (S.big_hex_deaths ? SF_EV_EXPLODE_BIGHEX : 0u) | (S.small_hex_deaths ? SF_EV_EXPLODE_SMALLHEX : 0u) |
             (fort_respawned ? SF_EV_FORTRESS_RESPAWN : 0u) | (new_s_slot >= 0 ? SF_EV_FORTRESS_FIRED : 0u) |
             (S.shell_deaths ? SF_EV_SHELL_HIT_SHIP : 0u) | (live_hits ? SF_EV_HIT_FORTRESS : 0u) |
             (S.vlner_incs ? SF_EV_VLNER_INCREASED : 0u) | (S.destroyed ? SF_EV_FORTRESS_DESTROYED : 0u) |
             (S.resets ? SF_EV_VLNER_RESET : 0u) | ((int)hit_count > live_hits ? SF_EV_HIT_DEAD_FORTRESS : 0u) |
             (S.missed ? SF_EV_MISSILE_LEFT : 0u) | (done ? SF_EV_GAME_OVER : 0u);
  }

  SF_STAMP(10, false);
  // ================= statistics and the vec-env worker's auto-reset (rl/train.py:80-88) ======
  // The tick's share of the per-episode counters (they ride above the timers, vlner, time and the cursor: sf_layout.h)
  L.ep_return += r;
  L.ep_kills += (unsigned)fort_kill;
  L.c_resets += (unsigned)S.resets;
  L.c_missed += (unsigned)S.missed;
  L.c_incs += (unsigned)S.vlner_incs;
  L.c_maxv = (unsigned)S.max_vlner > L.c_maxv ? (unsigned)S.max_vlner : L.c_maxv;  // counter 12: a running maximum
  L.c_big += (unsigned)S.big_hex_deaths;
  L.c_small += (unsigned)S.small_hex_deaths;
  L.c_shell += (unsigned)S.shell_deaths;
  L.c_destroyed += (unsigned)S.destroyed;
  if (XTRA && !REPEAT && !a.auto_reset) {  // uniform (a REPEAT launch: auto-resetting batches only)
    // The packed per-episode counters (sf_layout.h: SF_W_*) are sized for ONE episode.  A batch without auto-reset
    // keeps ticking past game over like the bare SSF_Env / Game (ENV:246) until the caller resets, and the reference's
    // plain ints keep counting: a field that no longer fits its bits is counted here (sticky: sf_check_state) instead
    // of wrapping silently.  Auto-resetting batches zero every field at 5 295 ticks, long before any of them fills up.
    const unsigned ov = ((L.c_resets | L.c_missed) >> 16) | ((L.c_incs | L.c_maxv | (unsigned)L.vlner) >> 12) |
                        ((L.c_big | L.c_small | L.c_shell | L.c_destroyed | L.ep_kills) >> 8) | ((unsigned)L.time >> 24) |
                        (((unsigned)(L.fire_t + 32768) | (unsigned)(L.thrust_t + 32768) | (unsigned)(L.left_t + 32768) |
                          (unsigned)(L.right_t + 32768)) >> 16) |
                        (unsigned)(S.shots && (L.kc0 & 0xFFFFu) == 0u) | (unsigned)(S.thrusts && (L.kc0 >> 16) == 0u) |
                        (unsigned)(S.lefts && (L.kc1 & 0xFFFFu) == 0u) | (unsigned)(S.rights && (L.kc1 >> 16) == 0u);
    if (__ballot(ov != 0u) != 0ull)
      if (ov != 0u && real) atomicAdd(&a.acc[SF_ACC_OVERFLOW], 1ull);
  }
  if constexpr (REPEAT) {  // this tick's share of the window's row, unless the env was parked before it
    rp_reward += rp_parked ? 0 : r;
    rp_events |= rp_parked ? 0u : evmask;
    rp_w += rp_parked ? 0u : 1u;
    rp_w |= rp_parked ? 0u : ((fort_kill ? kRpInfo : 0u) | ((S.big_hex_deaths | S.small_hex_deaths | S.shell_deaths) ? kRpDied : 0u));
  }
  if (REPEAT ? (done && !rp_parked) : (done && a.auto_reset)) {
    // episode totals (rl/train.py:81-88,161-164), this tick's share included
    const int ep_ret = L.ep_return, ep_kil = (int)L.ep_kills;
    const int deaths = (int)(L.c_big + L.c_small + L.c_shell);  // killShip's three call sites
    const int shots = (int)(L.kc0 & 0xFFFFu);  // this tick's press included
    if (real) {
      atomicAdd(&a.acc[0], 1ull);
      atomicAdd(&a.acc[1], (unsigned long long)(long long)ep_ret);
      atomicAdd(&a.acc[2], (unsigned long long)((long long)ep_ret * ep_ret));
      atomicAdd(&a.acc[3], (unsigned long long)(long long)ep_kil);
      atomicAdd(&a.acc[4], (unsigned long long)deaths);
      atomicAdd(&a.acc[5], (unsigned long long)shots);
      atomicMin((long long*)&a.acc[6], (long long)ep_ret);
      atomicMax((long long*)&a.acc[7], (long long)ep_ret);
    }
    // the finished game's last observation (a.final_obs: sf_set_final_obs_output): the row SSF_Env.step returned for this
    // tick (ENV:246-253), from the state as it stands and the tick's own bearings, before the new game replaces both.  Once
    // per 5 295 ticks and lane: plain stores straight to the row, no staging
    if ((FOBS || REPEAT) && a.final_obs != nullptr) {  // uniform
      if (real) write_obs_row(a, a.final_obs, i, L, compute_extras(a, L, a_pos, a_vel));
    }
    if constexpr (REPEAT) {
      // parked (see rp_w above): the rest of the window is ticks of a game in which nothing happens.  Its missiles fly on in
      // the tile's pool, unowned (their events meet an empty mask), and leave with the new game behind the loop
      rp_w |= kRpParked;
      L.fl &= ~SF_FL_SHIP_ALIVE;
      L.death_t = -(1 << 24);  // (255 ticks add 8 670)
      L.mmask = L.smask = 0u;
    } else {
    // a new Game (ENV:163-178).  Its missiles are gone with it: the pool entries this lane still owns leave below
    new_game(a, L);
    a_pos = sf_atan2<true>(L.sy - sfc::fort_y, L.sx - sfc::fort_x);
    a_vel = sf_atan2<false>(L.vy, L.vx);
    }
  }
  if constexpr (!REPEAT) SF_PURGE_POOL(__ballot(done && a.auto_reset))

  SF_STAMP(11, false);
  if constexpr (!REPEAT)
    if (draw_now) SF_DRAW_HEADER(done && a.auto_reset, dr_proj)  // uniform
  if (!FUSED && !kEarlySt) store_lane_buf(rs, o, L);
  if (kEarlySt) {
    // the ship's chunks and the score chunk went out above; a new game rewrites them: once per 5 295 ticks the tile stores
    // them again, behind new_game and -- same wave, same addresses, same kind of store -- in program order behind the first.
    // The other four chunks hold a timer, the reward byte or a counter the reward feeds: nothing of them is final earlier.
    if (__ballot(done && a.auto_reset) != 0ull) {
      store_lane_ship(rs, o, L);
      store_lane_score(rs, o, L);
    }
    store_lane_rest(rs, o, L);
  }
  SF_STAMP(14, false);

  if constexpr (REPEAT) {
    rp_apos = a_pos;
    rp_avel = a_vel;
    rp_proj = dr_proj;
    if (__ballot(!(rp_w & kRpParked)) == 0ull) break;  // uniform: every env of the tile is parked (batches run in lockstep)
  } else {
  if (real) {
    if (reward_out) SF_ST(int32_t, (unsigned char*)(reward_out + so), g.o4, r);
    if (done_out) SF_ST(uint8_t, (unsigned char*)(done_out + so), g.o1, (uint8_t)done);
    if (info_out) SF_ST(uint8_t, (unsigned char*)(info_out + so), g.o1, (uint8_t)fort_kill);
    if (a.events) SF_ST(uint32_t, (unsigned char*)(a.events + so), g.o4, evmask);
    if (XTRA && a.act_out) SF_ST(uint8_t, (unsigned char*)(a.act_out + so), g.o1, (uint8_t)act_raw);  // what the lane played (sampled or given)
    SF_STAMP(15, false);
    if (a.t_reward) {  // uniform; the same float32 operations in the same order as rl/train.py:82-88
      const float rf = (float)r, mask = done ? 0.0f : 1.0f;
      SF_ST(float, (unsigned char*)(a.t_reward + so), g.o4, rf);
      if (a.t_mask) SF_ST(float, (unsigned char*)(a.t_mask + so), g.o4, mask);
      if (a.t_episode) {
        const float ep = SF_LD(float, (const unsigned char*)a.t_episode, g.o4) + rf;  // episode_rewards += reward
        if (a.t_final) {
          float fin = SF_LD(float, (const unsigned char*)a.t_final, g.o4) * mask;     // final_rewards *= masks
          fin = fin + (1.0f - mask) * ep;                                              // += (1 - masks) * episode_rewards
          SF_ST(float, (unsigned char*)a.t_final, g.o4, fin);
        }
        SF_ST(float, (unsigned char*)a.t_episode, g.o4, ep * mask);                    // episode_rewards *= masks
      }
      if (a.t_actions) SF_ST(long long, (unsigned char*)(a.t_actions + so), g.o8, (long long)act_raw);
    }
  }
  SF_STAMP(7, false);
  SF_WRITE_OBSERVATION(so, a_pos, a_vel, done && a.auto_reset)
  if constexpr (OBSK != 1) {
    // image batches: which ships died this tick, one word per tile.  sf_render_kernel starts those frames first (the
    // first frame of an explosion costs three ordinary ones, sf_render.hip); a scheduling hint, nothing else reads it
    if (a.hint) {  // uniform
      const unsigned long long died = __ballot(real && (S.big_hex_deaths | S.small_hex_deaths | S.shell_deaths) != 0);
      if (lane == 0) a.hint[i >> 6] = died;
    }
  }
  if (!FUSED && a.n_partials) {  // uniform: VecNormalize's reduction rides on the step (sf_step_normalize)
    double my_ret = 0;
    if (a.n_ret && real) {
      my_ret = SF_LD(double, (const unsigned char*)a.n_ret, g.o8) * a.n_gamma + (double)r;  // ret = ret * gamma + rews
      SF_ST(double, (unsigned char*)a.n_ret, g.o8, my_ret);
    }
    const bool has_obs = obs != nullptr && a.obs_type != 3;
    if (a.obs_f64)
      norm_partials_wave<double>(a, lds + kLdsStage + (size_t)(tid & ~63u) * a.obs_dim, i & ~63u, lane, my_ret, has_obs);
    else
      norm_partials_wave<float>(a, reinterpret_cast<float*>(lds + kLdsStage) + (size_t)(tid & ~63u) * a.obs_dim, i & ~63u,
                                lane, my_ret, has_obs);
  }
  }  // (!REPEAT)
  }  // tick loop
  if constexpr (REPEAT) {
    // the parked envs' new games (ENV:163-178; rl/train.py:80), of which no tick is played in this launch; their missiles --
    // the finished games' -- leave the tile's pool
    const bool parked = (rp_w & kRpParked) != 0u;
    const unsigned long long pk = __ballot(parked);
    if (pk != 0ull) {
      if (parked) {
        new_game(a, L);
        rp_apos = sf_atan2<true>(L.sy - sfc::fort_y, L.sx - sfc::fort_x);
        rp_avel = sf_atan2<false>(L.vy, L.vx);
      }
      SF_PURGE_POOL(pk)
    }
  }
  if (FUSED) store_lane_buf(rs, o, L);
  if constexpr (REPEAT) {  // the window's one row (a.act_out: the ticks played, sf_launch_step_repeat)
    const bool parked = (rp_w & kRpParked) != 0u;
    if (OBSK != 1 && a.draw != nullptr) SF_DRAW_HEADER(parked, rp_proj)  // uniform
    if (real) {
      if (reward_out) SF_ST(int32_t, (unsigned char*)reward_out, g.o4, rp_reward);
      if (done_out) SF_ST(uint8_t, (unsigned char*)done_out, g.o1, (uint8_t)parked);
      if (info_out) SF_ST(uint8_t, (unsigned char*)info_out, g.o1, (uint8_t)((rp_w & kRpInfo) != 0u));
      if (a.events) SF_ST(uint32_t, (unsigned char*)a.events, g.o4, rp_events);
      if (a.act_out) SF_ST(uint8_t, (unsigned char*)a.act_out, g.o1, (uint8_t)(rp_w & 0xFFu));
    }
    SF_WRITE_OBSERVATION((size_t)0, rp_apos, rp_avel, parked)
    if constexpr (OBSK != 1) {
      if (a.hint) {  // uniform: the ships that died in ANY tick of the window (it only decides when a frame is drawn)
        const unsigned long long died = __ballot(real && (rp_w & kRpDied) != 0u);
        if (lane == 0) a.hint[i >> 6] = died;
      }
    }
  }
  if (XTRA && !REPEAT && act_type == SF_ACT_SAMPLED && lane == 0)  // the tile's tick counter moves on by the ticks of this launch
    reinterpret_cast<unsigned*>(const_cast<void*>(actions))[4 * (size_t)(i >> 6)] = act_rec.x + (unsigned)n_iter;
  SF_STAMP(8, false);
  SF_STAMP(9, true);
#ifdef SF_STAMPS
  stamp_[13] = __builtin_amdgcn_s_memrealtime();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if (a.dbg != nullptr && (tid & 63) == 0) {
    unsigned long long* d = a.dbg + (size_t)(i >> 6) * SF_STAMP_SLOTS;
#pragma unroll
    for (int k = 0; k < SF_STAMP_SLOTS; k++) d[k] = stamp_[k];
  }
#endif
}

// ---------------------------------------------------------------------------------------------
// launchers (called by sf_capi.cpp)

hipError_t sf_launch_reset(const SfKernelArgs& a, int first, unsigned cursor0, unsigned stride, void* obs,
                           hipStream_t stream) {
  const unsigned grid = (unsigned)(a.lanes / SF_BLOCK);
  hipLaunchKernelGGL(sf_reset_kernel, dim3(grid), dim3(SF_BLOCK), 0, stream, a, first, cursor0, stride, obs);
  return hipGetLastError();
}

hipError_t sf_launch_step(const SfKernelArgs& a, bool autoturn, bool shaped, const void* actions, int act_type, void* obs,
                          int32_t* reward, uint8_t* done, uint8_t* info, int n_steps, bool fused, hipStream_t stream) {
  // threads per workgroup: the smallest of 64 / 128 / 256 that still makes a workgroup per CU (256 of them) -- see sf_step_kernel
  int blk = fused ? SF_BLOCK : (a.lanes <= 64 * 256 ? 64 : (a.lanes <= 128 * 256 ? 128 : SF_BLOCK));
  const size_t elem = a.obs_f64 ? sizeof(double) : sizeof(float);
  // 16-byte obs stores need every tick's row of the output to start 16-byte aligned
  const int vec_ok = ((uintptr_t)obs & 15u) == 0 && (!fused || ((size_t)a.n_envs * a.obs_dim * elem) % 16 == 0);
  // the default observation has its own instantiations (OBSK = 1): see write_features_f32
  const bool fast_obs = obs != nullptr && a.obs_type == 0 && !a.obs_f64 && vec_ok && a.n_envs % 64 == 0 &&
                        a.obs_dim == (autoturn ? 17 : 19) && !a.ref_reset_obs;
  // (the final-observation output: the XTRA instantiations' FOBS twins, whatever else the launch asks for)
  const bool fobs = a.final_obs != nullptr;
  const bool xtra = act_type == SF_ACT_SAMPLED || a.act_out != nullptr || !a.auto_reset || fobs;
  // a split launch (sf_step_kernel: a missile wave per tile) where a tile's wave is alone on its SIMD otherwise
  // (SF_SPLIT 2, for tests: every batch it can serve)
  // (SFMI_FORCE_SPLIT=1 in the environment, for tests: every batch the instantiation can serve; =2 says so once on stderr)
  static const int force_split = [] { const char* e = getenv("SFMI_FORCE_SPLIT"); return e ? atoi(e) : 0; }();
  const bool split = SF_SPLIT && !fused && fast_obs && !xtra && (a.lanes <= 65536 || SF_SPLIT == 2 || force_split) && a.draw == nullptr;
  if (split && force_split == 2) {
    static bool said = false;
    if (!said) fprintf(stderr, "sfmi: split launch (%ld lanes)\n", (long)a.lanes);
    said = true;
  }
  const unsigned grid = (unsigned)(a.lanes / blk);
  // (sf_step_kernel's LDS map: the cos/sin table, the event words, the atan table -- a split launch: the staged constants
  //  block, the event words, the hand-over words -- then the observation staging rows)
  size_t lds_bytes = (size_t)(SF_LDS_DOUBLES + blk + SF_ATAB_DOUBLES) * sizeof(double) + (size_t)blk * a.obs_dim * elem;
  if (split) lds_bytes = (size_t)(SF_LDS_SPLIT_DOUBLES + blk + 2 * (2 * blk + blk / 2) + blk / 32) * sizeof(double) + (size_t)blk * a.obs_dim * elem;
#define SF_GO2(AT, SH, FU, OK, XT, BL, FO)                                                                            \
  hipLaunchKernelGGL((sf_step_kernel<AT, SH, FU, OK, XT, BL, FO>), dim3(grid), dim3((BL) > 1000 ? 2 * ((BL) - 1000) : (BL)), lds_bytes, stream, a.state,    \
                     a.consts, actions, a.n_envs, act_type, reward, done, info, a, obs, vec_ok, n_steps)
#define SF_GO1(AT, SH, FU, OK, XT, FO)                                                                             \
  do {                                                                                                             \
    if (FU || blk == SF_BLOCK) SF_GO2(AT, SH, FU, OK, XT, SF_BLOCK, FO);                                           \
    else if (blk == 128) SF_GO2(AT, SH, false, OK, XT, 128, FO);                                                   \
    else SF_GO2(AT, SH, false, OK, XT, 64, FO);                                                                    \
  } while (0)
#if SF_SPLIT
#define SF_GO_SPLIT(AT, SH)                                                                                        \
  if (split) {                                                                                                     \
    if (blk == SF_BLOCK) SF_GO2(AT, SH, false, 1, false, 1256, false);                                             \
    else if (blk == 128) SF_GO2(AT, SH, false, 1, false, 1128, false);                                             \
    else SF_GO2(AT, SH, false, 1, false, 1064, false);                                                             \
  } else
#else
#define SF_GO_SPLIT(AT, SH)
#endif
#define SF_GO(AT, SH, FU)                                                                                          \
  SF_GO_SPLIT(AT, SH)                                                                                              \
  if (fast_obs) {                                                                                                  \
    if (fobs) SF_GO1(AT, SH, FU, 1, true, true);                                                                   \
    else if (xtra) SF_GO1(AT, SH, FU, 1, true, false); else SF_GO1(AT, SH, FU, 1, false, false);                   \
  } else {                                                                                                         \
    if (fobs) SF_GO1(AT, SH, FU, 0, true, true);                                                                   \
    else if (xtra) SF_GO1(AT, SH, FU, 0, true, false); else SF_GO1(AT, SH, FU, 0, false, false);                   \
  }
  // the four presets of SRC/configs.cpp:51-89 are exactly (autoTurn) x (shaped scoring)
  const int sel = (autoturn ? 4 : 0) | (shaped ? 2 : 0) | (fused ? 1 : 0);
  switch (sel) {
    case 0: SF_GO(false, false, false); break;
    case 1: SF_GO(false, false, true); break;
    case 2: SF_GO(false, true, false); break;
    case 3: SF_GO(false, true, true); break;
    case 4: SF_GO(true, false, false); break;
    case 5: SF_GO(true, false, true); break;
    case 6: SF_GO(true, true, false); break;
    default: SF_GO(true, true, true); break;
  }
#undef SF_GO
#undef SF_GO1
#undef SF_GO_SPLIT
#undef SF_GO2
  return hipGetLastError();
}

// sf_step_repeat (sfmi_repeat.h): `repeat` ticks of one action per env in ONE launch of a REPEAT instantiation (BLKP = 2000 +
// SF_BLOCK; sf_step_kernel), one row of outputs; `ticks` (uint8 [n_envs], may be null) travels in a.act_out, which no REPEAT
// launch uses for anything else.  The batch auto-resets (the caller checked).
hipError_t sf_launch_step_repeat(const SfKernelArgs& a0, bool autoturn, bool shaped, const void* actions, int act_type, void* obs,
                                 int32_t* reward, uint8_t* done, uint8_t* info, uint8_t* ticks, int repeat, hipStream_t stream) {
  SfKernelArgs a = a0;
  a.act_out = ticks;
  const size_t elem = a.obs_f64 ? sizeof(double) : sizeof(float);
  const int vec_ok = ((uintptr_t)obs & 15u) == 0;  // (one row of observations: row 0)
  const bool fast_obs = obs != nullptr && a.obs_type == 0 && !a.obs_f64 && vec_ok && a.n_envs % 64 == 0 &&
                        a.obs_dim == (autoturn ? 17 : 19) && !a.ref_reset_obs;
  const unsigned grid = (unsigned)(a.lanes / SF_BLOCK);
  const size_t lds_bytes = (size_t)(SF_LDS_DOUBLES + SF_BLOCK + SF_ATAB_DOUBLES) * sizeof(double) + (size_t)SF_BLOCK * a.obs_dim * elem;
#define SF_GO(AT, SH)                                                                                                       \
  do {                                                                                                                      \
    if (fast_obs)                                                                                                           \
      hipLaunchKernelGGL((sf_step_kernel<AT, SH, true, 1, true, 2000 + SF_BLOCK, false>), dim3(grid), dim3(SF_BLOCK), lds_bytes, \
                         stream, a.state, a.consts, actions, a.n_envs, act_type, reward, done, info, a, obs, vec_ok, repeat);  \
    else                                                                                                                    \
      hipLaunchKernelGGL((sf_step_kernel<AT, SH, true, 0, true, 2000 + SF_BLOCK, false>), dim3(grid), dim3(SF_BLOCK), lds_bytes, \
                         stream, a.state, a.consts, actions, a.n_envs, act_type, reward, done, info, a, obs, vec_ok, repeat);  \
  } while (0)
  switch ((autoturn ? 2 : 0) | (shaped ? 1 : 0)) {
    case 0: SF_GO(false, false); break;
    case 1: SF_GO(false, true); break;
    case 2: SF_GO(true, false); break;
    default: SF_GO(true, true); break;
  }
#undef SF_GO
  return hipGetLastError();
}
