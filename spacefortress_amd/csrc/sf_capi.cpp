// sf_capi.cpp -- the C ABI of include/sfmi.h: batch lifecycle, step/reset launches, the accumulator readers.
// Host code only; the kernels are in sf_kernels.hip (reset, step).  What draws is in sf_image_capi.cpp, field access and the
// lane states in sf_state_capi.cpp; the batch itself is sf_batch.h.  There is no CPU implementation of the path in this
// library: every entry point that computes needs a HIP device.
#include <limits.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "sf_batch.h"
#include "sf_raster.h"

namespace {

const unsigned long long kAccInit[SF_ACC_WORDS] = {
    0, 0, 0, 0, 0, 0, (unsigned long long)LLONG_MAX, (unsigned long long)LLONG_MIN, 0, 0, 0};
static_assert(SF_ACC_BAD_ACTION == SF_EPISODE_STATS_LEN && SF_ACC_OVERFLOW == SF_EPISODE_STATS_LEN + 1, "acc layout");

// the sampler records of sf_step_sampled (sf_layout.h: SF_ACT_SAMPLED): per tile (tick, key0, key1, first lane of the job)
int write_action_records(sf_batch* b, uint64_t seed, uint32_t first_lane, hipStream_t stream) {
  const size_t tiles = (size_t)(b->args.lanes / 64);
  std::vector<uint32_t> rec(4 * tiles);
  for (size_t t = 0; t < tiles; t++) {
    rec[4 * t + 0] = 0u;
    rec[4 * t + 1] = (uint32_t)seed;
    rec[4 * t + 2] = (uint32_t)(seed >> 32);
    rec[4 * t + 3] = first_lane + (uint32_t)(64 * t);
  }
  HIP_TRY(hipMemcpyAsync(b->d_actrec.get(), rec.data(), rec.size() * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  HIP_TRY(hipStreamSynchronize(stream));  // `rec` is pageable host memory that dies with this call
  return SF_OK;
}

bool is_pow2(long v) { return v > 0 && (v & (v - 1)) == 0; }

// `count` zeroed T on the device
template <typename T>
int alloc_zeroed(DevBuf<T>& d, size_t count) {
  HIP_TRY(d.alloc(count));
  HIP_TRY(hipMemset(d.get(), 0, count * sizeof(T)));
  return SF_OK;
}

}  // namespace

extern "C" int sf_create(const sf_create_params* p, sf_batch** out) {
  if (!p || !out || !p->gametype) {
    sf_set_error("sf_create: null argument");
    return SF_ERR_ARG;
  }
  *out = nullptr;
  sf_preset preset;
  int rc = sf_preset_get(p->gametype, &preset);
  if (rc != SF_OK) return rc;
  if (p->n_envs <= 0) {
    sf_set_error("sf_create: n_envs must be positive (got %d)", p->n_envs);
    return SF_ERR_ARG;
  }
  if (p->obs_type < SF_OBS_FEATURES || p->obs_type > SF_OBS_IMAGE_RAW) {
    // ENV:51 assert obs_type in ('image', 'features', 'normalized-features', 'monitors')
    sf_set_error("sf_create: unsupported obs_type %d", p->obs_type);
    return SF_ERR_ARG;
  }
  uint8_t keys[16];
  int n_actions = sf_action_table(p->gametype, p->action_set, keys);
  if (n_actions < 0) return n_actions;
  if (p->spawn_skip < 0 || p->spawn_stride < 0) {
    sf_set_error("sf_create: spawn_skip / spawn_stride must be >= 0");
    return SF_ERR_ARG;
  }
  // Lane i starts at entry spawn_skip + spawn_stride * i of the accepted-spawn sequence and must be able to walk on
  // from there as the libc stream does (SRC/game.cpp:133-149), not wrap into somebody else's stretch: the default
  // table reaches SF_SPAWN_MARGIN entries (about 370 episodes of respawns) past the LAST lane's start.
  const long last_start = (long)p->spawn_skip + (long)p->spawn_stride * ((long)p->n_envs - 1);
  long spawn_len = p->spawn_table_len;
  if (spawn_len == 0) {
    spawn_len = 65536;
    while (spawn_len < last_start + SF_SPAWN_MARGIN && spawn_len < (1l << 24)) spawn_len <<= 1;
  }
  if (!is_pow2(spawn_len) || spawn_len > (1l << 24)) {
    sf_set_error("sf_create: spawn_table_len must be a power of two <= 2^24 (got %ld)", spawn_len);
    return SF_ERR_ARG;
  }
  if (last_start >= spawn_len) {
    sf_set_error("sf_create: lane %d would start at entry %ld of a %ld-entry spawn table (spawn_skip %d, spawn_stride %d): "
                 "pass a larger spawn_table_len (<= 2^24) or smaller offsets", p->n_envs - 1, last_start, spawn_len,
                 p->spawn_skip, p->spawn_stride);
    return SF_ERR_ARG;
  }

  int n_dev = 0;
  hipError_t e = hipGetDeviceCount(&n_dev);
  if (e != hipSuccess || n_dev <= 0) {
    sf_set_error("sf_create: no HIP device available (%s); libsfmi has no CPU path",
                 e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    return SF_ERR_NO_DEVICE;
  }
  if (p->device_id < 0 || p->device_id >= n_dev) {
    sf_set_error("sf_create: device_id %d out of range (%d devices)", p->device_id, n_dev);
    return SF_ERR_ARG;
  }
  DeviceGuard guard(p->device_id);

  // (behind the guard: an error return frees what the batch holds so far, on its device)
  std::unique_ptr<sf_batch> owner(new sf_batch());
  sf_batch* const b = owner.get();
  b->preset = preset;
  b->autoturn = preset.auto_turn != 0;
  b->device = p->device_id;
  b->n_envs = p->n_envs;
  b->act_count = n_actions;
  b->spawn_skip = p->spawn_skip;
  b->spawn_stride = p->spawn_stride;
  b->seed = p->seed;
  b->spawn_len = spawn_len;
  b->obs_mode = p->obs_type;

  const long lanes = ((long)p->n_envs + 255) / 256 * 256;
  const size_t tiles = (size_t)(lanes / 64);
  b->state_bytes = (size_t)sfl::kBytesPerLane * lanes;

  // host tables
  std::vector<double> consts(SF_CONST_DOUBLES);
  sf_host_fill_consts(preset, consts.data());
  // Everything else of baseConfig (SRC/configs.cpp:3-49) is identical in the four presets and is compiled into the kernels
  // (namespace sfc).  Refuse to run if a preset ever disagrees with what was compiled in.
  if (!sf_preset_compiled_in(preset, consts.data())) {
    sf_set_error("sf_create: preset `%s' differs from the constants compiled into the kernels", p->gametype);
    return SF_ERR_ARG;
  }
  std::vector<int16_t> spawn(4 * (size_t)spawn_len);
  SF_TRY(sf_spawn_table(p->seed, (int)spawn_len, spawn.data()));

  // the state and its tables
  SF_TRY(alloc_zeroed(b->d_state, b->state_bytes));  // dead projectile slots are read (and ignored): keep them defined
  HIP_TRY(b->d_consts.alloc(consts.size()));
  HIP_TRY(b->d_spawn.alloc(spawn.size()));
  HIP_TRY(b->d_acc.alloc(SF_ACC_WORDS));
  HIP_TRY(b->d_scratch.alloc((size_t)p->n_envs * SF_NSLOT * 16));
  HIP_TRY(hipMemcpy(b->d_consts.get(), consts.data(), consts.size() * sizeof(double), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b->d_spawn.get(), spawn.data(), spawn.size() * sizeof(int16_t), hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(b->d_acc.get(), kAccInit, sizeof(kAccInit), hipMemcpyHostToDevice));
  HIP_TRY(b->d_actrec.alloc(tiles * 4));
  {
    // the lane-state load's bookkeeping: map [lanes] int32 (-1), tile flags and list [lanes / 64], list length, refusals
    const size_t map_b = (size_t)lanes * 4, rest = tiles * 8 + 16;
    HIP_TRY(b->d_lanes.alloc(map_b + rest));
    unsigned char* const base = b->d_lanes.get();
    HIP_TRY(hipMemset(base, 0xFF, map_b));
    HIP_TRY(hipMemset(base + map_b, 0, rest));
    b->d_lmap = (int*)base;
    b->d_ltflag = (unsigned*)(base + map_b);
    b->d_ltlist = b->d_ltflag + tiles;
    b->d_lrefused = (unsigned long long*)(b->d_ltlist + tiles);
    b->d_ltcount = (unsigned*)(b->d_lrefused + 1);
  }
  SF_TRY(sfb_create_image_tables(b));

  SfKernelArgs& a = b->args;
  a.state = b->d_state.get();
  a.lanes = lanes;
  a.n_envs = p->n_envs;
  a.consts = b->d_consts.get();
  a.spawn = b->d_spawn.get();
  a.spawn_mask = (unsigned)(spawn_len - 1);
  a.action_keys = 0;
  for (int i = 0; i < n_actions; i++) a.action_keys |= (unsigned long long)(keys[i] & 0xF) << (4 * i);
  a.n_actions = n_actions;
  a.start_vx = preset.start_vx;  // libm values of the host, SRC/configs.cpp:43-44
  a.start_vy = preset.start_vy;
  const bool image = sfb_is_image(b);
  a.obs_type = image ? SF_OBS_NONE : p->obs_type;  // frames come from sf_render, after the step kernel
  a.obs_f64 = (p->flags & SF_FLAG_OBS_F64) ? 1 : 0;
  a.real_shell_count = (p->flags & SF_FLAG_REAL_SHELL_COUNT) ? 1 : 0;
  a.auto_reset = (p->flags & SF_FLAG_NO_AUTO_RESET) ? 0 : 1;
  a.ref_reset_obs = (p->flags & SF_FLAG_REF_RESET_OBS) ? 1 : 0;
  a.obs_dim = p->obs_type == SF_OBS_MONITORS ? 10 : ((p->obs_type == SF_OBS_NONE || image) ? 0 : 15 + preset.n_keys);
  static_assert(sfc::pb_width == (double)(int)(450 * .2) && sfc::pb_height == (double)(int)(460 * .2), "ENV:57-58");
  static_assert(sfc::max_ticks == (double)(sfc::game_time / sfc::tick_ms), "ENV:165");
  a.acc = b->d_acc.get();
  SF_TRY(write_action_records(b, p->seed, 0u, nullptr));  // sf_step_sampled's default stream: (seed, lane, tick 0)
  if (image && !getenv("SFMI_NO_RENDER_ORDER")) {  // the render kernel's launch order (sf_render.hip: pick_env)
    SF_TRY(alloc_zeroed(b->d_hint, tiles));
    a.hint = b->d_hint.get();
  }
#ifdef SF_STAMPS  // diagnostic build (tools/stamps.py): per-wave clock stamps, never in the product
  SF_TRY(alloc_zeroed(b->d_dbg, tiles * SF_STAMP_SLOTS));
  a.dbg = b->d_dbg.get();
#endif

  // the first games
  HIP_TRY(sf_launch_reset(a, 1, (unsigned)p->spawn_skip, (unsigned)p->spawn_stride, nullptr, nullptr));
  HIP_TRY(hipStreamSynchronize(nullptr));
  if (image) {  // the render caches and pictures, and the draw records the step launches of this batch keep current
    SF_TRY(sfb_ensure_render_resources(b, nullptr));
    a.draw = b->d_draw.get();
    a.draw_pics = b->d_xcache ? 1 : 0;
  }
  *out = owner.release();
  return SF_OK;
}

extern "C" int sf_destroy(sf_batch* b) {
  if (!b) return SF_OK;
  DeviceGuard guard(b->device);  // (in scope while the batch's buffers are freed)
  delete b;
  return SF_OK;
}

#ifdef SF_STAMPS
extern "C" int sf_debug_slots(void) { return SF_STAMP_SLOTS; }  // stamps per wave: the width of sf_debug_read's rows
extern "C" int sf_debug_read(sf_batch* b, unsigned long long* host) {
  DeviceGuard guard(b->device);
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(host, b->args.dbg, (size_t)(b->args.lanes / 64) * SF_STAMP_SLOTS * sizeof(unsigned long long),
                    hipMemcpyDeviceToHost));
  return SF_OK;
}
#endif

extern "C" int sf_n_envs(const sf_batch* b) { return b ? b->n_envs : SF_ERR_ARG; }
extern "C" int sf_obs_dim(const sf_batch* b) {
  if (!b) return SF_ERR_ARG;
  if (b->obs_mode == SF_OBS_IMAGE) return SF_OUT * SF_OUT;
  if (b->obs_mode == SF_OBS_IMAGE_RAW) return b->g_w ? b->g_w * b->g_h : SF_IMG_W * SF_IMG_H;
  return b->args.obs_dim;
}
extern "C" int sf_n_actions(const sf_batch* b) { return b ? b->act_count : SF_ERR_ARG; }
extern "C" int sf_tick_ms(const sf_batch* b) { return b ? sfc::tick_ms : SF_ERR_ARG; }
extern "C" int sf_max_ticks(const sf_batch* b) { return b ? (int)sfc::max_ticks : SF_ERR_ARG; }

extern "C" int sf_reset(sf_batch* b, void* obs_dev, void* stream) {
  if (!b) {
    sf_set_error("sf_reset: null batch");
    return SF_ERR_ARG;
  }
  DeviceGuard guard(b->device);
  const bool image = sfb_is_image(b);
  b->mslots_dirty = false;  // new games everywhere: no missiles, whatever a caller wrote into the slot view
  b->draw_current = false;
  HIP_TRY(hipMemsetAsync(b->d_acc.get() + SF_ACC_OVERFLOW, 0, sizeof(unsigned long long), (hipStream_t)stream));  // new games: nothing is wrapped
  HIP_TRY(sf_launch_reset(b->args, 0, 0, 0, image ? nullptr : obs_dev, (hipStream_t)stream));
  if (image && obs_dev) return sfb_render(b, b->obs_mode, (uint8_t*)obs_dev, 0, (hipStream_t)stream);
  return SF_OK;
}

extern "C" int sf_reset_lanes(sf_batch* b, const uint8_t* mask_dev, void* obs_dev, void* stream) {
  if (!b) {
    sf_set_error("sf_reset_lanes: null batch");
    return SF_ERR_ARG;
  }
  if (!mask_dev) {
    sf_set_error("sf_reset_lanes: null mask (uint8 [n_envs] on the device; sf_reset restarts every env)");
    return SF_ERR_ARG;
  }
  DeviceGuard guard(b->device);
  const bool image = sfb_is_image(b);
  SF_FLUSH_VIEW(b, stream);  // (the kept lanes' missiles as a caller edited them)
  // (the episode accumulators, the sticky overflow count and the sampler's tick stay: an abandoned game is no finished episode)
  HIP_TRY(sf_launch_reset_lanes(b->args, mask_dev, image ? nullptr : obs_dev, (hipStream_t)stream));
  b->draw_current = false;
  // an image batch whose resources exist: its draw records follow the state at once
  if (b->args.draw && b->render_ready) SF_TRY(sfb_rebuild_draw_records(b, (hipStream_t)stream));
  if (image && obs_dev) return sfb_render(b, b->obs_mode, (uint8_t*)obs_dev, 0, (hipStream_t)stream);
  return SF_OK;
}

// One step launch as an entry point asks for it: what sf_step, sf_step_record, sf_rollout, ... differ in.
struct StepLaunch {
  const char* who;                // the entry point's name in error texts
  const void* actions = nullptr;  // the caller's action array, or the batch's sampler records (act_type SF_ACT_SAMPLED)
  int act_type = SF_ACT_SAMPLED;
  int n_steps = 1;
  bool fused = false;  // a rollout: the n_steps ticks in ONE launch (unless an image batch's frames are asked for)
  int32_t* reward = nullptr;
  uint8_t* done = nullptr;
  uint8_t* info = nullptr;
  int repeat = 1;            // > 1: ONE launch plays every env's action for up to `repeat` ticks (sf_step_repeat)
  uint8_t* ticks = nullptr;  // ... and says here how many each env played
  // optional patches to the batch's SfKernelArgs
  float *t_reward = nullptr, *t_mask = nullptr, *t_episode = nullptr, *t_final = nullptr;  // trainer outputs (sf_step_record)
  int64_t* t_actions = nullptr;
  uint8_t* act_out = nullptr;  // the sampled actions
  double *n_partials = nullptr, *n_ret = nullptr;  // the normaliser's partial sums and returns
  double n_gamma = 0.0;
  const uint8_t* active = nullptr;  // sf_step_where: uint8 [n_envs], zero = the env is held around the launch (sfmi_hold.h)
};

static int check_act_type(const char* who, int act_type) {
  if (act_type != SF_ACT_U8 && act_type != SF_ACT_I32 && act_type != SF_ACT_I64) {
    sf_set_error("%s: act_type must be 1, 4 or 8 (got %d)", who, act_type);
    return SF_ERR_ARG;
  }
  return SF_OK;
}

// a step launch of launch_steps: if it fails behind a queued hold-begin, the held envs are still put back (their chunks and pool
// entries live only in the stash, which the next masked step overwrites) before the error is returned
#define STEP_TRY(expr)                                                                              \
  do {                                                                                              \
    const hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess) {                                                                         \
      (void)held_back();                                                                            \
      sf_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__);      \
      return SF_ERR_HIP;                                                                            \
    }                                                                                               \
  } while (0)

// guard -> flush -> launch -> draw_current -> frames: the one path from an entry point to sf_launch_step / sf_launch_step_repeat
static int launch_steps(sf_batch* b, const StepLaunch& d, void* obs_dev, void* stream) {
  DeviceGuard guard(b->device);
  const bool image = sfb_is_image(b), sampled = d.act_type == SF_ACT_SAMPLED;
  SfKernelArgs args = b->args;
  if (d.t_reward) {
    args.t_reward = d.t_reward;
    args.t_mask = d.t_mask;
    args.t_episode = d.t_episode;
    args.t_final = d.t_final;
    args.t_actions = (long long*)d.t_actions;
  }
  if (sampled) args.act_out = d.act_out;
  if (d.n_partials) {
    args.n_partials = d.n_partials;
    args.n_ret = d.n_ret;
    args.n_gamma = d.n_gamma;
  }
  const void* actions = sampled ? b->d_actrec.get() : d.actions;
  // final frames (sfmi_final.h): the step launches run with auto-reset off, tick by tick, and every one is followed by the
  // finished envs' frames and their finish -- totals, new games, draw records (sfb_finish_with_final_frames)
  const bool finals = b->final_frames != nullptr;
  if (finals) {
    SF_TRY(sfb_final_frames_fit(b, d.who));
    args.auto_reset = 0;
  }
  SF_FLUSH_VIEW(b, stream);
  // a masked step: the held envs leave in front of the launch and come back behind it, with their output rows -- and, image
  // batches, their draw records -- in front of the frames
  if (d.active) HIP_TRY(sf_launch_hold_begin(args, d.active, b->d_hold.get(), (hipStream_t)stream));
  const auto held_back = [&]() -> hipError_t {
    if (!d.active) return hipSuccess;
    return sf_launch_hold_end(args, d.active, b->d_hold.get(), image ? nullptr : obs_dev, d.reward, d.done, d.info, d.ticks,
                              d.repeat == 1, (hipStream_t)stream);  // (sf_step says no ticks: every active env played its one)
  };
  if (d.repeat > 1) {  // one REPEAT launch; an image batch's frame: one sfb_render from the draw records it left
    STEP_TRY(sf_launch_step_repeat(args, b->autoturn, b->preset.shaped != 0, actions, d.act_type, image ? nullptr : obs_dev, d.reward,
                                  d.done, d.info, d.ticks, d.repeat, (hipStream_t)stream));
    HIP_TRY(held_back());
    b->draw_current = b->args.draw != nullptr;  // (the draw records of the state the window ends in)
    if (image && obs_dev) return sfb_render(b, b->obs_mode, (uint8_t*)obs_dev, 0, (hipStream_t)stream);
    return SF_OK;
  }
  if (!(image && obs_dev) && !finals) {
    STEP_TRY(sf_launch_step(args, b->autoturn, b->preset.shaped != 0, actions, d.act_type, image ? nullptr : obs_dev, d.reward,
                           d.done, d.info, d.n_steps, d.fused, (hipStream_t)stream));
    HIP_TRY(held_back());
    b->draw_current = b->args.draw != nullptr;  // (an image batch's step launch leaves the draw records of the new state)
    return SF_OK;
  }
  // frames are rendered from the state in HBM, which the fused launch keeps in registers: with frames asked for, the K ticks
  // go out as K step launches, each followed by its frames -- what K sf_step calls do, in one call.  (Sampled actions: the
  // tiles' tick counters move on by one per launch, so the actions drawn are the fused launch's.)
  // (final frames: the same K launches with or without frames asked for -- the finish needs the state in HBM between ticks)
  const size_t n = (size_t)b->n_envs, frame = (size_t)sf_obs_dim(b);
  for (int t = 0; t < d.n_steps; t++) {
    const size_t row = (size_t)t * n;  // (a rollout's outputs, event masks included, are [n_steps][n_envs])
    SfKernelArgs at = args;
    if (at.act_out) at.act_out += row;
    if (at.events) at.events += row;
    uint8_t* const done_t = d.done ? d.done + row : (finals ? b->d_fdone.get() : nullptr);  // (the finish reads the tick's done bytes)
    STEP_TRY(sf_launch_step(at, b->autoturn, b->preset.shaped != 0,
                           sampled ? actions : (const unsigned char*)actions + row * (size_t)d.act_type, d.act_type, nullptr,
                           d.reward ? d.reward + row : nullptr, done_t, d.info ? d.info + row : nullptr,
                           1, false, (hipStream_t)stream));
    HIP_TRY(held_back());  // (a masked step is one tick: n_steps == 1)
    if (finals) SF_TRY(sfb_finish_with_final_frames(b, done_t, (hipStream_t)stream));
    b->draw_current = b->args.draw != nullptr;
    if (!obs_dev) continue;
    const int rc = sfb_render(b, b->obs_mode, (uint8_t*)obs_dev + row * frame, 0, (hipStream_t)stream);
    if (rc != SF_OK) return rc;
  }
  return SF_OK;
}
#undef STEP_TRY

extern "C" int sf_step(sf_batch* b, const void* actions_dev, int act_type, void* obs_dev, int32_t* reward_dev,
                       uint8_t* done_dev, uint8_t* info_dev, void* stream) {
  if (!b || !actions_dev) {
    sf_set_error("sf_step: null batch or actions");
    return SF_ERR_ARG;
  }
  StepLaunch d{"sf_step", actions_dev, act_type, 1, false, reward_dev, done_dev, info_dev};
  if (check_act_type(d.who, act_type) != SF_OK) return SF_ERR_ARG;
  return launch_steps(b, d, obs_dev, stream);
}

// sfmi_repeat.h.  One REPEAT launch of the step kernel; an image batch's frames: one sfb_render from the draw records it left.
extern "C" int sf_step_repeat(sf_batch* b, const void* actions_dev, int act_type, int repeat, void* obs_dev, int32_t* reward_dev,
                              uint8_t* done_dev, uint8_t* info_dev, uint8_t* ticks_dev, void* stream) {
  if (!b || !actions_dev) {
    sf_set_error("sf_step_repeat: null batch or actions");
    return SF_ERR_ARG;
  }
  if (check_act_type("sf_step_repeat", act_type) != SF_OK) return SF_ERR_ARG;
  if (repeat < 1 || repeat > 255) {
    sf_set_error("sf_step_repeat: repeat must be in [1, 255] (got %d)", repeat);
    return SF_ERR_ARG;
  }
  if (!b->args.auto_reset) {
    sf_set_error("sf_step_repeat: a SF_FLAG_NO_AUTO_RESET batch has no action repeat: an env that finishes inside the window "
                 "would have to be frozen in place, and a parked lane is given its new game; step such a batch tick by tick");
    return SF_ERR_ARG;
  }
  if (repeat > 1 && b->final_frames) {
    sf_set_error("sf_step_repeat: no action repeat while a final-frame output is set (sf_set_final_frame_output): an env parked "
                 "inside the window no longer holds its last frame's state; final frames of a repeat window are a follow-up -- "
                 "switch the output off (NULL) or step with repeat 1");
    return SF_ERR_ARG;
  }
  StepLaunch d{"sf_step_repeat", actions_dev, act_type, 1, false, reward_dev, done_dev, info_dev, repeat, ticks_dev};
  const int rc = launch_steps(b, d, obs_dev, stream);
  if (rc != SF_OK || repeat > 1) return rc;
  // repeat == 1 was sf_step itself; every env played its one tick
  DeviceGuard guard(b->device);
  if (ticks_dev) HIP_TRY(hipMemsetAsync(ticks_dev, 1, (size_t)b->n_envs, (hipStream_t)stream));
  return SF_OK;
}

// sfmi_hold.h.  launch_steps' path with the two hold launches around the step launch; the stash is the batch's, made here once.
extern "C" int sf_step_where(sf_batch* b, const uint8_t* active_dev, const void* actions_dev, int act_type, int repeat, void* obs_dev,
                             int32_t* reward_dev, uint8_t* done_dev, uint8_t* info_dev, uint8_t* ticks_dev, void* stream) {
  if (!b || !active_dev || !actions_dev) {
    sf_set_error("sf_step_where: null batch, mask or actions (the mask: uint8 [n_envs] on the device, non-zero = the env steps)");
    return SF_ERR_ARG;
  }
  if (check_act_type("sf_step_where", act_type) != SF_OK) return SF_ERR_ARG;
  if (repeat < 1 || repeat > 255) {
    sf_set_error("sf_step_where: repeat must be in [1, 255] (got %d)", repeat);
    return SF_ERR_ARG;
  }
  if (repeat > 1 && !b->args.auto_reset) {
    sf_set_error("sf_step_where: a SF_FLAG_NO_AUTO_RESET batch has no action repeat (sf_step_repeat: an ACTIVE env that finishes "
                 "inside the window would be given its new game); step such a batch with repeat 1");
    return SF_ERR_ARG;
  }
  if (b->final_frames) {
    sf_set_error("sf_step_where: no masked step while a final-frame output is set (sf_set_final_frame_output): the held envs' "
                 "stand-ins would finish and restart in their place; final frames of a masked step are a follow-up -- switch "
                 "the output off (NULL) first");
    return SF_ERR_ARG;
  }
  if (!b->d_hold) {  // the first masked step of this batch (not capturable: it allocates)
    DeviceGuard guard(b->device);
    HIP_TRY(b->d_hold.alloc(b->state_bytes));
    HIP_TRY(hipMemsetAsync(b->d_hold.get(), 0, b->state_bytes, (hipStream_t)stream));
  }
  StepLaunch d{"sf_step_where", actions_dev, act_type, 1, false, reward_dev, done_dev, info_dev, repeat, ticks_dev};
  d.active = active_dev;
  return launch_steps(b, d, obs_dev, stream);
}

int sf_step_with_norm_partials(sf_batch* b, const void* actions_dev, int act_type, void* obs_dev, int32_t* reward_dev,
                               uint8_t* done_dev, uint8_t* info_dev, double* partials, double* ret, double gamma, int* rows_out,
                               void* stream) {
  if (!b || !actions_dev || !partials) {
    sf_set_error("sf_step_normalize: null batch, actions or normalizer");
    return SF_ERR_ARG;
  }
  StepLaunch d{"sf_step_normalize", actions_dev, act_type, 1, false, reward_dev, done_dev, info_dev};
  if (check_act_type(d.who, act_type) != SF_OK) return SF_ERR_ARG;
  if (sfb_is_image(b) || b->args.obs_dim < 4) {
    sf_set_error("sf_step_normalize: VecNormalize applies to 1-D observations (rl/train.py:35)");
    return SF_ERR_ARG;
  }
  d.n_partials = partials;
  d.n_ret = ret;
  d.n_gamma = gamma;
  const int rc = launch_steps(b, d, obs_dev, stream);
  if (rc != SF_OK) return rc;
  *rows_out = (int)(b->args.lanes / 64);
  return SF_OK;
}

extern "C" int sf_step_record(sf_batch* b, const void* actions_dev, int act_type, void* obs_dev, int32_t* reward_dev,
                              uint8_t* done_dev, uint8_t* info_dev, float* reward_f32, float* mask_f32, float* episode_rewards,
                              float* final_rewards, int64_t* actions_out, void* stream) {
  if (!b || !actions_dev || !reward_f32) {
    sf_set_error("sf_step_record: null batch, actions or reward_f32");
    return SF_ERR_ARG;
  }
  StepLaunch d{"sf_step_record", actions_dev, act_type, 1, false, reward_dev, done_dev, info_dev};
  if (check_act_type(d.who, act_type) != SF_OK) return SF_ERR_ARG;
  if (((uintptr_t)reward_f32 | (uintptr_t)mask_f32 | (uintptr_t)episode_rewards | (uintptr_t)final_rewards) & 3 ||
      ((uintptr_t)actions_out & 7)) {
    sf_set_error("sf_step_record: float outputs must be 4-byte, actions_out 8-byte aligned");
    return SF_ERR_ARG;
  }
  d.t_reward = reward_f32;  // (never null here: it is what switches the trainer outputs on)
  d.t_mask = mask_f32;
  d.t_episode = episode_rewards;
  d.t_final = final_rewards;
  d.t_actions = actions_out;
  return launch_steps(b, d, obs_dev, stream);
}

extern "C" int sf_rollout(sf_batch* b, const void* actions_dev, int act_type, int n_steps, void* obs_dev,
                          int32_t* reward_dev, uint8_t* done_dev, uint8_t* info_dev, void* stream) {
  if (!b || !actions_dev) {
    sf_set_error("sf_rollout: null batch or actions");
    return SF_ERR_ARG;
  }
  StepLaunch d{"sf_rollout", actions_dev, act_type, n_steps, true, reward_dev, done_dev, info_dev};
  if (check_act_type(d.who, act_type) != SF_OK) return SF_ERR_ARG;
  if (n_steps <= 0 || (double)n_steps * b->n_envs * 8.0 >= 4294967296.0) {
    sf_set_error("sf_rollout: n_steps must be positive and n_steps * n_envs * 8 < 2^32 (got %d)", n_steps);
    return SF_ERR_ARG;
  }
  return launch_steps(b, d, obs_dev, stream);
}

extern "C" int sf_seed_actions(sf_batch* b, uint64_t seed, uint32_t first_lane, void* stream) {
  if (!b) {
    sf_set_error("sf_seed_actions: null batch");
    return SF_ERR_ARG;
  }
  DeviceGuard guard(b->device);
  return write_action_records(b, seed, first_lane, (hipStream_t)stream);
}

extern "C" int sf_step_sampled(sf_batch* b, uint8_t* actions_out_dev, void* obs_dev, int32_t* reward_dev, uint8_t* done_dev,
                               uint8_t* info_dev, void* stream) {
  if (!b) {
    sf_set_error("sf_step_sampled: null batch");
    return SF_ERR_ARG;
  }
  StepLaunch d{"sf_step_sampled", nullptr, SF_ACT_SAMPLED, 1, false, reward_dev, done_dev, info_dev};
  d.act_out = actions_out_dev;
  return launch_steps(b, d, obs_dev, stream);
}

extern "C" int sf_rollout_sampled(sf_batch* b, int n_steps, uint8_t* actions_out_dev, void* obs_dev, int32_t* reward_dev,
                                  uint8_t* done_dev, uint8_t* info_dev, void* stream) {
  if (!b) {
    sf_set_error("sf_rollout_sampled: null batch");
    return SF_ERR_ARG;
  }
  if (n_steps <= 0 || (double)n_steps * b->n_envs >= 4294967296.0) {  // (no action array here: the outputs' 32-bit row offsets bound it)
    sf_set_error("sf_rollout_sampled: n_steps must be positive and n_steps * n_envs < 2^32 (got %d)", n_steps);
    return SF_ERR_ARG;
  }
  StepLaunch d{"sf_rollout_sampled", nullptr, SF_ACT_SAMPLED, n_steps, true, reward_dev, done_dev, info_dev};
  d.act_out = actions_out_dev;
  return launch_steps(b, d, obs_dev, stream);
}

extern "C" int sf_check_state(sf_batch* b, void* stream) {
  if (!b) return SF_ERR_ARG;
  DeviceGuard guard(b->device);
  unsigned long long two[2] = {0, 0};
  static_assert(SF_ACC_HANDOVER == SF_ACC_OVERFLOW + 1, "one copy for both");
  HIP_TRY(hipMemcpyAsync(two, b->d_acc.get() + SF_ACC_OVERFLOW, sizeof(two), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  const unsigned long long bad = two[0];
  if (two[1]) {  // (sticky for the batch's life: its state cannot be trusted)
    sf_set_error("%llu times a wave of a split step launch gave up waiting for its tile's other wave: the state of this batch is "
                 "not the reference's any more (an internal error: please report it with the batch size and the GPU)", two[1]);
    return SF_ERR_STATE;
  }
  if (bad) {  // sticky: the fields stay wrapped until new games start (sf_reset clears the count)
    sf_set_error("%llu times since the last sf_reset a per-episode counter or timer left its packed width (a batch without "
                 "auto-reset stepped for several episodes without sf_reset): stats / timers of those envs have wrapped", bad);
    return SF_ERR_STATE;
  }
  return SF_OK;
}

extern "C" int sf_set_event_output(sf_batch* b, uint32_t* events_dev) {
  if (!b) return SF_ERR_ARG;
  if (((uintptr_t)events_dev & 3) != 0) {
    sf_set_error("sf_set_event_output: the buffer must be 4-byte aligned");
    return SF_ERR_ARG;
  }
  b->args.events = events_dev;
  return SF_OK;
}

extern "C" int sf_set_final_obs_output(sf_batch* b, void* final_obs_dev) {
  if (!b) return SF_ERR_ARG;
  if (final_obs_dev != nullptr) {  // (switching it off is always possible)
    if (sfb_is_image(b)) {
      sf_set_error("sf_set_final_obs_output: image batches have no final-observation rows; their finished games' last frames "
                   "come from sf_set_final_frame_output (sfmi_final.h) -- or create the batch with SF_FLAG_NO_AUTO_RESET, read "
                   "the finished envs' frames and restart them with sf_reset_lanes");
      return SF_ERR_ARG;
    }
    if (!b->args.auto_reset) {
      sf_set_error("sf_set_final_obs_output: a SF_FLAG_NO_AUTO_RESET batch never replaces an observation: the row a finished "
                   "env's step wrote already is its last one (restart it with sf_reset_lanes)");
      return SF_ERR_ARG;
    }
    if (b->args.obs_type == SF_OBS_NONE || b->args.obs_dim <= 0) {
      sf_set_error("sf_set_final_obs_output: this batch has no observation rows");
      return SF_ERR_ARG;
    }
    if (((uintptr_t)final_obs_dev & 15) != 0) {
      sf_set_error("sf_set_final_obs_output: the buffer must be 16-byte aligned");
      return SF_ERR_ARG;
    }
  }
  b->args.final_obs = final_obs_dev;
  return SF_OK;
}

extern "C" int sf_check_actions(sf_batch* b, void* stream) {
  if (!b) return SF_ERR_ARG;
  DeviceGuard guard(b->device);
  unsigned long long bad = 0;
  HIP_TRY(hipMemcpyAsync(&bad, b->d_acc.get() + SF_EPISODE_STATS_LEN, sizeof(bad), hipMemcpyDeviceToHost,
                         (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  if (bad) {
    HIP_TRY(hipMemsetAsync(b->d_acc.get() + SF_EPISODE_STATS_LEN, 0, sizeof(bad), (hipStream_t)stream));
    sf_set_error("%llu action indices were outside [0, %d) and ran as NOOP", bad, b->act_count);
    return SF_ERR_ACTION;
  }
  return SF_OK;
}

extern "C" int sf_episode_stats(sf_batch* b, int64_t* out, int clear, void* stream) {
  if (!b || !out) return SF_ERR_ARG;
  DeviceGuard guard(b->device);
  // (all the words in one copy: the statistics, and behind them the sticky error counters -- a split launch whose hand-over
  //  timed out has played wrong games, and whoever reads statistics learns of it here without asking sf_check_state)
  unsigned long long all[SF_ACC_WORDS];
  HIP_TRY(hipMemcpyAsync(all, b->d_acc.get(), sizeof(all), hipMemcpyDeviceToHost, (hipStream_t)stream));
  HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
  memcpy(out, all, SF_EPISODE_STATS_LEN * sizeof(int64_t));  // (delivered either way)
  if (all[SF_ACC_HANDOVER]) {  // ... but NOT cleared: the window's statistics stay where they are for whoever looks into this
    sf_set_error("%llu times a wave of a split step launch gave up waiting for its tile's other wave: the state of this batch is "
                 "not the reference's any more (an internal error: please report it with the batch size and the GPU).  `out` holds "
                 "the statistics; nothing was cleared; the counter is sticky: make a new batch", all[SF_ACC_HANDOVER]);
    return SF_ERR_STATE;
  }
  if (clear)
    HIP_TRY(hipMemcpyAsync(b->d_acc.get(), kAccInit, SF_EPISODE_STATS_LEN * sizeof(int64_t), hipMemcpyHostToDevice,
                           (hipStream_t)stream));
  return SF_OK;
}
