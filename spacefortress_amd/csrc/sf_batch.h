// sf_batch.h -- what the host halves of the C ABI share (sf_capi.cpp, sf_image_capi.cpp, sf_state_capi.cpp, sf_norm_capi.cpp,
// sf_eplog_capi.cpp): the batch, the error macros, the device guard, the owner of a device allocation.  Host .cpp files only.
#pragma once
#include <stddef.h>

#include <utility>

#include "sf_internal.h"
#include "sf_view.h"

#define HIP_TRY(expr)                                                                  \
  do {                                                                                 \
    hipError_t e_ = (expr);                                                            \
    if (e_ != hipSuccess) {                                                            \
      sf_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
      return SF_ERR_HIP;                                                               \
    }                                                                                  \
  } while (0)

#define SF_TRY(expr) do { const int rc_ = (expr); if (rc_ != SF_OK) return rc_; } while (0) /* ... for a call that returns an SF_* code */

// keep the caller's (PyTorch's) current device untouched
struct DeviceGuard {
  int prev = -1;
  bool changed = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) == hipSuccess && prev != dev) changed = (hipSetDevice(dev) == hipSuccess);
  }
  ~DeviceGuard() {
    if (changed) (void)hipSetDevice(prev);
  }
};

// One hipMalloc allocation of `count` T, freed with its owner.  Move-only; whoever destroys it has the allocation's device
// current (DeviceGuard).
template <typename T>
class DevBuf {
  T* p_ = nullptr;

 public:
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p_ = o.p_;
      o.p_ = nullptr;
    }
    return *this;
  }
  ~DevBuf() { reset(); }
  T* get() const { return p_; }
  explicit operator bool() const { return p_ != nullptr; }
  hipError_t alloc(size_t count) {  // (whatever it held is freed first; empty after a failure)
    reset();
    const hipError_t e = hipMalloc((void**)&p_, count * sizeof(T));
    if (e != hipSuccess) p_ = nullptr;
    return e;
  }
  void reset() {
    if (p_) (void)hipFree(p_);
    p_ = nullptr;
  }
};

// sf_render_view: the device tables of one view (sf_view_host.cpp)
constexpr int kViewCache = 4;
struct ViewCache {
  SfViewRes res{};  // (its planes and format aside: the tables do not depend on them)
  DevBuf<uint8_t> d_bg;
  size_t bg_stride = 0;
  DevBuf<double> d_circle;
  DevBuf<SfGlyphAtlas> d_glyphs;
  unsigned long long used = 0;  // 0: an empty entry
};

struct sf_batch {
  SfKernelArgs args{};  // (raw pointers into the buffers below: what the kernels get, copied once per launch)
  sf_preset preset{};
  bool autoturn = false;
  int device = 0;
  int n_envs = 0;
  int act_count = 0;
  int spawn_skip = 0, spawn_stride = 0;
  DevBuf<unsigned char> d_state;
  size_t state_bytes = 0;
  DevBuf<double> d_consts;
  DevBuf<int16_t> d_spawn;
  DevBuf<unsigned long long> d_acc;
  DevBuf<unsigned long long> d_hint, d_dbg;  // args.hint (image batches), args.dbg (SF_STAMPS builds)
  DevBuf<unsigned char> d_scratch;  // linear staging for sf_get_field / sf_set_field (largest field)
  int obs_mode = 0;                 // the caller's SF_OBS_*; args.obs_type is SF_OBS_NONE for the image modes
  DevBuf<uint32_t> d_bg;            // image observation: static background, 92*90 bytes
  DevBuf<uint32_t> d_bg84;          // ... resampled to 84x84
  DevBuf<double> d_arcs;            // the explosion's arc constants (sf_arc_table), then nothing
  DevBuf<unsigned char> d_falpha;   // the live fortress's coverage at every whole-degree heading, 360 x 256 (sf_fort_alpha_table)
  DevBuf<uint32_t> d_tabs;          // INTER_AREA taps (sf_raster.h)
  DevBuf<unsigned char> d_xcache;   // explosion cache, SF_XC_BYTES per env; allocated by the first render
  // The missile fields as the reference has them (per env and slot), kept only while a caller looks at or edits them
  // through sf_get_field / sf_set_field: [SF_NSLOT][n_envs] (x, y) pairs and int32 headings.  The kernels keep a tile's
  // live missiles as one dense pool (sf_layout.h); `mslots_dirty` = the view was edited and the pools are rebuilt from it
  // (and from the alive masks) before the next launch that reads the state.
  DevBuf<unsigned char> d_ms_pos;
  DevBuf<int32_t> d_ms_ang;
  bool mslots_dirty = false;
  DevBuf<uint32_t> d_actrec;        // sf_step_sampled: one (tick, key0, key1, first lane) record per tile
  // The envs' draw records (sf_drawrec.h), SF_DR_BYTES per lane: what the frame kernel reads.  Image batches have them from
  // sf_create on and their step launches keep them current (args.draw); any other change of the state -- sf_reset,
  // sf_set_field, the missile view -- clears `draw_current`, and the next frame rebuilds them from the state first
  // (sf_drawrec_kernel).  Batches that step with a symbolic observation get the buffer with their first frame and rebuild
  // before every frame.
  DevBuf<unsigned char> d_draw;
  bool draw_current = false;
  // sf_set_image_geometry: a geometry other than the default one (sf_render_generic.hip); g_w == 0: the default
  int g_w = 0, g_h = 0;
  double g_sx = 0, g_sy = 0, g_vx = 0, g_vy = 0, g_lw = 0;  // scale_x = g_w / vp_w, scale_y = g_h / vp_h: NOT the caller's scale when vp_w * scale is not whole (SRC/draw.cpp:70-71)
  DevBuf<uint8_t> d_gbg;            // g_w * g_h bytes: the hexagons
  DevBuf<uint32_t> d_gtabs;         // the INTER_AREA taps g_w -> 84, g_h -> 84
  bool render_ready = false;        // the render caches and pictures exist (or were declined: SFMI_NO_EXPLOSION_CACHE)
  // the score text's glyph atlas of the CURRENT geometry (sf_glyphs.h; gw == 0: the seven-segment fallback), its device copy,
  // and the atlas the default geometry's static backgrounds and cached pictures were made with
  SfGlyphAtlas h_glyphs{}, baked_glyphs{};
  DevBuf<SfGlyphAtlas> d_glyphs;
  // sf_render_view: the device tables of the views drawn last (sf_view_host.cpp), kViewCache of them, least recently used
  // out first: a caller that alternates between a few views (a recorder's colour view and an agent's grey one) makes each once
  ViewCache views[kViewCache];
  unsigned long long view_clock = 0;
  // lane states (sfmi.h: sf_save_lanes ...): what the header of a row says of this batch, and the load's device bookkeeping --
  // lane -> k map (all -1 between calls), per tile a flag and the list of tiles a call touches, the list's length, the
  // refusal count (sf_check_lanes); sf_copy_lanes' scratch rows (lrows_cap of them, made by the first copy that needs them)
  uint32_t seed = 0;
  long spawn_len = 0;
  DevBuf<unsigned char> d_lanes;
  int* d_lmap = nullptr;  // (these five: views into d_lanes, not allocations of their own)
  unsigned *d_ltflag = nullptr, *d_ltlist = nullptr, *d_ltcount = nullptr;
  unsigned long long* d_lrefused = nullptr;
  DevBuf<unsigned char> d_lrows;
  long lrows_cap = 0;
  // sf_step_where (sfmi_hold.h): where the held envs wait while the others tick -- a buffer of the state's size, tile
  // layout, made by the first masked step
  DevBuf<unsigned char> d_hold;
  // sf_set_final_frame_output (sfmi_final.h): the caller's buffer (null: off) and its env stride in bytes; the done bytes of a
  // step the caller gave no done_dev; the default geometry's hexagons and INTER_AREA taps in the general renderer's table
  // forms (the painter draws the final frames in every geometry).  Made by the first setter call that switches the output on
  uint8_t* final_frames = nullptr;
  size_t final_stride = 0;
  DevBuf<uint8_t> d_fdone, d_fbg;
  DevBuf<uint32_t> d_ftabs;
};

inline bool sfb_is_image(const sf_batch* b) { return b->obs_mode == SF_OBS_IMAGE || b->obs_mode == SF_OBS_IMAGE_RAW; }

// sf_state_capi.cpp: rebuild the tiles' missile pools from the edited slot view, in stream order ahead of whatever reads the
// state next
int sfb_flush_missile_view(sf_batch* b, hipStream_t stream);
#define SF_FLUSH_VIEW(b, stream) SF_TRY(sfb_flush_missile_view((b), (hipStream_t)(stream)))

// sf_image_capi.cpp: the image observation's tables of a new batch (sf_create); what a batch needs to draw frames, made once;
// the envs' draw records from the state as it is; one frame per env, or one slot of a frame stack
// sf_final_capi.cpp: behind a step launch that ran with auto_reset off and wrote `done` -- the finished envs' frames into the
// final-frame output, then their episode totals, new games and draw records (sf_launch_finish_lanes); and, in front of that
// step launch, whether the output's buffer still fits the batch's geometry, which may have changed since the setter
int sfb_finish_with_final_frames(sf_batch* b, const uint8_t* done, hipStream_t stream);
int sfb_final_frames_fit(const sf_batch* b, const char* who);
int sfb_create_image_tables(sf_batch* b);
int sfb_ensure_render_resources(sf_batch* b, hipStream_t stream);
int sfb_rebuild_draw_records(sf_batch* b, hipStream_t stream);
int sfb_render(sf_batch* b, int mode, uint8_t* frames_dev, size_t env_stride, hipStream_t stream, const uint8_t* stack_done = nullptr,
               int stack_slot = 0, int stack_n = 1, const uint8_t* stack_prev = nullptr);
