// sf_internal.h -- declarations shared between the kernels, the host tables and the C ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sf_glyphs.h"
#include "sf_layout.h"
#include "sfmi.h"
#include "sfmi_final.h"
#include "sfmi_hold.h"
#include "sfmi_masked.h"
#include "sfmi_repeat.h"

// sf_kernels.hip: the hot path
hipError_t sf_launch_reset(const SfKernelArgs& a, int first, unsigned cursor0, unsigned stride, void* obs,
                           hipStream_t stream);
hipError_t sf_launch_step(const SfKernelArgs& a, bool autoturn, bool shaped, const void* actions, int act_type, void* obs,
                          int32_t* reward, uint8_t* done, uint8_t* info, int n_steps, bool fused, hipStream_t stream);
// `repeat` ticks of one action per env, one row of outputs (sfmi_repeat.h: sf_step_repeat); ticks: uint8 [n_envs] or null
hipError_t sf_launch_step_repeat(const SfKernelArgs& a, bool autoturn, bool shaped, const void* actions, int act_type, void* obs,
                                 int32_t* reward, uint8_t* done, uint8_t* info, uint8_t* ticks, int repeat, hipStream_t stream);

// sf_state_ops.hip: the state tools
// env.reset() in the envs whose byte of mask [n_envs] is not zero (sfmi.h: sf_reset_lanes); obs may be null
hipError_t sf_launch_reset_lanes(const SfKernelArgs& a, const uint8_t* mask, void* obs, hipStream_t stream);
// the envs' draw records (sf_drawrec.h) from the state as it is: a.draw / a.draw_pics say where and for which pictures
hipError_t sf_launch_drawrec(const SfKernelArgs& a, hipStream_t stream);
// sf_step_where (sfmi_hold.h): around a step launch, the envs whose byte of active [n_envs] is zero are swapped for a game in
// which nothing can happen and back.  stash: a buffer of the state's size.  End: the held envs' output rows (each may be
// null; a.events and a.hint as the batch has them) and, where a.draw is set, their draw records from the restored state.
// one_tick: the launch in between was a plain step, which writes no ticks: every active env's are 1
hipError_t sf_launch_hold_begin(const SfKernelArgs& a, const uint8_t* active, unsigned char* stash, hipStream_t stream);
hipError_t sf_launch_hold_end(const SfKernelArgs& a, const uint8_t* active, const unsigned char* stash, void* obs, int32_t* reward,
                              uint8_t* done, uint8_t* info, uint8_t* ticks, int one_tick, hipStream_t stream);

// final frames (sfmi_final.h), behind a step launch that ran with auto_reset off: the envs whose byte of done [n_envs] is not
// zero finish as the in-kernel auto-reset finishes them -- episode totals into a.acc, a new game on the lane's own prev_vlner
// and spawn cursor, their missiles out of the tile's pool, their hint bits cleared -- and, where a.draw is set, their draw
// records follow the new state (the others' are the step launch's own and stay)
hipError_t sf_launch_finish_lanes(const SfKernelArgs& a, const uint8_t* done, hipStream_t stream);

// sf_final_frames.hip: sf_launch_render_generic (below) for the envs whose byte of done [n_envs] is not zero -- one workgroup
// per env, which returns at once on a zero byte; no row of `out` but a finished env's is written
hipError_t sf_launch_final_frames(const unsigned char* state, const uint8_t* done, int n_envs, int W, int H, double sx, double sy,
                                  double vp_x, double vp_y, double line_w, const double* trig, const double* arcs, const uint8_t* bg,
                                  const uint32_t* tabs, uint8_t* out, size_t out_stride, int resize, const SfGlyphAtlas* glyphs,
                                  hipStream_t stream);
hipError_t sf_launch_final_stack_shift(const uint8_t* prev, uint8_t* fin, int num_stack, size_t frame_bytes, const uint8_t* done,
                                       int n_envs, hipStream_t stream);

// gather (to_linear) / scatter one field between the tiled state and a linear [count][n_envs] buffer
hipError_t sf_launch_field_copy(unsigned char* state, int n_envs, int field, unsigned char* linear, int to_linear,
                                hipStream_t stream);

// the missile fields as the reference has them, [SF_NSLOT][n_envs] slot-major ((x, y) pairs and int32 headings), from /
// to the tiles' pools; and one component of that view from / to a linear buffer (which: 0 x, 1 y, 2 heading as int16)
hipError_t sf_launch_mpool_to_slots(const unsigned char* state, int n_envs, void* sl_pos, int32_t* sl_ang, hipStream_t stream);
hipError_t sf_launch_slots_to_mpool(unsigned char* state, long lanes, int n_envs, const void* sl_pos, const int32_t* sl_ang,
                                    hipStream_t stream);
hipError_t sf_launch_mslot_component(void* sl_pos, int32_t* sl_ang, long total, int which, void* linear, int to_linear,
                                     hipStream_t stream);

// lane states (sfmi.h: sf_save_lanes / sf_load_lanes): rows of SF_LANE_STATE_BYTES <-> lanes.  idx64: the index arrays are int64
// (else int32).  Load: map = [lanes] int32 all -1, tflag = [lanes / 64] all 0, tlist = [lanes / 64], tcount = one word -- the
// launches leave map and tflag as they found them; refused counts the rejected (lane, row) pairs
hipError_t sf_launch_lanes_save(const unsigned char* state, int n_envs, const void* lanes, int idx64, int n, unsigned char* rows,
                                const uint32_t header[4], unsigned long long* refused, hipStream_t stream);
hipError_t sf_launch_lanes_load(const SfKernelArgs& a, const void* lanes, int idx64, int n, const unsigned char* rows, const void* row_idx,
                                long n_rows, const uint32_t header[4], int* map, unsigned* tflag, unsigned* tlist, unsigned* tcount,
                                unsigned long long* refused, void* obs, hipStream_t stream);

hipError_t sf_launch_group_copy(const unsigned char* state, int n_envs, int group, unsigned char* linear,
                                hipStream_t stream);

// sf_render.hip: one wave per env; bg = 92*90 bytes, bg84 = its 84*84 INTER_AREA image, tabs = SF_TAB_WORDS
hipError_t sf_launch_render(const unsigned char* state, const unsigned char* draw, int n_envs, const uint32_t* bg, const uint32_t* bg84,
                            const uint32_t* tabs, uint8_t* out, size_t out_stride, unsigned char* xcache,
                            const unsigned char* fpatch, int resize, const uint8_t* stack_done, int stack_slot, int stack_n,
                            const uint8_t* stack_prev, const unsigned long long* hint, const unsigned char* hud,
                            const double* trig, const double* arcs, const unsigned char* falpha, const SfGlyphAtlas* glyphs,
                            hipStream_t stream);
// the score / bar pictures (SF_HUD_BYTES, sf_raster.h)
hipError_t sf_launch_hud_pictures(const uint32_t* bg, const uint32_t* bg84, const uint32_t* tabs, unsigned char* hud,
                                  const SfGlyphAtlas* glyphs, hipStream_t stream);
// sf_image.cpp: the live fortress's coverage over its 16 x 16 box at heading 0..359; all 360 of them (nullptr: see sf_last_error)
int sf_fort_alpha_heading(int heading, uint8_t* out256);
const uint8_t* sf_fort_alpha_table();
// ... and the 36 x 4 backgrounds with the fortress in them, behind the four plain ones (SF_BG_COUNT, sf_raster.h)
hipError_t sf_launch_fort_patches(uint32_t* bg, uint32_t* bg84, const uint32_t* tabs, unsigned char* fpatch, const double* arcs,
                                  const unsigned char* falpha, hipStream_t stream);

// sf_normalize.hip: reduce + apply (two launches); partials = SF_NORM_GROUPS x 2 (dim + 1) doubles; stats is the
// buffer of this step's parity, stats_next the other parity's
#define SF_NORM_GROUPS 256
hipError_t sf_launch_normalize(const void* obs, void* obs_out, int obs_f64, const int32_t* rew, float* rew_out, double* ret,
                               int n, int dim, double gamma, double eps, double clipob, double cliprew, int do_ob,
                               int do_ret, double* partials, const double* stats, double* stats_next,
                               hipStream_t stream);

// sf_render_generic.hip: the image observation in any geometry (sf_set_image_geometry): one workgroup per env, the W x H
// surface in dynamic LDS, bg = W * H bytes (the hexagons), tabs = the INTER_AREA taps (8 words per destination column, then
// per row: first, count, 4 weights, 2 pad)
hipError_t sf_launch_render_generic(const unsigned char* state, int n_envs, int W, int H, double sx, double sy, double vp_x, double vp_y,
                                    double line_w, const double* trig, const double* arcs, const uint8_t* bg, const uint32_t* tabs,
                                    uint8_t* out, size_t out_stride, int resize, const SfGlyphAtlas* glyphs, hipStream_t stream);
hipError_t sf_launch_stack_clear(uint8_t* stack, size_t bytes_per_env, const uint8_t* done, int n, hipStream_t stream);

hipError_t sf_launch_normalize_after_step(const void* obs, void* obs_out, int obs_f64, const int32_t* rew, float* rew_out, int n,
                                          int dim, double eps, double clipob, double cliprew, int do_ob, int do_ret,
                                          const double* partials, int rows, const double* stats, double* stats_next,
                                          hipStream_t stream);
// sf_capi.cpp: sf_step with the VecNormalize reduction riding on it (partials: [2 (obs_dim + 1)][lanes / 64])
int sf_step_with_norm_partials(sf_batch* b, const void* actions_dev, int act_type, void* obs_dev, int32_t* reward_dev,
                               uint8_t* done_dev, uint8_t* info_dev, double* partials, double* ret, double gamma, int* rows_out,
                               void* stream);

// sf_episode_log.hip: the episode log (sfmi.h: sf_eplog_*).  One update = count, scan, apply over groups of SF_EPLOG_ROWS
// rows; counts / offs hold SF_EPLOG_ROWS * ceil(n / 256) cells each
#define SF_EPLOG_ROWS 32
struct SfEplogHeader {
  unsigned long long total, rows_seen;  // episodes ever logged, rows ever consumed
  unsigned long long base_seq, base_row;  // total / rows_seen in front of the group of rows in flight (scan -> apply)
};
struct SfEplogArgs {
  int n, fire_action, bins;
  long long hist_lo;
  unsigned long long capacity;
  int4* acc;  // per env: return, length, kills, fire actions
  sf_episode_record* ring;
  unsigned long long* hist;
  SfEplogHeader* hdr;
  uint32_t *counts, *offs;
};
hipError_t sf_launch_eplog_update(const SfEplogArgs& a, const int32_t* rew, const uint8_t* done, const uint8_t* info,
                                  const void* actions, int act_type, int K, hipStream_t stream);
// zero the four running accumulators of the envs whose byte of mask [n] is not zero
hipError_t sf_launch_eplog_restart_where(const SfEplogArgs& a, const uint8_t* mask, hipStream_t stream);

// sf_host.cpp (no HIP calls: usable and tested without a GPU)
void sf_host_fill_consts(const sf_preset& p, double* consts /* SF_CONST_DOUBLES */);
// does the preset, with sf_host_fill_consts' block of it, agree with the constants compiled into the kernels (sfc::, the hexagons)?
bool sf_preset_compiled_in(const sf_preset& p, const double* consts);
// sf_set_field's range checks of `host` = field [count][n_envs]: the packed bit fields, the 13 statistics and their sum rule,
// the missile headings; SF_OK, or SF_ERR_ARG with the env (and slot) in the error text
int sf_field_values_fit(int field, const void* host, long n_envs);
void sf_set_error(const char* fmt, ...);
// sf_image.cpp: the INTER_AREA taps in the two device layouts -- the default geometry's (SF_TAB_WORDS words, sf_raster.h;
// refused unless they have the structure the frame kernel assumes) and a w x h surface's (16 * SF_OUT words, range-checked)
int sf_area_tabs_default(uint32_t* tabs);
int sf_area_tabs_geom(int w, int h, uint32_t* tabs);
// sf_image.cpp: the score text's glyph atlas (sf_glyphs.h) -- the built-in one, a caller's, and the static background with
// the score 0000000 of a given atlas baked in
void sf_glyphs_default(SfGlyphAtlas* G);
int sf_glyphs_pack(const sf_score_glyphs* layout, const uint8_t* alpha, const int* box, SfGlyphAtlas* G);
int sf_image_static_glyphs(int variant, const SfGlyphAtlas* G, uint8_t* out);
