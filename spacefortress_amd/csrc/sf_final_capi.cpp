// sf_final_capi.cpp -- the C ABI of include/sfmi_final.h: the final-frame output of an image batch and the history of a final
// stack.  Host code only; the kernels are in sf_final_frames.hip (the frames, the shift) and sf_state_ops.hip (the finish).
// launch_steps (sf_capi.cpp) is the one caller of sfb_finish_with_final_frames.
#include <vector>

#include "sf_batch.h"
#include "sf_raster.h"

namespace {

size_t final_frame_bytes(const sf_batch* b) {
  return b->obs_mode == SF_OBS_IMAGE ? (size_t)SF_OUT * SF_OUT : (b->g_w ? (size_t)b->g_w * b->g_h : (size_t)SF_IMG_W * SF_IMG_H);
}

// sf_render's rules for the batch's mode and CURRENT geometry (sfb_render); stride: already resolved (0 -> the frame)
int check_frames(const sf_batch* b, const char* who, const uint8_t* frames, size_t stride) {
  const size_t frame = final_frame_bytes(b);
  const bool resized = b->obs_mode == SF_OBS_IMAGE;
  if (stride < frame) {
    sf_set_error("%s: env_stride %zu below the frame size %zu", who, stride, frame);
    return SF_ERR_ARG;
  }
  if (b->g_w) {
    if (resized && (((uintptr_t)frames | stride) & 3) != 0) {
      sf_set_error("%s: image frames of a non-default geometry must be 4-byte aligned and env_stride a multiple of 4", who);
      return SF_ERR_ARG;
    }
    return SF_OK;
  }
  if (((uintptr_t)frames & 15) != 0 || (stride & (resized ? 15 : 7)) != 0) {
    sf_set_error("%s: image frames must be 16-byte aligned and env_stride a multiple of %d", who, resized ? 16 : 8);
    return SF_ERR_ARG;
  }
  return SF_OK;
}

}  // namespace

extern "C" int sf_set_final_frame_output(sf_batch* b, uint8_t* frames_dev, size_t env_stride) {
  if (!b) {
    sf_set_error("sf_set_final_frame_output: null batch");
    return SF_ERR_ARG;
  }
  if (!frames_dev) {  // (switching it off is always possible)
    b->final_frames = nullptr;
    b->final_stride = 0;
    return SF_OK;
  }
  if (!sfb_is_image(b)) {
    sf_set_error("sf_set_final_frame_output: this batch has no image observations (rows: sf_set_final_obs_output)");
    return SF_ERR_ARG;
  }
  if (!b->args.auto_reset) {
    sf_set_error("sf_set_final_frame_output: a SF_FLAG_NO_AUTO_RESET batch never replaces a frame: the one a finished env's step "
                 "drew already is its last one (restart it with sf_reset_lanes)");
    return SF_ERR_ARG;
  }
  const size_t stride = env_stride ? env_stride : final_frame_bytes(b);
  SF_TRY(check_frames(b, "sf_set_final_frame_output", frames_dev, stride));
  DeviceGuard guard(b->device);
  if (!b->d_ftabs) {  // everything the path will ever need, once: no step with the output set allocates
    std::vector<uint8_t> bg(((size_t)SF_IMG_W * SF_IMG_H + 15) & ~(size_t)15, 0);
    SF_TRY(sf_image_background_geom(SF_IMG_W, SF_IMG_H, SF_VP_X, SF_VP_Y, 450.0, 460.0, SF_LINE_W, bg.data()));
    uint32_t tabs[16 * SF_OUT];
    SF_TRY(sf_area_tabs_geom(SF_IMG_W, SF_IMG_H, tabs));
    DevBuf<uint8_t> ndone, nbg;
    DevBuf<uint32_t> ntabs;
    HIP_TRY(ndone.alloc((size_t)b->n_envs));
    HIP_TRY(nbg.alloc(bg.size()));
    HIP_TRY(ntabs.alloc(16 * SF_OUT));
    HIP_TRY(hipMemset(ndone.get(), 0, (size_t)b->n_envs));
    HIP_TRY(hipMemcpy(nbg.get(), bg.data(), bg.size(), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(ntabs.get(), tabs, sizeof(tabs), hipMemcpyHostToDevice));
    b->d_fdone = std::move(ndone);
    b->d_fbg = std::move(nbg);
    b->d_ftabs = std::move(ntabs);
  }
  b->final_frames = frames_dev;
  b->final_stride = stride;
  return SF_OK;
}

// in front of the step launch: the geometry may have changed since the setter saw the buffer
int sfb_final_frames_fit(const sf_batch* b, const char* who) { return check_frames(b, who, b->final_frames, b->final_stride); }

int sfb_finish_with_final_frames(sf_batch* b, const uint8_t* done, hipStream_t stream) {
  const double* const trig = b->d_consts.get() + SF_LDS_TRIG;
  const int resize = b->obs_mode == SF_OBS_IMAGE ? 1 : 0;
  if (b->g_w)  // the general renderer's own launch arguments (sfb_render)
    HIP_TRY(sf_launch_final_frames(b->d_state.get(), done, b->n_envs, b->g_w, b->g_h, b->g_sx, b->g_sy, b->g_vx, b->g_vy, b->g_lw, trig,
                                   b->d_arcs.get(), b->d_gbg.get(), b->d_gtabs.get(), b->final_frames, b->final_stride, resize,
                                   b->d_glyphs.get(), stream));
  else  // the default geometry as sf_set_image_geometry would resolve it
    HIP_TRY(sf_launch_final_frames(b->d_state.get(), done, b->n_envs, SF_IMG_W, SF_IMG_H, (double)SF_IMG_W / 450.0, (double)SF_IMG_H / 460.0,
                                   SF_VP_X, SF_VP_Y, SF_LINE_W, trig, b->d_arcs.get(), b->d_fbg.get(), b->d_ftabs.get(), b->final_frames,
                                   b->final_stride, resize, b->d_glyphs.get(), stream));
  HIP_TRY(sf_launch_finish_lanes(b->args, done, stream));
  return SF_OK;
}

extern "C" int sf_final_stack_shift(const uint8_t* prev_stack_dev, uint8_t* final_stack_dev, int num_stack, size_t frame_bytes,
                                    const uint8_t* done_dev, int n_envs, void* stream) {
  if (!prev_stack_dev || !final_stack_dev || !done_dev || n_envs <= 0 || num_stack < 1 || num_stack > 16 || frame_bytes == 0 ||
      (frame_bytes & 15) != 0 || frame_bytes > ((size_t)1 << 24) || (((uintptr_t)prev_stack_dev | (uintptr_t)final_stack_dev) & 15) != 0) {
    sf_set_error("sf_final_stack_shift: need two 16-byte aligned stacks [n_envs][num_stack][frame_bytes], done bytes, n_envs > 0, "
                 "1 <= num_stack <= 16 and frame_bytes a multiple of 16 (at most 2^24)");
    return SF_ERR_ARG;
  }
  const uintptr_t p0 = (uintptr_t)prev_stack_dev, s0 = (uintptr_t)final_stack_dev;
  const size_t bytes = (size_t)n_envs * (size_t)num_stack * frame_bytes;
  if (p0 < s0 + bytes && s0 < p0 + bytes) {
    sf_set_error("sf_final_stack_shift: the previous stack and the final one overlap");
    return SF_ERR_ARG;
  }
  HIP_TRY(sf_launch_final_stack_shift(prev_stack_dev, final_stack_dev, num_stack, frame_bytes, done_dev, n_envs, (hipStream_t)stream));
  return SF_OK;
}
