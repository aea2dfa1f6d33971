/* sfmi_final.h -- final frames: the last frame of every game that ends, for image batches.
 *
 * sfmi.h declares the ABI whose list of entry points is fixed per object; the two calls below are declared here and exported
 * by the same library, libsfmi.so.  They are the image sibling of sf_set_final_obs_output (sfmi.h): every episode of this game
 * ends by the clock, every `done` is a truncation, and the return target at `done` bootstraps with the critic's value of the
 * finished game's last observation -- for an image batch, of its last frame (stack).
 *
 * sf_set_final_frame_output: once set on an auto-resetting image batch, every stepping call that plays single ticks --
 *   sf_step, sf_step_sampled, sf_step_record, sf_rollout, sf_rollout_sampled -- writes, for each env whose done flag it sets,
 *   the frame of that env's finished game after its last tick (what SSF_Env.step returned as game_state for that tick, before
 *   the new game replaced it) to frames_dev + env * env_stride, whether or not the call was given an obs_dev.  No other row is
 *   written, ever: a row whose env has not finished keeps the caller's bytes.  sf_reset and sf_reset_lanes never write it.
 *   The frame has the batch's own observation mode and geometry (84 x 84 for SF_OBS_IMAGE, the raw surface for
 *   SF_OBS_IMAGE_RAW, the current sf_set_image_geometry); alignment and stride rules are sf_render's for that mode and
 *   geometry.  env_stride 0: dense; a larger stride writes straight into the last slot of a [n][S][frame] stack.
 *
 *   Everything else is byte for byte what the same call does with the output off: every output row and the frames in obs_dev
 *   (at a finish the new game's first frame), every env's lane-state row as sf_save_lanes writes it, the event words,
 *   sf_episode_stats, the sampler's tick, the sf_step_record epilogue.  With the output NULL nothing anywhere changes: the
 *   launches are the ones they always were.
 *
 *   How: around the unchanged step launch.  The step runs with its auto-reset argument off, so finished envs keep
 *   their last state; one workgroup per FINISHED env paints its frame from that state with the general renderer's painter
 *   (the others return at once); a masked finish adds the finished envs' episode totals and starts their new games exactly as
 *   the in-kernel auto-reset does; their draw records follow; then the ordinary frames, if asked for.  With the output set
 *   sf_rollout / sf_rollout_sampled issue their ticks as single step launches (as they do when frames are asked for); an env
 *   that finishes twice in one call keeps its later frame.
 *
 *   Plain stream work: no host read, no synchronise, and nothing is allocated after the setter (it allocates what the path
 *   needs; sf_destroy frees it): a step with the output set can be captured in a HIP graph and replayed.
 *
 *   SF_ERR_ARG (with a text, the batch left as it was): a batch without image observations; a SF_FLAG_NO_AUTO_RESET batch;
 *   a misaligned buffer or a stride below the frame.  NULL always switches the output off.
 *   While the output is set, sf_step_repeat with repeat > 1 and sf_step_where return SF_ERR_ARG and launch nothing: a parked
 *   env's state is no longer its last frame's, and the held envs' stand-ins complicate the order.  Both are follow-ups.
 *
 * sf_final_stack_shift: the history of a final STACK.  For every env whose byte of done_dev is non-zero, slots 1 .. S-1 of
 *   prev_stack_dev[env] become slots 0 .. S-2 of final_stack_dev[env]; slot S-1 is not touched (the step wrote the final frame
 *   there through env_stride); the rows of envs with a zero byte are not touched at all.  Both stacks are
 *   [n_envs][num_stack][frame_bytes], 16-byte aligned, frame_bytes a multiple of 16 (at most 2^24), 1 <= num_stack <= 16
 *   (S = 1: nothing is copied), and the two byte ranges must not intersect; anything else is SF_ERR_ARG with nothing launched.  Plain device
 *   pointers, plain stream work: it can be captured. */
#ifndef SFMI_FINAL_H
#define SFMI_FINAL_H

#include "sfmi.h"

#ifdef __cplusplus
extern "C" {
#endif

int sf_set_final_frame_output(sf_batch* b, uint8_t* frames_dev, size_t env_stride);
int sf_final_stack_shift(const uint8_t* prev_stack_dev, uint8_t* final_stack_dev, int num_stack, size_t frame_bytes,
                         const uint8_t* done_dev, int n_envs, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SFMI_FINAL_H */
