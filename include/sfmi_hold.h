/* sfmi_hold.h -- the masked step: chosen envs of a batch tick, the others hold in place.
 *
 * sfmi.h declares the ABI whose list of entry points is fixed per object; sf_step_where is declared here and exported by the
 * same library, libsfmi.so.  It is the stepping sibling of sf_reset_lanes (sfmi.h): EnvPool's send(env_id) / recv on a subset,
 * a per-env pause, exactly k episodes per env.
 *
 * sf_step_where: one agent step of the envs the mask marks.  active_dev: uint8 [n_envs] on the batch's device, any non-zero
 *   byte marks its env ACTIVE (sf_reset_lanes' convention); no byte at or beyond n_envs is read.  actions_dev / act_type /
 *   repeat and the five outputs are sf_step_repeat's (sfmi_repeat.h); every output may be NULL.
 *
 *   An ACTIVE env: every output, every byte of its state and every batch-level effect -- the episode accumulators
 *   (sf_episode_stats), its row of the sf_set_final_obs_output buffer, its event word, its render-hint bit, the bad-action
 *   count -- are exactly what sf_step_repeat(b, actions, act_type, repeat, ...) gives that env, parking and the new game
 *   inside a window included; repeat == 1 is sf_step.  It does not matter which other envs are held.
 *
 *   A HELD env, whatever its action:
 *     - its lane-state row as sf_save_lanes writes it is unchanged byte for byte (scalar fields, packed counters, the spawn
 *       cursor, prev_vlner, shells, missiles by slot);
 *     - reward_dev 0, done_dev 0, info_dev 0, ticks_dev 0, event word 0;
 *     - its row of obs_dev is the observation of its state as sf_load_lanes(obs) writes it: integer columns exact, the
 *       bearings inside the bounds of DESIGN 9, SF_FLAG_REF_RESET_OBS applied to a game of which no tick has been played;
 *       an image batch's frame is the frame of its unchanged state;
 *     - its row of the sf_set_final_obs_output buffer is untouched; it adds nothing to sf_episode_stats, does not count
 *       towards sf_check_state's overflow count, and its render-hint bit is clear;
 *     - an out-of-range action of a held env may or may not be counted by sf_check_actions: pass valid ids (or 0) there.
 *
 *   SF_FLAG_NO_AUTO_RESET batches are accepted with repeat == 1: a finished env that is held stays at its game over with
 *   every counter as it was, however long the others play on (hold the finished envs and sf_check_state stays clean).
 *
 *   How: the tick is straight-line code over a missile pool that the 64 envs of a tile share, so a held env cannot sit a
 *   launch out.  Around the unchanged step launch two small launches swap it for a game in which nothing can happen -- ship
 *   dead and not due back, no projectiles, time 0, counters zero: the state a repeat window parks a finished env in -- and
 *   back.  A tile without a held env is not touched by either; an all-ones mask costs those two launches, which
 *   return at once, a third that sets ticks_dev to 1 when repeat == 1 (not with ticks_dev NULL) and, image batches, a fourth
 *   for the held envs' draw records.  The feature is capability and exactness, not speed: a held env moves 3.6 KB per call
 *   (3.1 KB by the two hold launches, 464 B by the step launch that ticks its stand-in), a stepped one 464 B.
 *   If the step launch itself fails (SF_ERR_HIP), the held envs are still put back before the call returns.
 *
 *   Plain stream work on `stream`: the host never reads the mask and never synchronises.  The FIRST call on a batch allocates
 *   the batch-owned stash (the size of the state; sf_destroy frees it); from the second call on nothing is allocated and the
 *   call can be captured in a HIP graph.
 *   SF_ERR_ARG (with a text, nothing launched): a NULL batch, mask or actions; an act_type other than 1, 4, 8 (no sampled
 *   actions); repeat outside [1, 255]; repeat > 1 on a SF_FLAG_NO_AUTO_RESET batch (as sf_step_repeat). */
#ifndef SFMI_HOLD_H
#define SFMI_HOLD_H

#include "sfmi.h"

#ifdef __cplusplus
extern "C" {
#endif

int sf_step_where(sf_batch* b, const uint8_t* active_dev, const void* actions_dev, int act_type, int repeat, void* obs_dev,
                  int32_t* reward_dev, uint8_t* done_dev, uint8_t* info_dev, uint8_t* ticks_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SFMI_HOLD_H */
