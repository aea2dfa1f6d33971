/* sfmi_repeat.h -- action repeat (frame skip) on the device: K ticks per agent step in one launch.
 *
 * sfmi.h declares the ABI whose list of entry points is fixed per object; sf_step_repeat is declared here and exported by the
 * same library, libsfmi.so.
 *
 * sf_step_repeat: one agent step that plays the SAME action for up to `repeat` ticks (ALE's frameskip, gym's skip wrapper).  For
 *   every env, played alone, it is exactly
 *
 *       total, kill, ticks = 0, False, 0
 *       for j in range(repeat):
 *           obs, r, done, kill_j = env.step(a)        # SSF_Env.step, ENV:208-253
 *           total += r; kill |= kill_j; ticks += 1
 *           if done:
 *               final = obs; obs = env.reset(); break # the vec-env worker, rl/train.py:80
 *       return obs, total, done, kill, ticks
 *
 *   An env whose game ends at tick j < repeat - 1 of the window is parked until the next call, whatever the other envs of the
 *   batch do: it then holds a NEW game of which no tick has been played (prev_vlner carried over, exactly one entry of its spawn
 *   stream taken, counters zero, none of its missiles left in its tile's pool).  K calls of sf_step with the same actions cannot
 *   do that: they would play the new game on with the old action and add those ticks to the finished episode's reward.
 *
 *   actions_dev / act_type: as sf_step, one action per env.  An action outside the action set plays NOOP for the whole window and
 *   is reported by sf_check_actions (how many times it is counted is not specified).
 *   Outputs, each [n_envs] on the device, any of them may be NULL:
 *     obs_dev     the observation of the state the window leaves: the new game's first one for an env that finished
 *                 (SF_FLAG_REF_RESET_OBS applies to it).  Image batches: ONE frame per env, rendered from the draw records the
 *                 launch left -- one step launch and one frame launch, not `repeat` of each;
 *     reward_dev  int32: the sum of the played ticks' rewards;
 *     done_dev    uint8: 1 if the env's game ended inside the window;
 *     info_dev    uint8: the OR of the played ticks' fort_kill;
 *     ticks_dev   uint8: the ticks played, j + 1 for an env that finished at tick j, else `repeat`.
 *   The rest of the ABI sees the window as the ticks it played: sf_episode_stats accumulates a finished episode once, at its
 *   finishing tick; the row of sf_set_final_obs_output is written at the finishing tick with that tick's observation; the event
 *   word of sf_set_event_output is ONE uint32 per env, the OR of the played ticks' masks; the render-order hint is the OR over
 *   the window.  repeat == 1 is sf_step, bit for bit, in every output and every byte of state.
 *
 *   Plain stream work on `stream`: no allocation, no synchronise; capturable in a HIP graph.
 *   SF_ERR_ARG (with a text, nothing launched): a NULL batch or actions; an act_type other than 1, 4, 8; repeat outside
 *   [1, 255]; a SF_FLAG_NO_AUTO_RESET batch -- its finished env would have to be frozen in place for the rest of the window,
 *   which a parked lane is not (it is given its new game): step such a batch tick by tick. */
#ifndef SFMI_REPEAT_H
#define SFMI_REPEAT_H

#include "sfmi.h"

#ifdef __cplusplus
extern "C" {
#endif

int sf_step_repeat(sf_batch* b, const void* actions_dev, int act_type, int repeat, void* obs_dev, int32_t* reward_dev,
                   uint8_t* done_dev, uint8_t* info_dev, uint8_t* ticks_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SFMI_REPEAT_H */
