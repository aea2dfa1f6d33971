/* sfmi_masked.h -- companions of sf_reset_lanes (sfmi.h) for the objects that follow a batch from outside.
 *
 * sfmi.h declares the ABI whose list of entry points is fixed per object (batch, normaliser, episode log, ...); the masked
 * forms that only make sense beside sf_reset_lanes are declared here and exported by the same library, libsfmi.so.
 *
 * sf_eplog_restart_where: the masked form of sf_eplog_restart (sfmi.h, "episode log").  mask_dev: uint8 [n_envs] on the
 *   log's device, any non-zero byte marks its env -- the mask sf_reset_lanes took (env.reset() in those envs, ENV:163-178).
 *   It zeroes the four running accumulators (return, length, kills, fire actions) of the masked envs ONLY: an abandoned
 *   game leaves no record.  It emits no record, touches no histogram bin, neither total nor rows_seen, and no other env's
 *   accumulators.  Plain stream work on `stream`: no allocation, no host read of the mask, no synchronise; capturable in a
 *   HIP graph.  SF_ERR_ARG (with a text): a NULL log or mask_dev. */
#ifndef SFMI_MASKED_H
#define SFMI_MASKED_H

#include "sfmi.h"

#ifdef __cplusplus
extern "C" {
#endif

int sf_eplog_restart_where(sf_eplog* h, const uint8_t* mask_dev, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SFMI_MASKED_H */
