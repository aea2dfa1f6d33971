#!/usr/bin/env python3
"""Exactly k episodes per lane on a batch WITHOUT auto-reset, with the lanes that are through HELD: the loop steps only the
lanes still playing (SFVecEnv.step_where, sfmi_hold.h: sf_step_where), starts a new game in a lane whose episode ended and that
has more to play (reset_lanes), and leaves a lane that has finished its k-th episode at its game over -- not a tick more, so
its counters stay inside their packed widths and check_state() is clean however long the slowest lane takes.  Held lanes read
reward 0 / done 0, so nothing has to be filtered.  (examples/one_episode_per_lane.py is the same loop without the hold: it ticks
the finished lanes on and masks their rewards in torch.)  Nothing but the final tallies leaves the device.

    python examples/hold_finished_lanes.py --envs 256 --episodes 2
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spacefortress_amd import SFVecEnv  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--episodes", type=int, default=1, help="k: episodes per lane")
    ap.add_argument("--stagger", type=int, default=500, help="lanes start up to this many ticks into their first game")
    ap.add_argument("--gametype", default="youturn")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    n, k = a.envs, a.episodes
    env = SFVecEnv(n, gametype=a.gametype, spawn_stride=1, auto_reset=False, reuse_buffers=True)
    obs = env.reset()
    rng = np.random.default_rng(a.seed)
    env.set_field("time", (env.tickdur * rng.integers(0, a.stagger + 1, n)).astype(np.int32))
    gen = torch.Generator(device=env.device).manual_seed(a.seed)
    finished = torch.zeros(n, dtype=torch.int64, device=env.device)
    returns = torch.zeros(n, dtype=torch.int64, device=env.device)
    ticks = torch.zeros(n, dtype=torch.int64, device=env.device)
    steps = 0
    while True:
        act = torch.randint(0, env.n_actions, (n,), device=env.device, dtype=torch.uint8, generator=gen)
        running = finished < k
        obs, rew, done, info = env.step_where(act, running)  # (a held lane: reward 0, done 0)
        returns += rew.long()
        ticks += env.last_ticks.long()
        finished += (done != 0).long()
        env.reset_lanes(mask=(done != 0) & (finished < k), out=obs)  # the reset lanes' rows of `obs` are their new games'
        steps += 1
        if steps % 256 == 0 and bool((finished >= k).all()):  # (the only host read of the loop)
            break
    r, t = returns.cpu().numpy(), ticks.cpu().numpy()
    print("%d lanes x %d episodes in %d calls (%d to %d ticks per lane): return per lane mean %.1f, min %d, max %d"
          % (n, k, steps, t.min(), t.max(), r.mean(), r.min(), r.max()))
    env.check_state()
    env.close()


if __name__ == "__main__":
    main()
