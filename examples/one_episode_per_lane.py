#!/usr/bin/env python3
"""Exactly k episodes per lane, on a batch WITHOUT auto-reset: the loop steps, masks `done`, and starts new games in just those
lanes with the masked reset (SFVecEnv.reset_lanes, sfmi.h: sf_reset_lanes) until every lane has finished its k-th episode.  A
lane that is through keeps its last game over and is not reset again.  The lanes start at different game times (--stagger), so
they finish at different steps; nothing but the final tallies leaves the device.

    python examples/one_episode_per_lane.py --envs 256 --episodes 2
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
    steps = 0
    while True:
        act = torch.randint(0, env.n_actions, (n,), device=env.device, dtype=torch.uint8, generator=gen)
        obs, rew, done, info = env.step_tensors(act)
        running = finished < k
        ended = (done != 0) & running
        returns += torch.where(running, rew.long(), torch.zeros_like(returns))
        finished += ended.long()
        env.reset_lanes(mask=ended & (finished < k), out=obs)  # the reset lanes' rows of `obs` are their new games'
        steps += 1
        if steps % 256 == 0 and bool((finished >= k).all()):  # (the only host read of the loop)
            break
    r = returns.cpu().numpy()
    print("%d lanes x %d episodes in %d steps: return per lane mean %.1f, min %d, max %d"
          % (n, k, steps, r.mean(), r.min(), r.max()))
    env.check_state()
    env.close()


if __name__ == "__main__":
    main()
