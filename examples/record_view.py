#!/usr/bin/env python3
"""Record what an agent sees a person would see: N envs play on the device (here sampled actions, `step_sampled`; a policy
goes in the same place), and lane k's frames in the human-play front-end's view -- 450 x 460 colour, Game(config,
viewport=(130, 80, 450, 460), lw=2, grayscale=False) -- are kept and saved as one uint8 [T, 460, 450, 3] RGB .npy, what a
video encoder takes (no ffmpeg needed here).

    python examples/record_view.py --envs 256 --steps 600 --lane 3 --out lane3.npy
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
    ap.add_argument("--gametype", default="youturn")
    ap.add_argument("--envs", type=int, default=256)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--lane", type=int, default=0)
    ap.add_argument("--every", type=int, default=1, help="keep every n-th step's frame")
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default="view.npy")
    a = ap.parse_args()
    env = SFVecEnv(a.envs, gametype=a.gametype, obs_type="features")
    env.reset()
    env.seed_actions(a.seed)
    n = (a.steps + a.every - 1) // a.every
    frames = torch.empty((n, 460, 450, 3), dtype=torch.uint8, device=env.device)  # (2.4 GB for 4 000 frames: keep --steps modest)
    for t in range(a.steps):
        env.step_sampled()
        if t % a.every == 0:
            env.render_view(viewport=(130, 80, 450, 460), lw=2.0, grayscale=False, format="rgb", lanes=a.lane, out=frames[t // a.every:t // a.every + 1])
    np.save(a.out, frames.cpu().numpy())
    env.close()
    print("%s: %d frames of lane %d, %s" % (a.out, n, a.lane, tuple(frames.shape[1:])))


if __name__ == "__main__":
    main()
