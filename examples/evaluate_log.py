#!/usr/bin/env python3
"""The evaluator's per-episode line (rl/evaluate.py:82-99: episode reward, fortresses destroyed, shots -- last and running
average -- and the maximum reward) for a whole batch playing random actions, from the device's episode log: the loop never
looks at `done` or `reward`; every --every steps it drains the records that have finished since.

    python examples/evaluate_log.py --envs 64 --steps 6000
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spacefortress_amd import SFVecEnv  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--steps", type=int, default=6000)
    ap.add_argument("--every", type=int, default=1000, help="steps per fused launch and drain")
    ap.add_argument("--gametype", default="youturn")
    ap.add_argument("--seed", type=int, default=1)
    a = ap.parse_args()
    env = SFVecEnv(a.envs, gametype=a.gametype, spawn_stride=1)
    log = env.enable_episode_log()
    env.reset()
    env.seed_actions(a.seed)
    num_episodes = total_reward = total_fortress = total_shots = 0
    max_reward = 0
    for start in range(0, a.steps, a.every):
        env.rollout_sampled(min(a.every, a.steps - start), want_obs=False, want_actions=False)
        recs = log.drain()
        for env_id, ret, kills, shots in zip(recs["env"], recs["episode_return"], recs["kills"], recs["fire_actions"]):
            num_episodes += 1
            total_reward += int(ret)
            total_fortress += int(kills)
            total_shots += int(shots)
            max_reward = max(max_reward, int(ret))
            print("env %d  Episode Reward: |Last %d | Average %s || Fortress: |Last %d | Average %.3f || Shots: |Last %d | Average %.3f "
                  % (env_id, ret, total_reward / num_episodes, kills, total_fortress / num_episodes, shots, total_shots / num_episodes))
            print("Max Reward: ", max_reward)
        if recs["dropped"]:
            print("(%d records were overwritten before they were read: drain more often or raise capacity)" % recs["dropped"])
    print("%d episodes in %d steps of %d envs" % (num_episodes, a.steps, a.envs))
    env.close()


if __name__ == "__main__":
    main()
