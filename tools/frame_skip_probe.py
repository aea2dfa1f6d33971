#!/usr/bin/env python3
"""What an agent step with action repeat costs:  python tools/frame_skip_probe.py [--repeat 4] [--rounds 8] [--only features|image]

A = `repeat` sf_step launches per agent step with the same action tensor (all a trainer had before sf_step_repeat; it is also
wrong when an env finishes inside the window, which a fresh batch never does in the timed span), B = one sf_step_repeat.
Two configurations: 65 536 envs with the default features, and 16 384 image envs with their frames (A: repeat x (step + frame),
B: the repeat launch + one frame).  One process; every variant is a HIP graph of many agent steps on a batch of its own, replayed
in alternating rounds (A, B, A' then A', B, A); A' is a second capture of A on a third batch, and |A - A'| is the spread the
difference A - B has to beat.  Times are microseconds per AGENT step, the median over the rounds, from events around a replay.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import spacefortress_amd as sfa


def make_graph(env, acts, repeat, fused):
    """-> a captured graph of len(acts) agent steps on `env` (fresh games, reused output buffers)"""
    dev = env.device
    out = env._alloc()
    ticks = torch.zeros(env.num_envs, dtype=torch.uint8, device=dev)

    def agent_step(a):
        if fused:
            env.step_repeat(a, repeat, out=out, ticks_out=ticks)
        else:
            for _ in range(repeat):
                env.step_tensors(a, out=out)

    env.reset()
    agent_step(acts[0])  # (everything lazy -- render resources, the first launch's module load -- outside the capture)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            for a in acts:
                agent_step(a)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    return g, out


def measure(name, n, obs_type, steps, repeat, rounds):
    rng = np.random.default_rng(5)
    n_act = 5
    acts = torch.from_numpy(rng.integers(0, n_act, (steps, n)).astype(np.uint8)).cuda()
    # an episode is 5 295 ticks: the warm-up step, the warm-up replay and the timed rounds stay inside the first one
    assert repeat * (1 + steps * (rounds + 1)) < 5295, "the timed span would reach the first game over"
    envs = [sfa.SFVecEnv(n, gametype="youturn", obs_type=obs_type, spawn_stride=1) for _ in range(3)]
    graphs = {"A": make_graph(envs[0], acts, repeat, False), "B": make_graph(envs[1], acts, repeat, True),
              "A2": make_graph(envs[2], acts, repeat, False)}
    times = {k: [] for k in graphs}
    for r in range(rounds + 1):
        for k in (("A", "B", "A2") if r % 2 else ("A2", "B", "A")):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graphs[k][0].replay()
            e1.record()
            torch.cuda.synchronize()
            if r > 0:  # (round 0 warms up)
                times[k].append(e0.elapsed_time(e1) * 1e3 / steps)
    done = [int(graphs[k][1][2].sum()) for k in graphs]
    assert not any(done), "an env finished inside the timed span"
    for e in envs:
        e.check_state()
        e.close()
    med = {k: statistics.median(v) for k, v in times.items()}
    return dict(config=name, envs=n, repeat=repeat, agent_steps_per_graph=steps, rounds=rounds,
                us_per_agent_step_A=round(med["A"], 3), us_per_agent_step_A2=round(med["A2"], 3), us_per_agent_step_B=round(med["B"], 3),
                aa_spread_us=round(abs(med["A"] - med["A2"]), 3), a_minus_b_us=round(min(med["A"], med["A2"]) - med["B"], 3),
                ticks_per_second_A=round(n * repeat / min(med["A"], med["A2"]) * 1e6), ticks_per_second_B=round(n * repeat / med["B"] * 1e6),
                all_rounds_us={k: [round(x, 3) for x in v] for k, v in times.items()})


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--repeat", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--only", choices=["features", "image"])
    a = ap.parse_args()
    if a.only != "image":
        print(json.dumps(measure("features-65536", 65536, "features", 64, a.repeat, a.rounds)), flush=True)
    if a.only != "features":
        print(json.dumps(measure("image-16384", 16384, "image", 16, a.repeat, a.rounds)), flush=True)


if __name__ == "__main__":
    main()
