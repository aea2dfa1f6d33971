#!/usr/bin/env python3
"""What a masked step costs:  python tools/step_where_probe.py [--rounds 8] [--only features|image] [--plain-only]

Variants, each a HIP graph of many calls on a batch of its own (fresh games, reused output buffers):
  S   sf_step (step_tensors), and S2, a second capture of it on another batch: |S - S2| is the spread a difference has to beat;
  W1  step_where with an all-ones mask: the step launch plus the hold launches, which return at once in every tile;
  WR  step_where with half the envs held, drawn at random lane by lane (every tile is mixed);
  WT  step_where with half the envs held by whole tiles (every other tile held whole).
The masks stay the same over the graph: the held half waits, the other half plays.  Two configurations: 65 536 envs with the
default features, 16 384 image envs with their frames.  One process; the graphs are replayed in alternating rounds (forwards,
then backwards); times are microseconds per call, the median over the rounds, from device events around a replay.
--plain-only times S and S2 alone: run it once per library (SFMI_LIB_PATH) to compare the plain step of two builds.
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


def make_graph(env, acts, mask):
    """-> a captured graph of len(acts) calls on `env`: step_tensors (mask None) or step_where(mask)"""
    dev = env.device
    out = env._alloc()
    ticks = torch.zeros(env.num_envs, dtype=torch.uint8, device=dev)

    def call(a):
        if mask is None:
            env.step_tensors(a, out=out)
        else:
            env.step_where(a, mask, out=out, ticks_out=ticks)

    env.reset()
    call(acts[0])  # (everything lazy -- the stash, render resources, the first launch's module load -- outside the capture)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            for a in acts:
                call(a)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    return g, out


def measure(name, n, obs_type, steps, rounds, plain_only):
    rng = np.random.default_rng(5)
    acts = torch.from_numpy(rng.integers(0, 5, (steps, n)).astype(np.uint8)).cuda()
    assert 1 + steps * (rounds + 1) < 5295, "the timed span would reach the first game over"
    ones = torch.ones(n, dtype=torch.uint8, device="cuda")
    rand = torch.from_numpy((rng.random(n) < 0.5).astype(np.uint8)).cuda()
    tiles = ((torch.arange(n, device="cuda") // 64) % 2).to(torch.uint8)
    masks = {"S": None, "S2": None} if plain_only else {"S": None, "W1": ones, "WR": rand, "WT": tiles, "S2": None}
    envs = {k: sfa.SFVecEnv(n, gametype="youturn", obs_type=obs_type, spawn_stride=1) for k in masks}
    graphs = {k: make_graph(envs[k], acts, m) for k, m in masks.items()}
    times = {k: [] for k in graphs}
    order = list(graphs)
    for r in range(rounds + 1):
        for k in (order if r % 2 else order[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graphs[k][0].replay()
            e1.record()
            torch.cuda.synchronize()
            if r > 0:  # (round 0 warms up)
                times[k].append(e0.elapsed_time(e1) * 1e3 / steps)
    for e in envs.values():
        e.check_state()
        e.close()
    med = {k: statistics.median(v) for k, v in times.items()}
    out = dict(config=name, envs=n, calls_per_graph=steps, rounds=rounds, lib=os.environ.get("SFMI_LIB_PATH", "this tree's"),
               us_per_call={k: round(v, 3) for k, v in med.items()}, ss_spread_us=round(abs(med["S"] - med["S2"]), 3),
               all_rounds_us={k: [round(x, 3) for x in v] for k, v in times.items()})
    if not plain_only:
        out["held_fraction"] = {"WR": round(1 - float(rand.float().mean()), 4), "WT": round(1 - float(tiles.float().mean()), 4)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--rounds", type=int, default=8)
    ap.add_argument("--only", choices=["features", "image"])
    ap.add_argument("--plain-only", action="store_true")
    a = ap.parse_args()
    if a.only != "image":
        print(json.dumps(measure("features-65536", 65536, "features", 64, a.rounds, a.plain_only)), flush=True)
    if a.only != "features":
        print(json.dumps(measure("image-16384", 16384, "image", 16, a.rounds, a.plain_only)), flush=True)


if __name__ == "__main__":
    main()
