#!/usr/bin/env python3
"""Measure what the episode log (SFVecEnv.enable_episode_log; csrc/sf_episode_log.hip) costs per step: `step_tensors` in the
features configuration with the log off and on, in one build, the two alternating inside one process.  profiles/episode_log.md
holds what this printed.

    python tools/episode_log_probe.py [--envs 4096 65536] [--steps 2000] [--rounds 5] [--root DIR] [--out DIR]

--root DIR imports the package from another tree (a build of the parent commit, which has no log: only "off" is measured
there) so that the same script gives the parent's figure and, from two runs of it, the noise.

Times are device events around whole windows of `steps` launches (eager: what a trainer's loop pays, host launch path
included) and around replays of a captured graph of 100 steps (the device's share alone), after a warm-up of the same shapes.
Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, nargs="+", default=[4096, 65536])
ap.add_argument("--steps", type=int, default=2000)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--label", default="this")
ap.add_argument("--out", default=None, help="directory for episode_log_probe_<label>.json")
ARGS = ap.parse_args()
sys.path.insert(0, os.path.abspath(ARGS.root))
import spacefortress_amd as sfa  # noqa: E402
from spacefortress_amd import _lib  # noqa: E402

GRAPH_STEPS = 100


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps  # ms


def probe(n, steps, rounds):
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(1)
    acts = torch.randint(0, 5, (64, n), device=dev, generator=g, dtype=torch.uint8)
    variants = ["off"] + (["on"] if hasattr(sfa.SFVecEnv, "enable_episode_log") else [])
    envs = {k: sfa.SFVecEnv(n, gametype="youturn", obs_type="features", spawn_stride=1, reuse_buffers=True) for k in variants}
    logs = {}
    if "on" in envs:
        logs["on"] = envs["on"].enable_episode_log()
    # games that end inside the window, staggered over it: the log's append path is part of what is timed
    for e in envs.values():
        e.set_field("time", (34 * (5295 - 50 - torch.arange(n) % max(1, steps - 100)).numpy()).astype("int32"))

    def run(k, count):
        e = envs[k]
        for t in range(count):
            e.step_tensors(acts[t & 63])

    for k in envs:
        run(k, 200)
    eager = {k: [] for k in envs}
    for _ in range(rounds):
        for k in envs:  # alternating
            eager[k].append(round(1e3 * timed(lambda: run(k, steps), 1) / steps, 3))
    graphs, graph = {}, {k: [] for k in envs}
    for k in envs:
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        graphs[k] = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graphs[k], stream=side):  # (one stream, no parallel branches)
                run(k, GRAPH_STEPS)
        torch.cuda.current_stream(dev).wait_stream(side)
        graphs[k].replay()
    for _ in range(rounds):
        for k in envs:
            graph[k].append(round(1e3 * timed(graphs[k].replay, 10) / GRAPH_STEPS, 3))
    del graphs
    res = {"n_envs": n, "steps": steps, "step_us_eager": eager, "step_us_graph": graph}
    if logs:
        res["episodes_logged"] = logs["on"].total
        res["episodes_counted"] = int(envs["on"].episode_stats()[0])
    for e in envs.values():
        e.close()
    return res


def main():
    assert torch.cuda.is_available(), "the probe measures on a GPU"
    all_res = {"label": ARGS.label, "build_id": _lib.lib().sf_build_id().decode(), "device": torch.cuda.get_device_name(0), "results": []}
    for n in ARGS.envs:
        r = probe(n, ARGS.steps, ARGS.rounds)
        all_res["results"].append(r)
        print(ARGS.label, json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    if ARGS.out:
        os.makedirs(ARGS.out, exist_ok=True)
        with open(os.path.join(ARGS.out, "episode_log_probe_%s.json" % ARGS.label), "w") as f:
            json.dump(all_res, f, indent=1)


if __name__ == "__main__":
    main()
