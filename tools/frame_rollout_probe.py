#!/usr/bin/env python3
"""Measure the deduplicated image rollout storage (FrameRollout) against the stacked one (DeviceRollout, num_stack=4) in the
same build: per-step time of a whole rollout, and the minibatch gather, for both store layouts.  profiles/frame_rollout.md
holds what this printed.

    python tools/frame_rollout_probe.py [--envs 4096 16384] [--steps 128] [--out DIR]

Times are device events around whole windows (a rollout of T steps; `reps` gathers), after a warm-up of the same shapes, the
variants alternating inside one process.  Bytes are counted from shapes: a gathered stack is 28 224 bytes read and 28 224
(uint8) or 112 896 (float32) written.  Needs a GPU; there is no fallback."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import spacefortress_amd as sfa  # noqa: E402
from spacefortress_amd import _lib  # noqa: E402

S, STACK = 4, 4 * 84 * 84


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps  # ms


def rollout(ro, acts):
    for t in range(acts.shape[0]):
        ro.step(t, acts[t])


def probe(n, T, rounds):
    dev = torch.device("cuda")
    res = {"n_envs": n, "T": T, "num_stack": S}
    g = torch.Generator(device=dev).manual_seed(1)
    acts = torch.randint(0, 3, (T, n), device=dev, generator=g, dtype=torch.uint8)
    make = {"stacked": lambda e: sfa.DeviceRollout(e, T, num_stack=S),
            "frames_time": lambda e: sfa.FrameRollout(e, T, num_stack=S, layout="time"),
            "frames_env": lambda e: sfa.FrameRollout(e, T, num_stack=S, layout="env")}
    envs = {k: sfa.SFVecEnv(n, gametype="autoturn", obs_type="image", spawn_stride=1) for k in make}
    ros = {k: make[k](envs[k]) for k in make}
    res["nbytes"] = {k: ros[k].nbytes() for k in ros}
    for k in ros:  # warm-up: one whole rollout each
        ros[k].reset()
        rollout(ros[k], acts)
        ros[k].after_update()
    step_ms = {k: [] for k in ros}
    for _ in range(rounds):
        for k in ros:  # alternating
            step_ms[k].append(timed(lambda: rollout(ros[k], acts), 1) / T)
            ros[k].after_update()
    res["step_us"] = {k: [round(1e3 * x, 2) for x in v] for k, v in step_ms.items()}
    # the same T steps in a captured graph: what is left when the host's launch path is out of the picture
    graph_us = {}
    grs = {}
    for k in ros:
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        grs[k] = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(grs[k], stream=side):  # (one stream, no parallel branches)
                rollout(ros[k], acts)
        torch.cuda.current_stream(dev).wait_stream(side)
        grs[k].replay()
        graph_us[k] = []
    for _ in range(rounds):
        for k in ros:  # alternating
            graph_us[k].append(round(1e3 * timed(grs[k].replay, 1) / T, 2))
    del grs
    res["step_us_graph"] = graph_us
    # the same frames in all three (twin batches, same actions): compare once at the size that is timed
    ref = ros["stacked"].observations[T]
    res["equal"] = bool(torch.equal(ros["frames_time"].stack_at(T), ref) and torch.equal(ros["frames_env"].stack_at(T), ref))
    # minibatch gathers
    gather = {}
    for what, m, dtype in (("u8", T * n // 4, torch.uint8), ("f32", T * n // 16, torch.float32)):
        idx = torch.randperm(T * n, device=dev)[:m]
        out = torch.empty((m, S, 84, 84), dtype=dtype, device=dev)
        obs = ros["stacked"].observations[:-1].reshape(T * n, S, 84, 84)
        fns = {"stacked": (lambda: obs[idx]) if dtype == torch.uint8 else (lambda: obs[idx].float()),
               "stacked_index_select_out": (lambda: torch.index_select(obs, 0, idx, out=out)) if dtype == torch.uint8 else None,
               "frames_time": lambda: ros["frames_time"].stacks(idx, out=out),
               "frames_env": lambda: ros["frames_env"].stacks(idx, out=out)}
        moved = m * STACK * (1 + out.element_size())
        row = {"samples": m, "bytes_moved": moved}
        for k, fn in fns.items():
            if fn is None:
                continue
            fn()
            ms = [timed(fn, 5) for _ in range(rounds)]
            row[k] = {"ms": [round(x, 3) for x in ms], "GBps": round(moved / (min(ms) * 1e-3) / 1e9, 1)}
        row["equal"] = bool(torch.equal(ros["frames_time"].stacks(idx, dtype=dtype), obs[idx].to(dtype)))
        gather[what] = row
        del out
    res["gather"] = gather
    for e in envs.values():
        e.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None, help="directory for frame_rollout_probe.json")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "the probe measures on a GPU"
    all_res = {"build_id": _lib.lib().sf_build_id().decode(), "device": torch.cuda.get_device_name(0), "results": []}
    for n in a.envs:
        r = probe(n, a.steps, a.rounds)
        all_res["results"].append(r)
        print(json.dumps(r), flush=True)
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(a.out, exist_ok=True)
        with open(os.path.join(a.out, "frame_rollout_probe.json"), "w") as f:
            json.dump(all_res, f, indent=1)


if __name__ == "__main__":
    main()
