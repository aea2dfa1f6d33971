#!/usr/bin/env python3
"""A/B timing for the final-observation output (profiles/final_obs.md): differently built libsfmi variants on ONE device in
interleaved rounds, like tools/ab.py, for the three launches that change can touch:

    step          the plain step (sf_step), HIP graphs of 256 launches        -- the split launch at <= 65 536 envs
    step-fobs     the same with SFVecEnv.enable_final_obs()                   -- the XTRA/FOBS instantiation (new libraries only)
    rollout-samp  sf_rollout_sampled, K ticks per launch                      -- the fused XTRA instantiation

    python tools/final_obs_ab.py parent.so child.so [--modes step,rollout-samp,step-fobs] [--envs 65536] [--rounds 5]

Each (variant, mode) runs in its own subprocess per round (a process loads one libsfmi); rounds interleave them.  Prints the
median and the spread of the rounds in us per tick.  A block spans two episode rollovers (5 295 ticks each), so the tick on
which every env finishes, and writes its row, is inside the window.
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(a):
    sys.path.insert(0, ROOT)
    import torch
    from spacefortress_amd import SFVecEnv

    n, K = a.envs, a.k
    env = SFVecEnv(n, gametype=a.gametype, spawn_stride=1, reuse_buffers=True)
    env.reset()
    if a.child == "step-fobs":
        env.enable_final_obs()
    dev = env.device
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    if a.child == "rollout-samp":
        env.seed_actions(7)
        launches = max(1, a.ticks // K)
        run = lambda: [env.rollout_sampled(K, want_actions=False) for _ in range(launches)]
        ticks = launches * K
    else:
        g = torch.Generator().manual_seed(1)
        acts = torch.randint(0, env.n_actions, (256, n), generator=g, dtype=torch.uint8).to(dev)
        side = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(side):
            for k in range(8):
                env.step_tensors(acts[k])
        side.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):
                for k in range(256):
                    env.step_tensors(acts[k])
        torch.cuda.synchronize()
        reps = max(1, a.ticks // 256)
        run = lambda: [graph.replay() for _ in range(reps)]
        ticks = reps * 256
    run()  # warm-up: one whole block
    torch.cuda.synchronize()
    blocks = []
    for _ in range(a.blocks):
        ev[0].record()
        run()
        ev[1].record()
        torch.cuda.synchronize()
        blocks.append(ev[0].elapsed_time(ev[1]) * 1e3 / ticks)
    env.check_state()
    print(json.dumps({"us_per_tick": sorted(blocks)[len(blocks) // 2], "blocks": blocks, "ticks": ticks,
                      "episodes": int(env.episode_stats()[0])}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="*")
    ap.add_argument("--modes", default="step,rollout-samp,step-fobs")
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--ticks", type=int, default=12032, help="ticks per timed block")
    ap.add_argument("--blocks", type=int, default=5, help="timed blocks per process (their median is the round's figure)")
    ap.add_argument("--k", type=int, default=64, help="ticks per sf_rollout_sampled launch")
    ap.add_argument("--gametype", default="youturn")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    jobs = [(l, m) for m in a.modes.split(",") for k, l in enumerate(a.libs) if m != "step-fobs" or k == len(a.libs) - 1]
    res = {j: [] for j in jobs}
    for r in range(a.rounds):
        for l, m in jobs:
            env = dict(os.environ, SFMI_LIB_PATH=os.path.abspath(l))
            out = subprocess.check_output([sys.executable, os.path.abspath(__file__), "--child", m, "--envs", str(a.envs), "--ticks",
                                           str(a.ticks), "--blocks", str(a.blocks), "--k", str(a.k), "--gametype", a.gametype],
                                          env=env, stderr=subprocess.DEVNULL, text=True, timeout=300)
            res[(l, m)].append(json.loads(out.strip().splitlines()[-1])["us_per_tick"])
    for (l, m), v in res.items():
        s = sorted(v)
        print("%-14s %-28s median %.3f us  min %.3f  max %.3f  (%s)" % (m, os.path.basename(l), s[len(s) // 2], s[0], s[-1],
                                                                       " ".join("%.3f" % x for x in v)))


if __name__ == "__main__":
    main()
