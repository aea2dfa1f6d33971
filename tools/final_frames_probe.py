#!/usr/bin/env python3
"""What the final-frame output costs (profiles/final_frames.md): the image step of a batch, default geometry, timed with the
output off and on, and against another build of libsfmi (the parent commit's), on ONE device in interleaved rounds.

    python tools/final_frames_probe.py [--parent parent.so] [--envs 16384,256] [--rounds 3] [--blocks 10] [--steps 100]

Each (variant, batch size) runs in its own subprocess per round (a process loads one libsfmi); rounds interleave the
variants: `this` (this tree's library, blocks alternating output off / output on), `this-plain` (the same library, the output
never switched on) and `parent`.  A frame's cost depends on what the games show, which depends on how long they have run, so
EVERY variant plays the same schedule from the same reset -- blocks of `steps` step_tensors calls in alternating slots A and B,
each timed with device events around it, no env finishing inside one -- and only `this` has the output on in its B slots: A
against A and B against B compare the same ticks of the same games.  Then the tick on which EVERY env finishes, five times per
mode: the clocks are set, the device drained, one step timed.  Prints one JSON line per child and, at the end, medians over a
slot's blocks, per round, in us per step.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(a):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from spacefortress_amd import SFVecEnv, _lib

    n = a.child_envs
    env = SFVecEnv(n, gametype="youturn", obs_type="image", reuse_buffers=True)
    has_final = a.child == "this"
    assert not has_final or hasattr(_lib.lib(), "sf_set_final_frame_output")
    dev = env.device
    g = torch.Generator().manual_seed(1)
    acts = torch.randint(0, env.n_actions, (a.steps, n), generator=g, dtype=torch.uint8).to(dev)
    fin = torch.zeros((n, 1, 84, 84), dtype=torch.uint8, device=dev) if has_final else None
    modes = ["off", "on"]  # slots A and B: "on" is off as well where the output is never switched on
    assert a.steps * (a.blocks * len(modes) + 2) < env.max_ticks, "an env would finish inside a timed block"

    def switch(mode):
        if has_final:
            env.enable_final_frames(out=fin) if mode == "on" else env.enable_final_frames(False)

    def block():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for k in range(a.steps):
            env.step_tensors(acts[k])
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.steps

    env.reset()
    for mode in modes:  # warm-up: every launch shape the timed window uses
        switch(mode)
        block()
    per = {m: [] for m in modes}
    for _ in range(a.blocks):
        for mode in modes:
            switch(mode)
            per[mode].append(block())
    # the tick on which every env finishes
    finish = {m: [] for m in modes}
    two_left = np.full(n, 180000 - 2 * 34, np.int32)
    for _ in range(5):
        for mode in modes:
            switch(mode)
            env.set_field("time", two_left)
            _, _, done, _ = env.step_tensors(acts[0])  # (not timed: the frame behind an edit rebuilds the draw records)
            torch.cuda.synchronize()
            assert not bool(done.any())
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _, _, done, _ = env.step_tensors(acts[1])
            e1.record()
            torch.cuda.synchronize()
            assert bool(done.all())
            finish[mode].append(e0.elapsed_time(e1) * 1e3)
    if not has_final:
        per, finish = {"off": per["off"], "off (B slots)": per["on"]}, {"off": finish["off"], "off (B slots)": finish["on"]}
    print(json.dumps({"lib": a.child, "build": _lib.lib().sf_build_id().decode(), "envs": n, "step_us": per, "all_finish_us": finish}))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--parent", default=None, help="another libsfmi.so to compare with (the parent commit's build)")
    p.add_argument("--envs", default="16384,256")
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--blocks", type=int, default=10)
    p.add_argument("--steps", type=int, default=100)
    p.add_argument("--child", default=None)
    p.add_argument("--child-envs", type=int, default=0)
    a = p.parse_args()
    if a.child:
        return child(a)
    libs = [("this", None), ("this-plain", None)] + ([("parent", os.path.abspath(a.parent))] if a.parent else [])
    results = []
    for r in range(a.rounds):
        for n in (int(x) for x in a.envs.split(",")):
            for name, path in (libs if r % 2 == 0 else libs[::-1]):
                env = dict(os.environ)
                if path:
                    env["SFMI_LIB_PATH"] = path
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name, "--child-envs", str(n), "--blocks",
                                      str(a.blocks), "--steps", str(a.steps)], env=env, capture_output=True, text=True, timeout=300)
                if out.returncode != 0:
                    sys.stderr.write(out.stderr[-2000:])
                    return out.returncode  # (nothing more is started behind a child that failed)
                line = out.stdout.strip().splitlines()[-1]
                print(line, flush=True)
                results.append(json.loads(line))
    print("\n| envs | variant (build) | mode | step us: median of the slot's blocks, per round | min .. max of all blocks | all-finish tick us: median (min .. max) |")
    print("|---|---|---|---|---|---|")
    keys = sorted({(x["envs"], x["lib"]) for x in results}, key=lambda k: (-k[0], k[1]))
    for n, lib in keys:
        runs = [x for x in results if x["envs"] == n and x["lib"] == lib]
        for mode in runs[0]["step_us"]:
            meds = [statistics.median(x["step_us"][mode]) for x in runs]
            allb = [v for x in runs for v in x["step_us"][mode]]
            fin = [v for x in runs for v in x["all_finish_us"][mode]]
            print("| %d | %s (%s) | %s | %s | %.1f .. %.1f | %.0f (%.0f .. %.0f) |"
                  % (n, lib, runs[0]["build"], mode, ", ".join("%.1f" % m for m in meds), min(allb), max(allb),
                     statistics.median(fin), min(fin), max(fin)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
