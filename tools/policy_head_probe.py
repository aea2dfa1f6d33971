#!/usr/bin/env python3
"""What the policy head costs and what it replaces (profiles/policy_head.md).

    python tools/policy_head_probe.py [--shapes 256x5,4096x5,65536x5,65536x16] [--blocks 15] [--calls 200]
    python tools/policy_head_probe.py --example [--parent-tree DIR] [--rounds 3] [--envs 4096] [--iters 20]

Without --example: per shape, on ONE stream after a warm-up of both, blocks of `calls` calls timed with device events, the two
paths alternating block by block, the median over a path's blocks (and, for the head alone, `calls` launches captured in one
graph and replayed per block: what a launch takes once the host is out of the way):
  head    PolicyHead.sample(logits, out=(actions, action_log_probs row, entropy)): ONE launch;
  torch   what examples/ppo_loop.py does per agent step without --device-policy-head, as it stands there (argument validation
          of torch.distributions at its default): Categorical(logits=...), sample(), log_prob(action).unsqueeze(1), and the
          two copy_ into the rollout's actions and action_log_probs rows.
With --example: examples/ppo_loop.py --envs N --iters K in a fresh process per run, `rounds` rounds that rotate through this tree
without the flag, this tree with --device-policy-head, and -- given --parent-tree, a checkout of the parent commit with its own
built library -- the parent's example: the env-steps/s of each run's last log line.  One run in front is not counted (the
first process on a box starts cold).  Prints JSON lines, then a table.
"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def launches(a):
    sys.path.insert(0, ROOT)
    import torch
    from spacefortress_amd import PolicyHead

    dev = torch.device("cuda", torch.cuda.current_device())
    rows = []
    for shape in a.shapes.split(","):
        n, A = (int(v) for v in shape.split("x"))
        g = torch.Generator().manual_seed(n + A)
        x = torch.randn(n, A, generator=g).to(dev)
        head = PolicyHead(n, A, seed=1, device=dev)
        act8 = torch.zeros(n, dtype=torch.uint8, device=dev)
        actions, logps, ent = torch.zeros(n, 1, dtype=torch.long, device=dev), torch.zeros(n, 1, device=dev), torch.zeros(n, device=dev)

        def run_head():
            head.sample(x, out=(act8, logps, ent))

        def run_torch():
            dist = torch.distributions.Categorical(logits=x)
            action = dist.sample()
            lp = dist.log_prob(action).unsqueeze(1)
            actions.copy_(action.unsqueeze(1))
            logps.copy_(lp)

        def block(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / a.calls

        def block_of(replay):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            replay()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / a.calls

        per = {"head": [], "torch": []}
        for fn in (run_head, run_torch):  # warm-up: every launch shape the timed window uses
            block(fn)
        for _ in range(a.blocks):
            per["head"].append(block(run_head))
            per["torch"].append(block(run_torch))
        # the head alone, off the host's clock: `calls` launches captured in one graph, a replay per block
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(g, stream=side):
                for _ in range(a.calls):
                    run_head()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize()
        per["graph"] = [block_of(g.replay) for _ in range(a.blocks + 1)][1:]
        assert head.check() == 0
        row = {"envs": n, "actions": A, "calls_per_block": a.calls,
               "head_in_graph_us": statistics.median(per["graph"]), "head_in_graph_min_max": [min(per["graph"]), max(per["graph"])],
               "head_us": statistics.median(per["head"]), "head_min_max": [min(per["head"]), max(per["head"])],
               "torch_us": statistics.median(per["torch"]), "torch_min_max": [min(per["torch"]), max(per["torch"])]}
        print(json.dumps(row), flush=True)
        rows.append(row)
    print("\n| envs x actions | head us / call: median (min .. max) | torch path us / call: median (min .. max) | torch / head "
          "| head us / launch inside a graph |")
    print("|---|---|---|---|---|")
    for r in rows:
        print("| %d x %d | %.2f (%.2f .. %.2f) | %.2f (%.2f .. %.2f) | %.1f | %.2f (%.2f .. %.2f) |" % (
            r["envs"], r["actions"], r["head_us"], *r["head_min_max"], r["torch_us"], *r["torch_min_max"], r["torch_us"] / r["head_us"],
            r["head_in_graph_us"], *r["head_in_graph_min_max"]))
    return 0


def example(a):
    variants = [("this", ROOT, []), ("this --device-policy-head", ROOT, ["--device-policy-head"])]
    if a.parent_tree:
        variants.insert(0, ("parent", os.path.abspath(a.parent_tree), []))
    rate = re.compile(r"iter\s+%d\s+env-steps\s+\d+\s+(\S+) env-steps/s" % a.iters)
    runs = {name: [] for name, _, _ in variants}
    for r in range(-1, a.rounds):  # round -1: the box's first process pays for cold caches; run and shown, not counted
        k = r % len(variants)  # the order rotates: a run's place in the round shows in its rate (profiles/policy_head.md)
        for name, tree, flags in (variants[:1] if r < 0 else variants[k:] + variants[:k]):
            out = subprocess.run([sys.executable, os.path.join(tree, "examples", "ppo_loop.py"), "--envs", str(a.envs), "--iters",
                                  str(a.iters)] + flags, cwd=tree, capture_output=True, text=True, timeout=240)
            if out.returncode != 0:
                sys.stderr.write(out.stdout[-1000:] + out.stderr[-2000:])
                return out.returncode  # (nothing more is started behind a run that failed)
            m = rate.search(out.stdout)
            assert m, out.stdout[-1000:]
            if r >= 0:
                runs[name].append(float(m.group(1)))
            extra = [l.strip() for l in out.stdout.splitlines() if "policy head" in l][-1:]
            print(json.dumps({"variant": name, "round": r, "env_steps_per_s": float(m.group(1)), "log": extra}), flush=True)
    print("\n| examples/ppo_loop.py --envs %d --iters %d | env-steps/s (whole loop), per round | min .. max |" % (a.envs, a.iters))
    print("|---|---|---|")
    for name, v in runs.items():
        print("| %s | %s | %.3g .. %.3g |" % (name, ", ".join("%.3g" % x for x in v), min(v), max(v)))
    return 0


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shapes", default="256x5,4096x5,65536x5,65536x16")
    p.add_argument("--blocks", type=int, default=15)
    p.add_argument("--calls", type=int, default=200)
    p.add_argument("--example", action="store_true")
    p.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--envs", type=int, default=4096)
    p.add_argument("--iters", type=int, default=20)
    a = p.parse_args()
    return example(a) if a.example else launches(a)


if __name__ == "__main__":
    sys.exit(main())
