#!/usr/bin/env python3
"""What the PPO loss head costs and what it replaces (profiles/policy_eval.md).

    python tools/policy_eval_probe.py [--shapes 4096x5,327680x5,327680x16] [--blocks 15] [--calls 100] [--graph-calls 50]
    python tools/policy_eval_probe.py --example --parent-tree DIR [--rounds 4] [--envs 4096] [--iters 20]

Without --example: per shape M x A, on ONE stream after a warm-up of both, forward + backward of the loss head alone -- from the
network's logits [M, A] and values [M, 1] to their gradients -- timed in blocks of `calls` between two device events, the two
paths alternating block by block, the median over a path's blocks:
  device  spacefortress_amd.ppo_loss(...) and torch.autograd.grad of its loss: two launches forward, one backward (and what
          autograd adds around them);
  torch   the expressions of examples/ppo_loop.py's default update, as they stand there: Categorical(logits=...) with its
          default argument validation, log_prob, exp, two products, clamp, min, the three means, the weighted sum, and
          torch.autograd.grad of that.
Then both once more with the host out of the way: `graph-calls` forward + backward passes captured in one graph and replayed per
block (the torch path with validate_args=False there: the validation reads a flag back to the host, which a capture refuses).
With --example: examples/ppo_loop.py --device-policy-head --envs N --iters K in a fresh process per run, `rounds` rounds that
rotate through the parent's tree (a checkout of the parent commit with its own built library, where the flag moves the sampling
only) and this tree (where it moves the update's loss head as well): the env-steps/s of each run's last log line.  One run in
front is not counted.  Prints JSON lines, then a table.
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
    from spacefortress_amd import ppo_loss

    dev = torch.device("cuda", torch.cuda.current_device())
    rows = []
    for shape in a.shapes.split(","):
        M, A = (int(v) for v in shape.split("x"))
        g = torch.Generator().manual_seed(M + A)
        logits = torch.randn(M, A, generator=g).to(dev).requires_grad_(True)
        values = torch.randn(M, 1, generator=g).to(dev).requires_grad_(True)
        act = torch.randint(0, A, (M, 1), generator=g).to(dev)
        with torch.no_grad():
            old = torch.log_softmax(logits, 1).gather(1, act) + 0.1 * torch.randn(M, 1, generator=g).to(dev)
        adv, ret = torch.randn(M, 1, generator=g).to(dev), torch.randn(M, 1, generator=g).to(dev)

        def run_device():
            loss = ppo_loss(logits, values, act, old, adv, ret, 0.1, 0.5, 0.01)[0]
            return torch.autograd.grad(loss, [logits, values])

        def run_torch(validate=None):
            dist = torch.distributions.Categorical(logits=logits, validate_args=validate)
            ratio = torch.exp(dist.log_prob(act.squeeze(1)).unsqueeze(1) - old)
            loss = (-torch.min(ratio * adv, torch.clamp(ratio, 0.9, 1.1) * adv).mean()
                    + 0.5 * (values - ret).pow(2).mean() - 0.01 * dist.entropy().mean())
            return torch.autograd.grad(loss, [logits, values])

        def block(fn, calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / calls

        def captured(fn):
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                for _ in range(3):
                    fn()
                side.synchronize()
                with torch.cuda.graph(graph, stream=side):
                    for _ in range(a.graph_calls):
                        fn()
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize()
            return graph

        per = {"device": [], "torch": [], "device_graph": [], "torch_graph": []}
        for fn in (run_device, run_torch):  # warm-up: every launch shape the timed window uses
            block(fn, a.calls)
        d, t = run_device(), run_torch()
        agree = max(float((p - q).abs().max()) for p, q in zip(d, t))
        for _ in range(a.blocks):
            per["device"].append(block(run_device, a.calls))
            per["torch"].append(block(run_torch, a.calls))
        graphs = {"device_graph": captured(run_device)}
        try:
            graphs["torch_graph"] = captured(lambda: run_torch(False))
        except RuntimeError as e:  # (said in the table, not hidden: the torch path could not be captured on this stack)
            print(json.dumps({"rows": M, "actions": A, "torch_graph": "not captured: %s" % str(e).splitlines()[0]}), flush=True)
        for _ in range(a.blocks + 1):  # (the first replay of each is not counted)
            for k, graph in graphs.items():
                per[k].append(block(graph.replay, 1) / a.graph_calls)
        for k in graphs:
            per[k] = per[k][1:]
        assert ppo_loss.check() == 0
        row = {"rows": M, "actions": A, "calls_per_block": a.calls, "passes_per_graph": a.graph_calls, "largest_gradient_difference": agree}
        for k, v in per.items():
            row[k + "_us"] = statistics.median(v) if v else float("nan")
            row[k + "_min_max"] = [min(v), max(v)] if v else [float("nan")] * 2
        print(json.dumps(row), flush=True)
        rows.append(row)
    print("\n| rows x actions | device, from Python | torch, from Python | torch / device | device, in a graph | torch, in a graph "
          "| torch / device |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        cell = lambda k: "%.1f (%.1f .. %.1f)" % (r[k + "_us"], *r[k + "_min_max"])
        print("| %d x %d | %s | %s | %.1f | %s | %s | %.1f |" % (
            r["rows"], r["actions"], cell("device"), cell("torch"), r["torch_us"] / r["device_us"], cell("device_graph"),
            cell("torch_graph"), r["torch_graph_us"] / r["device_graph_us"]))
    return 0


def example(a):
    flags = ["--device-policy-head"]
    variants = [("parent", os.path.abspath(a.parent_tree)), ("this", ROOT)]
    rate = re.compile(r"iter\s+%d\s+env-steps\s+\d+\s+(\S+) env-steps/s" % a.iters)
    runs = {name: [] for name, _ in variants}
    for r in range(-1, a.rounds):  # round -1: the machine's first process pays for cold caches; run and shown, not counted
        k = r % len(variants)  # the order rotates: a run's place in the round shows in its rate (profiles/policy_head.md)
        for name, tree in (variants[:1] if r < 0 else variants[k:] + variants[:k]):
            out = subprocess.run([sys.executable, os.path.join(tree, "examples", "ppo_loop.py"), "--envs", str(a.envs), "--iters",
                                  str(a.iters)] + flags, cwd=tree, capture_output=True, text=True, timeout=240)
            if out.returncode != 0:
                sys.stderr.write(out.stdout[-1000:] + out.stderr[-2000:])
                return out.returncode  # (nothing more is started behind a run that failed)
            m = rate.search(out.stdout)
            assert m, out.stdout[-1000:]
            if r >= 0:
                runs[name].append(float(m.group(1)))
            extra = [l.strip() for l in out.stdout.splitlines() if "last minibatch" in l][-1:]
            print(json.dumps({"variant": name, "round": r, "env_steps_per_s": float(m.group(1)), "log": extra}), flush=True)
    print("\n| examples/ppo_loop.py --device-policy-head --envs %d --iters %d | env-steps/s (whole loop), per round | min .. max "
          "| median |" % (a.envs, a.iters))
    print("|---|---|---|---|")
    for name, v in runs.items():
        print("| %s | %s | %.3g .. %.3g | %.3g |" % (name, ", ".join("%.3g" % x for x in v), min(v), max(v), statistics.median(v)))
    return 0


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shapes", default="4096x5,327680x5,327680x16")
    p.add_argument("--blocks", type=int, default=15)
    p.add_argument("--calls", type=int, default=100)
    p.add_argument("--graph-calls", type=int, default=50)
    p.add_argument("--example", action="store_true")
    p.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    p.add_argument("--rounds", type=int, default=4)
    p.add_argument("--envs", type=int, default=4096)
    p.add_argument("--iters", type=int, default=20)
    a = p.parse_args()
    if a.example and not a.parent_tree:
        p.error("--example needs --parent-tree")
    return example(a) if a.example else launches(a)


if __name__ == "__main__":
    sys.exit(main())
