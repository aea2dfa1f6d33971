#!/usr/bin/env python3
"""What the end of a PPO update costs -- clip_grad_norm_ + torch.optim.Adam(capturable=True) against DeviceAdam.step() -- and
what the whole loop makes of it (profiles/device_adam.md).

    python tools/adam_probe.py [--sets mlp,conv,acnet] [--blocks 15] [--calls 50] [--graph-calls 20] [--max-grad-norm 0.5]
    python tools/adam_probe.py --example [--rounds 3] [--envs 4096] [--iters 20]

Without --example: per parameter set, on ONE stream after a warm-up of both, one optimiser step timed in blocks of `calls`
between two device events, the two paths alternating block by block, the median over a path's blocks; then both once more with
the host out of the way: `graph-calls` steps captured in one graph and replayed per block.  The gradients are fixed random
tensors; clip_grad_norm_ scales them in place, so BOTH paths refill their grads from a copy inside the timed step (one
_foreach_copy_ each): the norm stays what it was and the two paths keep taking the same steps.  `launches` counts the device
kernels of one eager step of each path, the refill included, with torch's profiler.  Parameter sets:
  mlp    examples/ppo_loop.py's ActorCritic at the features observation (8 tensors)
  conv   its ConvActorCritic (10 tensors)
  acnet  14 tensors shaped like the reference's ACNet with its GRU, about 1.1e6 elements
With --example: examples/ppo_loop.py --graph-update --max-grad-norm X in a fresh process per run, with and without
--device-optimizer, `rounds` rounds in rotating order; the env-steps/s of each run's last log line.  One run in front is not
counted.  Prints JSON lines, then a table.
"""
import argparse
import importlib.util
import json
import os
import re
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the 14 tensors of the reference's ACNet with its GRU (rl/networks.py:24-32, three actions): two convolutions, a linear layer of
# 2592 -> 256, a GRU cell of 256 and the two heads; 1 071 924 elements
ACNET_SHAPES = [(16, 4, 8, 8), (16,), (32, 16, 4, 4), (32,), (256, 2592), (256,), (768, 256), (768, 256), (768,), (768,),
                (3, 256), (3,), (1, 256), (1,)]


def parameter_sets(names, dev):
    import torch

    spec = importlib.util.spec_from_file_location("ppo_loop_example", os.path.join(ROOT, "examples", "ppo_loop.py"))
    ex = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ex)
    torch.manual_seed(0)
    for name in names:
        if name == "mlp":
            ps = list(ex.ActorCritic(15, 3).to(dev).parameters())
        elif name == "conv":
            ps = list(ex.ConvActorCritic(4, 3).to(dev).parameters())
        elif name == "acnet":
            ps = [torch.nn.Parameter(torch.randn(s, device=dev) * 0.05) for s in ACNET_SHAPES]
        else:
            raise SystemExit("unknown parameter set %r" % name)
        yield name, ps


def kernel_nodes(graph_fn):
    """Kernel launches of one call of graph_fn, counted by the profiler's device-side kernel events."""
    import torch
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        graph_fn()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA and "Memcpy" not in e.name
               and "Memset" not in e.name)


def steps(a):
    sys.path.insert(0, ROOT)
    import torch
    from spacefortress_amd import DeviceAdam

    dev = torch.device("cuda", 0)
    rows = []
    for name, ps_t in parameter_sets([s for s in a.sets.split(",") if s], dev):
        ps_d = [torch.nn.Parameter(p.detach().clone()) for p in ps_t]
        grads = [torch.randn_like(p) * 0.1 for p in ps_t]
        for p, q, g in zip(ps_t, ps_d, grads):
            p.grad, q.grad = g.clone(), g.clone()
        gt, gd = [p.grad for p in ps_t], [q.grad for q in ps_d]
        topt = torch.optim.Adam(ps_t, lr=7e-4, capturable=True)
        dopt = DeviceAdam(ps_d, lr=7e-4, max_grad_norm=a.max_grad_norm)

        def run_torch():
            torch._foreach_copy_(gt, grads)
            torch.nn.utils.clip_grad_norm_(ps_t, a.max_grad_norm)
            topt.step()

        def run_device():
            torch._foreach_copy_(gd, grads)
            dopt.step()

        def block(fn, calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) * 1e3 / calls

        def captured(fn, n):
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                for _ in range(3):
                    fn()
                side.synchronize()
                with torch.cuda.graph(graph, stream=side):
                    for _ in range(n):
                        fn()
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize()
            return graph

        per = {"device": [], "torch": [], "device_graph": [], "torch_graph": []}
        for fn in (run_device, run_torch):  # warm-up: every launch shape the timed window uses
            block(fn, a.calls)
        for _ in range(a.blocks):
            per["device"].append(block(run_device, a.calls))
            per["torch"].append(block(run_torch, a.calls))
        graphs = {"device_graph": captured(run_device, a.graph_calls), "torch_graph": captured(run_torch, a.graph_calls)}
        for _ in range(a.blocks + 1):  # (the first replay of each is not counted)
            for k, graph in graphs.items():
                per[k].append(block(graph.replay, 1) / a.graph_calls)
        for k in graphs:
            per[k] = per[k][1:]
        launches = {}
        if not a.no_launch_count:
            try:
                launches = {"device": kernel_nodes(run_device), "torch": kernel_nodes(run_torch)}
            except Exception as e:  # (the profiler is a tool beside the measurement: its failure is reported, not hidden)
                launches = {"error": "%s: %s" % (type(e).__name__, e)}
        assert dopt.check() == 0
        # both paths took the same number of steps from the same start on the same gradients: how far apart they ended
        diff = max(float((p.detach() - q.detach()).abs().max()) for p, q in zip(ps_t, ps_d))
        row = {"set": name, "tensors": len(ps_t), "elements": sum(p.numel() for p in ps_t), "calls_per_block": a.calls,
               "steps_per_graph": a.graph_calls, "steps_taken": dopt.steps(), "max_abs_param_difference": diff,
               "launches_per_step_including_the_refill": launches, "last_norm": dopt.last_norm(), "last_coef": dopt.last_coef()}
        for k, v in per.items():
            row[k + "_us"] = statistics.median(v)
            row[k + "_min_max"] = [min(v), max(v)]
        print(json.dumps(row), flush=True)
        rows.append(row)
        del graphs
    print("\n| set, tensors, elements | DeviceAdam, from Python | clip + Adam, from Python | torch / device "
          "| DeviceAdam, in a graph | clip + Adam, in a graph | torch / device | launches device / torch |")
    print("|---|---|---|---|---|---|---|---|")
    for r in rows:
        cell = lambda k: "%.1f (%.1f .. %.1f)" % (r[k + "_us"], *r[k + "_min_max"])
        la = r["launches_per_step_including_the_refill"]
        print("| %s, %d, %d | %s | %s | %.2f | %s | %s | %.2f | %s / %s |" % (
            r["set"], r["tensors"], r["elements"], cell("device"), cell("torch"), r["torch_us"] / r["device_us"],
            cell("device_graph"), cell("torch_graph"), r["torch_graph_us"] / r["device_graph_us"], la.get("device", "-"),
            la.get("torch", "-")))
    return 0


def example(a):
    base = ["--graph-update", "--max-grad-norm", str(a.max_grad_norm)]
    variants = [("--graph-update --max-grad-norm, torch.optim.Adam", base), ("the same with --device-optimizer", base + ["--device-optimizer"])]
    rate = re.compile(r"iter\s+%d\s+env-steps\s+\d+\s+(\S+) env-steps/s" % a.iters)
    runs = {name: [] for name, _ in variants}
    for r in range(-1, a.rounds):  # round -1: the machine's first process pays for cold caches; run and shown, not counted
        k = r % len(variants)  # the order rotates: a run's place in the round shows in its rate (profiles/policy_head.md)
        for name, flags in (variants[:1] if r < 0 else variants[k:] + variants[:k]):
            out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ppo_loop.py"), "--envs", str(a.envs), "--iters",
                                  str(a.iters)] + flags, cwd=ROOT, capture_output=True, text=True, timeout=240)
            if out.returncode != 0:
                sys.stderr.write(out.stdout[-1000:] + out.stderr[-2000:])
                return out.returncode  # (nothing more is started behind a run that failed)
            m = rate.search(out.stdout)
            assert m, out.stdout[-1000:]
            if r >= 0:
                runs[name].append(float(m.group(1)))
            extra = [l.strip() for l in out.stdout.splitlines() if "device optimizer" in l][-1:]
            print(json.dumps({"variant": name, "round": r, "env_steps_per_s": float(m.group(1)), "log": extra}), flush=True)
    print("\n| examples/ppo_loop.py --envs %d --iters %d | env-steps/s (whole loop), per round | min .. max | median |" % (a.envs, a.iters))
    print("|---|---|---|---|")
    for name, v in runs.items():
        print("| %s | %s | %.3g .. %.3g | %.3g |" % (name, ", ".join("%.3g" % x for x in v), min(v), max(v), statistics.median(v)))
    return 0


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--sets", default="mlp,conv,acnet")
    p.add_argument("--blocks", type=int, default=15)
    p.add_argument("--calls", type=int, default=50)
    p.add_argument("--graph-calls", type=int, default=20)
    p.add_argument("--max-grad-norm", type=float, default=0.5)
    p.add_argument("--no-launch-count", action="store_true", help="skip the profiler pass that counts kernel launches")
    p.add_argument("--example", action="store_true")
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--envs", type=int, default=4096)
    p.add_argument("--iters", type=int, default=20)
    a = p.parse_args()
    return example(a) if a.example else steps(a)


if __name__ == "__main__":
    sys.exit(main())
