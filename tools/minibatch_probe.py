#!/usr/bin/env python3
"""What a PPO minibatch costs to sample, and what the whole loop makes of it (profiles/minibatch.md).

    python tools/minibatch_probe.py [--shapes 4096x20,16384x20] [--frames 1024x32] [--blocks 15] [--calls 50] [--graph-calls 20]
    python tools/minibatch_probe.py --example --parent-tree DIR [--rounds 3] [--envs 4096] [--iters 20]

Without --example: per shape envs x steps (four minibatches, as the example's defaults have them), on ONE stream after a warm-up
of both, one minibatch timed in blocks of `calls` between two device events, the two paths alternating block by block, the
median over a path's blocks:
  gather  MiniBatcher.next(): one gather launch and the one-thread advance of the device cursor, into fixed buffers
          (FrameRollout: then sf_gather_stacks on the gathered row indices);
  index   the body of feed_forward_generator as it stands: seven fancy-index launches on a slice of the permutation, into fresh
          tensors (FrameRollout: sf_gather_stacks and six).
Then both once more with the host out of the way: `graph-calls` minibatches captured in one graph and replayed per block.
`--frames` shapes run a FrameRollout (uint8 stacks, S = 4) instead of a DeviceRollout.  Run the same call twice for the spread.
With --example: examples/ppo_loop.py --envs N --iters K in a fresh process per run, `rounds` rounds that rotate through the
parent's tree with --device-policy-head (a checkout of the parent commit with its own built library) and this tree with
--device-policy-head --device-minibatches and with --graph-update: the env-steps/s of each run's last log line.  One run in
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
    from spacefortress_amd import DeviceRollout, FrameRollout, SFVecEnv

    rows = []
    cases = [(s, False) for s in a.shapes.split(",") if s] + [(s, True) for s in a.frames.split(",") if s]
    for shape, frames in cases:
        n, T = (int(v) for v in shape.split("x"))
        env = SFVecEnv(n, gametype="autoturn", obs_type="image" if frames else "features", spawn_stride=1)
        dev = env.device
        ro = FrameRollout(env, T, num_stack=4) if frames else DeviceRollout(env, T)
        for t in (ro.states, ro.returns, ro.value_preds, ro.action_log_probs):
            t.normal_()
        if frames:
            ro.frames.random_(0, 256)
        else:
            ro.observations.normal_()
        adv = ro.advantages()
        nmb = 4
        batch = T * n
        mb = batch // nmb
        b = ro.batcher(adv, nmb)
        b.shuffle()
        perm = b.index.clone()
        flat = lambda t: t.reshape(batch, t.shape[-1])
        cols = [flat(ro.states[:-1]), flat(ro.actions), flat(ro.returns[:-1]), flat(ro.masks[:-1]), flat(ro.action_log_probs),
                adv.reshape(batch, 1)]
        obs = None if frames else ro.observations[:-1].reshape(batch, *ro.observations.shape[2:])
        state = {"k": 0}

        def run_index():
            k = state["k"] = (state["k"] + 1) % nmb
            idx = perm[k * mb:(k + 1) * mb]
            first = ro.stacks(idx) if frames else obs[idx]
            return (first,) + tuple(c[idx] for c in cols)

        def run_gather():
            return b.next()

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

        calls = max(2, a.calls // 10) if frames else a.calls
        per = {"gather": [], "index": [], "gather_graph": [], "index_graph": []}
        for fn in (run_gather, run_index):  # warm-up: every launch shape the timed window uses
            block(fn, calls)
        b.shuffle(perm)  # the two paths agree on minibatch 0
        state["k"] = -1
        same = all(bool((p == q).all()) for p, q in zip(run_gather(), run_index()))
        for _ in range(a.blocks):
            per["gather"].append(block(run_gather, calls))
            per["index"].append(block(run_index, calls))
        graphs = {"gather_graph": captured(run_gather), "index_graph": captured(run_index)}
        for _ in range(a.blocks + 1):  # (the first replay of each is not counted)
            for k, graph in graphs.items():
                per[k].append(block(graph.replay, 1) / a.graph_calls)
        for k in graphs:
            per[k] = per[k][1:]
        assert b.errors() == 0 and same
        row_bytes = sum(t.element_size() * t[0].numel() for t in b.tuple)
        row = {"rollout": "frames" if frames else "features", "envs": n, "steps": T, "rows_per_minibatch": mb,
               "bytes_per_minibatch": row_bytes * mb, "calls_per_block": calls, "minibatches_per_graph": a.graph_calls}
        for k, v in per.items():
            row[k + "_us"] = statistics.median(v)
            row[k + "_min_max"] = [min(v), max(v)]
        print(json.dumps(row), flush=True)
        rows.append(row)
        del graphs, b, ro
        env.close()
    print("\n| rollout, envs x steps, rows per minibatch | gather, from Python | index, from Python | index / gather "
          "| gather, in a graph | index, in a graph | index / gather |")
    print("|---|---|---|---|---|---|---|")
    for r in rows:
        cell = lambda k: "%.1f (%.1f .. %.1f)" % (r[k + "_us"], *r[k + "_min_max"])
        print("| %s, %d x %d, %d | %s | %s | %.2f | %s | %s | %.2f |" % (
            r["rollout"], r["envs"], r["steps"], r["rows_per_minibatch"], cell("gather"), cell("index"),
            r["index_us"] / r["gather_us"], cell("gather_graph"), cell("index_graph"), r["index_graph_us"] / r["gather_graph_us"]))
    return 0


def example(a):
    variants = [("parent, --device-policy-head", os.path.abspath(a.parent_tree), ["--device-policy-head"]),
                ("this, --device-policy-head --device-minibatches", ROOT, ["--device-policy-head", "--device-minibatches"]),
                ("this, --graph-update", ROOT, ["--graph-update"])]
    rate = re.compile(r"iter\s+%d\s+env-steps\s+\d+\s+(\S+) env-steps/s" % a.iters)
    runs = {name: [] for name, _, _ in variants}
    for r in range(-1, a.rounds):  # round -1: the machine's first process pays for cold caches; run and shown, not counted
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
            extra = [l.strip() for l in out.stdout.splitlines() if "last minibatch" in l][-1:]
            print(json.dumps({"variant": name, "round": r, "env_steps_per_s": float(m.group(1)), "log": extra}), flush=True)
    print("\n| examples/ppo_loop.py --envs %d --iters %d | env-steps/s (whole loop), per round | min .. max | median |" % (a.envs, a.iters))
    print("|---|---|---|---|")
    for name, v in runs.items():
        print("| %s | %s | %.3g .. %.3g | %.3g |" % (name, ", ".join("%.3g" % x for x in v), min(v), max(v), statistics.median(v)))
    return 0


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--shapes", default="4096x20,16384x20", help="DeviceRollout shapes, envs x steps")
    p.add_argument("--frames", default="1024x32", help="FrameRollout shapes, envs x steps")
    p.add_argument("--blocks", type=int, default=15)
    p.add_argument("--calls", type=int, default=50)
    p.add_argument("--graph-calls", type=int, default=20)
    p.add_argument("--example", action="store_true")
    p.add_argument("--parent-tree", default=None, help="a checkout of the parent commit with its library built")
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--envs", type=int, default=4096)
    p.add_argument("--iters", type=int, default=20)
    a = p.parse_args()
    if a.example and not a.parent_tree:
        p.error("--example needs --parent-tree")
    return example(a) if a.example else launches(a)


if __name__ == "__main__":
    sys.exit(main())
