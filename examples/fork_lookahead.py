"""One-step-greedy lookahead from the true simulator, with lane states (sfmi.h: sf_save_lanes / sf_load_lanes).

Every env of a batch is forked into one lane per action of a second batch (a one-to-many load: row i into lanes
i * A .. i * A + A - 1), each fork plays its first action and then k random ticks, and the env takes the action whose forks
scored best.

    python examples/fork_lookahead.py [--envs 64] [--k 16] [--steps 50]
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from spacefortress_amd import SFVecEnv  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=64)
    ap.add_argument("--k", type=int, default=16)
    ap.add_argument("--steps", type=int, default=50)
    args = ap.parse_args()
    n = args.envs
    env = SFVecEnv(n, gametype="autoturn")
    A = env.n_actions
    sim = SFVecEnv(n * A, gametype="autoturn")  # the same preset, seed and spawn table: the rows load there
    dev = env.device
    g = torch.Generator(device=dev).manual_seed(0)
    fork_rows = torch.arange(n, device=dev).repeat_interleave(A)  # row i -> lanes i*A .. i*A+A-1
    first = torch.arange(A, device=dev, dtype=torch.uint8).repeat(n)
    total = torch.zeros(n, dtype=torch.int64, device=dev)
    for _ in range(args.steps):
        sim.load_lanes(env.save_lanes(), rows=fork_rows, check=False)
        ret = sim.step_tensors(first)[1].to(torch.int64)
        for _ in range(args.k):
            a = torch.randint(0, A, (n * A,), device=dev, dtype=torch.uint8, generator=g)
            ret += sim.step_tensors(a)[1]
        best = ret.view(n, A).argmax(1).to(torch.uint8)
        total += env.step_tensors(best)[1]
    sim.check_lanes()
    print("mean return over %d steps of %d envs with %d-tick lookahead: %.2f" % (args.steps, n, args.k, total.float().mean().item()))


if __name__ == "__main__":
    main()
