"""Lane states: time save / load / fork / copy (sfmi.h: sf_save_lanes ...) at 4 096 and 65 536 lanes with device events,
warmed up, over a window of many calls, and report GB/s against the bytes each call moves and against sf_calibration_copy's
ceiling (the step kernel's own access pattern, 16 B per lane, 64-lane rows).

    python tools/lanes_probe.py [--iters 200] [--sizes 4096,65536]

Bytes per env (estimates from sizes, not counters): save reads the lane's 47 state chunks (752 B) and its tile's pool
entries it owns, writes a 1136-byte row; load reads the row and writes the 47 chunks plus the pool entries; fork = load of ONE
row into every lane (the row stays in cache: write-bound); copy = save + load through the batch's scratch rows."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from spacefortress_amd import SFVecEnv, _lib  # noqa: E402

ROW = _lib.LANE_STATE_BYTES
CHUNKS = 47 * 16


def timed(fn, iters, warm=20):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # us per call


def ceiling(env):
    """GB/s of sf_calibration_copy: bytes it reports over the device time between two events around it (it synchronises
    itself, so one call per window: the launch's ramp is in it as it is in every call measured here)"""
    moved = C.c_size_t()
    L = _lib.lib()
    L.sf_calibration_copy(env._h, 0, C.byref(moved))
    best = None
    for _ in range(10):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        L.sf_calibration_copy(env._h, 0, C.byref(moved))
        b.record()
        torch.cuda.synchronize()
        ms = a.elapsed_time(b)
        best = ms if best is None else min(best, ms)
    return moved.value / (best * 1e-3) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--sizes", default="4096,65536")
    args = ap.parse_args()
    rng = np.random.default_rng(0)
    out = []
    for n in [int(s) for s in args.sizes.split(",")]:
        env = SFVecEnv(n, gametype="youturn", spawn_stride=1)
        env.rollout(torch.from_numpy(rng.integers(0, 5, (200, n)).astype(np.uint8)).to(env.device), want_obs=False)
        L, h, st = env._L, env._h, env._stream()
        rows = torch.empty((n, ROW), dtype=torch.uint8, device=env.device)
        perm = torch.randperm(n, device=env.device).to(torch.int32)
        zeros = torch.zeros(n, dtype=torch.int32, device=env.device)
        rp, pp, zp = C.c_void_p(rows.data_ptr()), C.c_void_p(perm.data_ptr()), C.c_void_p(zeros.data_ptr())
        L.sf_save_lanes(h, None, _lib.ACT_I32, n, rp, st)
        cases = {
            "save": (lambda: L.sf_save_lanes(h, None, _lib.ACT_I32, n, rp, st), CHUNKS + ROW),
            "load": (lambda: L.sf_load_lanes(h, pp, _lib.ACT_I32, n, rp, n, None, None, st), ROW + CHUNKS),
            "fork": (lambda: L.sf_load_lanes(h, None, _lib.ACT_I32, n, rp, 1, zp, None, st), CHUNKS),
            "copy": (lambda: L.sf_copy_lanes(h, pp, h, None, _lib.ACT_I32, n, None, st), 2 * (CHUNKS + ROW)),
        }
        cases["copy"][0]()  # (the scratch rows: made by the first call)
        ceil = ceiling(env)
        for name, (fn, bpe) in cases.items():
            us = timed(fn, args.iters)
            gbs = n * bpe / us / 1e3
            out.append({"n_envs": n, "op": name, "us": round(us, 2), "bytes_per_env": bpe, "GB/s": round(gbs, 1),
                        "of_ceiling": round(gbs / ceil, 3), "ceiling_GB/s": round(ceil, 1)})
            print(json.dumps(out[-1]), flush=True)
        _lib.check(L.sf_check_lanes(h, st))
        env.close()


if __name__ == "__main__":
    main()
