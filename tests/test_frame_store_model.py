"""The frame store (spacefortress_amd/frame_rollout.py, sfmi.h: sf_gather_stacks) without a GPU: the stack rule -- a stack as
a function of frames stored once and their start flags -- equals the trainer's own running update of its current observation
(rl/train.py:51-56,92-97) on random frames and done patterns, and the new entry point is declared, bound and exported."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from framestore_np import NpFrameStore, RunningStack, gather


def _run(n, T, S, rollouts, done_at, seed):
    """done_at(k, t, e) -> bool: does env e finish on step t of rollout k.  Checks every stack of every step."""
    rng = np.random.default_rng(seed)
    shape = (3, 5)
    first = rng.integers(1, 256, (n,) + shape).astype(np.uint8)  # (no zero pixels: a zeroed slot cannot pass for a frame)
    st = NpFrameStore(n, T, S, shape)
    st.reset(first)
    run = RunningStack(first, S)
    assert np.array_equal(st.stack_at(0), run.cur)
    for k in range(rollouts):
        per_step = [run.cur.copy()]
        for t in range(T):
            frame = rng.integers(1, 256, (n,) + shape).astype(np.uint8)
            done = np.array([done_at(k, t, e) for e in range(n)], np.uint8)
            st.step(t, frame, done)
            per_step.append(run.step(frame, done).copy())
            assert np.array_equal(st.stack_at(t + 1), per_step[-1]), (k, t)
        for t in range(T + 1):  # ... and every earlier step is still what it was
            assert np.array_equal(st.stack_at(t), per_step[t]), (k, t)
        idx = rng.permutation(T * n)
        got, bad = gather(st.frames, st.starts, S, idx)
        assert bad == 0 and np.array_equal(got, np.concatenate(per_step[:-1])[idx])
        st.after_update()
        assert np.array_equal(st.stack_at(0), per_step[-1]), k


@pytest.mark.parametrize("S", [1, 2, 3, 4, 5, 6])
def test_rule_equals_the_running_stack_on_random_dones(S):
    rng = np.random.default_rng(100 + S)
    pat = rng.random((3, 9, 7)) < 0.3
    _run(7, 9, S, 3, lambda k, t, e: bool(pat[k, t, e]), S)


@pytest.mark.parametrize("S", [1, 2, 4, 6])
def test_rule_on_chosen_done_patterns(S):
    """Dones on consecutive steps, two steps apart, at step 0, on the last step (so that the flag crosses after_update), and a
    rollout shorter than the stack."""
    pats = {0: {(0, 0), (0, 1), (0, 2)},          # env 0: three in a row from step 0
            1: {(0, 1), (0, 3)},                  # env 1: two steps apart
            2: {(0, 4), (1, 0)},                  # env 2: last step of a rollout, then step 0 of the next
            3: {(1, 3), (1, 4), (2, 0), (2, 1)},  # env 3: a run across after_update
            4: set()}                             # env 4: never
    _run(5, 5, S, 3, lambda k, t, e: (k, t) in pats[e], 7)
    _run(3, 2, S, 4, lambda k, t, e: (k + t + e) % 3 == 0, 8)  # T < S for S = 4, 6


def test_out_of_range_indices_give_zero_stacks_and_are_counted():
    rng = np.random.default_rng(3)
    n, T, S = 4, 3, 2
    frames = rng.integers(1, 256, (T + S, n, 2, 2)).astype(np.uint8)
    starts = np.zeros((T + S, n), np.uint8)
    got, bad = gather(frames, starts, S, [0, -1, T * n, T * n - 1, 1 << 40])
    assert bad == 3 and not got[1].any() and not got[2].any() and not got[4].any() and got[0].all() and got[3].all()


def test_header_declares_the_gather_and_the_table_binds_it():
    from spacefortress_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "sfmi.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("sf_gather_stacks", "sf_gather_errors"):
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m, name + " is not declared in include/sfmi.h"
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == n_args, name
    for k, v in (("SF_STACK_U8", _lib.STACK_U8), ("SF_STACK_F16", _lib.STACK_F16), ("SF_STACK_F32", _lib.STACK_F32)):
        assert re.search(r"#define\s+%s\s+%d\b" % (k, v), hdr), k


def test_frame_rollout_is_exported():
    import spacefortress_amd

    assert "FrameRollout" in spacefortress_amd.__all__
    fr = spacefortress_amd.FrameRollout
    assert issubclass(fr, spacefortress_amd.DeviceRollout)
    for name in ("reset", "step", "stack_at", "after_update", "feed_forward_generator", "recurrent_generator", "nbytes",
                 "compute_returns"):
        assert callable(getattr(fr, name)), name
    assert callable(spacefortress_amd.DeviceRollout.nbytes)
