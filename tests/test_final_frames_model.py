"""The numpy model of the final stack (tests/finalframes_np.py), pinned by hand-made cases.  No GPU.

A frame is one number here (frame_shape (1,)): the frame of env e after step t is 10 * t + e (t = 0: the reset's), the last frame
of a game that finished in step t is 1000 + 10 * t + e.  Stacks are written out by hand below.
"""
import os
import re

import numpy as np
import pytest

import finalframes_np as FF

FILL = 255


def _frames(t, n):
    return (10 * t + np.arange(n))[:, None].astype(np.int32)


def _run(n, S, dones):
    """dones: [T][n] -> (model, the stacks after every step)"""
    m = FF.FinalStackModel(n, S, (1,), np.int32, FILL)
    m.reset(_frames(0, n))
    seen = []
    for t, d in enumerate(dones, 1):
        seen.append(m.step(np.array(d), 1000 + _frames(t, n), _frames(t, n)).copy())
    return m, seen


def test_s1_is_the_final_frame_alone():
    m, seen = _run(2, 1, [[0, 0], [1, 0], [0, 0]])
    assert m.final[:, 0, 0].tolist() == [1020, FILL]
    assert [s[:, 0, 0].tolist() for s in seen] == [[10, 11], [20, 21], [30, 31]]


def test_s2_a_finish_in_the_first_step_has_zero_history():
    m, seen = _run(2, 2, [[1, 0], [0, 1]])
    # env 0 finishes in step 1: the stack it started from is (0, frame 0) -> final (frame 0, last frame)
    # env 1 finishes in step 2: it started from (frame 1, frame 11) -> (11, 1021)
    assert m.final[:, :, 0].tolist() == [[0, 1010], [11, 1021]]
    assert seen[0][:, :, 0].tolist() == [[0, 10], [1, 11]]       # env 0: zeroed behind the finish, the new game's first frame
    assert seen[1][:, :, 0].tolist() == [[10, 20], [0, 21]]


def test_s4_history_is_the_three_frames_before():
    dones = [[0], [0], [0], [0], [1], [0]]
    m, seen = _run(1, 4, dones)
    assert m.final[0, :, 0].tolist() == [20, 30, 40, 1050]
    assert seen[4][0, :, 0].tolist() == [0, 0, 0, 50] and seen[5][0, :, 0].tolist() == [0, 0, 50, 60]


def test_s4_two_finishes_within_the_stack_keep_the_later_one():
    # finishes in steps 2 and 4: the second final stack's history holds the zeros the first finish left and the new game's frames
    m, seen = _run(1, 4, [[0], [1], [0], [1]])
    assert seen[2][0, :, 0].tolist() == [0, 0, 20, 30]
    assert m.final[0, :, 0].tolist() == [0, 20, 30, 1040]
    m1, _ = _run(1, 4, [[0], [1]])
    assert m1.final[0, :, 0].tolist() == [0, 0, 10, 1020]  # (the reset's zero history, the reset frame, step 1's)


def test_s16_first_step_and_full_history():
    m, _ = _run(1, 16, [[1]])
    assert m.final[0, :, 0].tolist() == [0] * 14 + [0, 1010]
    m, _ = _run(1, 16, [[0]] * 19 + [[1]])
    assert m.final[0, :, 0].tolist() == [10 * t for t in range(5, 20)] + [1200]


@pytest.mark.parametrize("S", [1, 2, 4, 16])
def test_rows_of_envs_that_never_finish_keep_their_bytes(S):
    n = 5
    dones = np.zeros((S + 3, n), np.uint8)
    dones[1, 1] = 1
    dones[S + 1, 3] = 7  # (any non-zero byte)
    m, _ = _run(n, S, dones)
    assert (m.final[[0, 2, 4]] == FILL).all() and (m.final[[1, 3]] != FILL).all()


def test_shift_leaves_the_last_slot_and_the_other_rows():
    prev = np.arange(3 * 4 * 2, dtype=np.int32).reshape(3, 4, 2)
    fin = np.full_like(prev, -1)
    FF.shift(prev, fin, [0, 9, 0])
    assert (fin[[0, 2]] == -1).all() and (fin[1, 3] == -1).all() and np.array_equal(fin[1, :3], prev[1, 1:])
    one = np.full((2, 1, 2), -1, np.int32)
    FF.shift(np.zeros_like(one), one, [1, 1])
    assert (one == -1).all()  # S = 1: nothing is copied


def test_header_declares_what_the_binding_binds():
    from spacefortress_amd import _lib as lib
    from spacefortress_amd import build as sfbuild

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "include", "sfmi_final.h")
    bare = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    assert set(re.findall(r"\b(sf_[a-z_0-9]+)\s*\(", bare)) == set(lib.FINAL_SYMBOLS) == {"sf_set_final_frame_output", "sf_final_stack_shift"}
    for name, (_, args) in lib.FINAL_SYMBOLS.items():
        m = re.search(name + r"\(([^)]*)\)", bare)
        assert m and len(m.group(1).split(",")) == len(args), name
    assert os.path.abspath(path) in [os.path.abspath(h) for h in sfbuild.HEADERS if os.path.isabs(h)]
    assert "sf_final_frames.hip" in sfbuild.SOURCES and "sf_final_capi.cpp" in sfbuild.SOURCES
