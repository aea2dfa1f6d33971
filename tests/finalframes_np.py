"""TEST INFRASTRUCTURE ONLY -- the numpy statement of the final STACK of an image rollout (include/sfmi_final.h).

The trainer's current stack (rl/train.py:51-56,92-97): `current_obs *= masks` zeroes a finished env's stack, the stack shifts by
one frame, the new frame goes last.  The stack the critic should have seen at a truncation is the one that was never built:
the stack the step STARTED from, shifted by one frame, with the finished game's last frame last -- no zeroing, the game had not
ended when those frames were drawn.  Frames are opaque arrays here; nothing is rendered.
"""
import numpy as np


def shift(prev, final, done):
    """sf_final_stack_shift: for the envs whose done byte is non-zero, slots 1 .. S-1 of prev [n, S, ...] become slots 0 .. S-2
    of final [n, S, ...]; slot S-1 and every other env's row stay.  In place; returns final."""
    assert prev.shape == final.shape and prev.dtype == final.dtype
    d = np.asarray(done).reshape(-1) != 0
    assert d.shape == (prev.shape[0],)
    if prev.shape[1] > 1:
        final[d, :-1] = prev[d, 1:]
    return final


class FinalStackModel:
    """n envs, stacks of S frames of `frame_shape`.  `cur` is the trainer's stack, `final` the final stacks, which start as
    `fill` in every byte (a row that was never written keeps it)."""

    def __init__(self, n, S, frame_shape, dtype=np.uint8, fill=0):
        self.n, self.S = int(n), int(S)
        self.cur = np.zeros((self.n, self.S) + tuple(frame_shape), dtype)
        self.final = np.full_like(self.cur, fill)

    def reset(self, frames):
        """envs.reset() + update_current_obs on a zeroed stack"""
        self.cur[:] = 0
        self.cur[:, -1] = frames
        return self.cur

    def step(self, done, final_frames, new_frames):
        """One env step: `done` [n]; `final_frames` [n, ...]: the finished games' last frames (rows of envs that did not
        finish are not looked at); `new_frames` [n, ...]: the observation the step returned (a finished env's: its new game's
        first frame)."""
        d = np.asarray(done).reshape(-1) != 0
        shift(self.cur, self.final, d)
        self.final[d, -1] = np.asarray(final_frames)[d]
        nxt = np.empty_like(self.cur)
        nxt[:, :-1] = self.cur[:, 1:]
        nxt[d, :-1] = 0
        nxt[:, -1] = new_frames
        self.cur = nxt
        return self.cur
