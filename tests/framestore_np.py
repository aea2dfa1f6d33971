"""The frame store's stack rule in numpy (include/sfmi.h: sf_gather_stacks), and an independent running-stack loop: what the
trainer does to its current observation every step (rl/train.py:51-56,92-97) -- multiply the stack by the mask, shift it
by a frame, put the new frame last.  Test-only; the two are written apart so that one can check the other."""
import numpy as np


def store_rows(T, S):
    return T + S  # S - 1 rows of history, then the rollout's T + 1


def stack_from_store(frames, starts, t, e, S):
    """frames [rows, n, ...] (store row r = the frame of step r - (S - 1)), starts [rows, n] -> stack(t, e) as [S, ...]:
    slot j is store row t + j unless one of the rows t + j + 1 .. t + S - 1 carries a start flag; then it is zero."""
    out = np.zeros((S,) + frames.shape[2:], frames.dtype)
    for j in range(S):
        if not starts[t + j + 1:t + S, e].any():
            out[j] = frames[t + j, e]
    return out


def gather(frames, starts, S, index=None, step=0, T=None):
    """What sf_gather_stacks returns: index = flat transition indices t * n + e (out of [0, T n): a zero stack), or None
    for the n stacks of `step`.  -> (stacks [m, S, ...], number of indices out of range)"""
    rows, n = starts.shape
    T = rows - S if T is None else T
    if index is None:
        return np.stack([stack_from_store(frames, starts, step, e, S) for e in range(n)]), 0
    out = np.zeros((len(index), S) + frames.shape[2:], frames.dtype)
    bad = 0
    for k, i in enumerate(np.asarray(index, np.int64)):
        if 0 <= i < T * n:
            out[k] = stack_from_store(frames, starts, int(i // n), int(i % n), S)
        else:
            bad += 1
    return out, bad


class RunningStack:
    """The trainer's current observation: [n, S, ...], updated once per step."""

    def __init__(self, first_frames, S):
        self.cur = np.zeros((first_frames.shape[0], S) + first_frames.shape[1:], first_frames.dtype)
        self.cur[:, -1] = first_frames

    def step(self, new_frames, done):
        keep = (1 - np.asarray(done, np.uint8)).astype(self.cur.dtype)
        self.cur = self.cur * keep.reshape((-1,) + (1,) * (self.cur.ndim - 1))  # current_obs *= masks
        self.cur[:, :-1] = self.cur[:, 1:].copy()                                # shift by a frame
        self.cur[:, -1] = new_frames                                            # the new frame last
        return self.cur


class NpFrameStore:
    """FrameRollout's bookkeeping on the host: reset / step / after_update on a [rows, n, ...] store."""

    def __init__(self, n, T, S, frame_shape, dtype=np.uint8):
        self.n, self.T, self.S = n, T, S
        self.frames = np.zeros((store_rows(T, S), n) + tuple(frame_shape), dtype)
        self.starts = np.zeros((store_rows(T, S), n), np.uint8)

    def reset(self, first_frames):
        H = self.S - 1
        self.frames[:H] = 0
        self.starts[:H] = 0
        self.frames[H] = first_frames
        self.starts[H] = 1

    def step(self, t, new_frames, done):
        self.frames[self.S + t] = new_frames  # frame t + 1 -> row t + 1 + (S - 1)
        self.starts[self.S + t] = np.asarray(done, np.uint8)

    def after_update(self):
        self.frames[:self.S] = self.frames[self.T:].copy()
        self.starts[:self.S] = self.starts[self.T:].copy()

    def stack_at(self, t):
        return gather(self.frames, self.starts, self.S, None, t)[0]
