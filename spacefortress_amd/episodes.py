"""EpisodeLog -- per-episode records and a histogram of episode returns, kept on the device (sfmi.h: sf_eplog_*).

The trainer logs mean / median / min / max of the episode returns (rl/train.py:158-165) and the evaluator prints one line per
finished episode: return, fortresses destroyed, shots (rl/evaluate.py:82-99).  `sf_episode_stats` keeps eight sums and extremes
per batch, so neither a median nor a single episode can come out of it; without this log a trainer would have to bring `done`
and `reward` to the host at every step to learn them.

The log follows the (reward, done, info, action) rows of every step with three small launches (count, scan, apply:
csrc/sf_episode_log.hip).  At each episode end one 32-byte record -- env, return, length, kills, fire actions, the row it
ended on -- goes into a ring, and the return into a histogram.  Game over is time-only, so a fresh batch finishes all at once:
the order of the ring is a prefix sum over `done` in (step, env) order, the same from run to run.

    log = env.enable_episode_log()          # off by default; SFVecEnv forwards every stepping path to log.update
    ...
    recs = log.drain()                      # synchronises: the records since the last drain, in (step, env) order
    for r, k, s in zip(recs["episode_return"], recs["kills"], recs["fire_actions"]): ...
    stats.summarize(env.episode_stats(), log.histogram(), log.hist_lo)["median_return"]
"""
import ctypes as C

import numpy as np
import torch

from . import _lib

_ACT_TYPES = {torch.uint8: 1, torch.int32: 4, torch.int64: 8}
# sf_episode_record (include/sfmi.h)
RECORD_DTYPE = np.dtype([("env", "<i4"), ("episode_return", "<i4"), ("length", "<i4"), ("kills", "<i4"), ("fire_actions", "<i4"),
                         ("reserved", "<i4"), ("end_row", "<i8")])
assert RECORD_DTYPE.itemsize == _lib.EPISODE_RECORD_BYTES
FIELDS = ("env", "episode_return", "length", "kills", "fire_actions", "end_row")


class EpisodeLog:
    """n_envs running accumulators, a ring of `capacity` records and a histogram of `hist = (lo, bins)`: bin b counts the
    returns lo + b; the two end bins also take everything beyond them.  `fire_action`: the action index counted as a shot
    (rl/evaluate.py:84: `cpu_actions == 1`)."""

    def __init__(self, n_envs, device, capacity=65536, hist=(-256, 512), fire_action=1):
        self._L = _lib.lib()
        self._h = None
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.SfmiError("EpisodeLog lives on the GPU only (got device %s); there is no CPU fallback" % (self.device,))
        idx = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", idx)
        self.n_envs, self.capacity = int(n_envs), int(capacity)
        self.hist_lo, self.bins = int(hist[0]), int(hist[1])
        self.fire_action = int(fire_action)
        h = C.c_void_p()
        _lib.check(self._L.sf_eplog_create(self.n_envs, self.capacity, self.hist_lo, self.bins, self.fire_action, idx, C.byref(h)))
        self._h = h
        self._drained = 0  # sequence number of the first record drain() has not returned yet

    def _stream(self):
        return _lib.raw_stream(self.device)

    def _rows(self, t, dtype, what):
        if t.dtype == torch.bool and dtype == torch.uint8:
            t = t.view(torch.uint8)
        if t.dtype != dtype or t.device != self.device or not t.is_contiguous() or t.dim() not in (1, 2) \
                or t.shape[-1] != self.n_envs:
            raise ValueError("%s must be a contiguous %s tensor [%d] or [K, %d] on %s" % (what, dtype, self.n_envs, self.n_envs,
                                                                                        self.device))
        return t

    def update(self, rew, done, info, actions=None):
        """Follow one step ([N] tensors) or K steps ([K, N]): rew int32, done / info uint8 (or bool), actions uint8 / int32 /
        int64 or None (no shots are counted then).  Stream work on the current stream: nothing synchronises."""
        rew = self._rows(rew, torch.int32, "rew")
        done = self._rows(done, torch.uint8, "done")
        info = self._rows(info, torch.uint8, "info")
        if not (rew.shape == done.shape == info.shape):
            raise ValueError("rew, done and info must have one shape")
        ap, at = None, 0
        if actions is not None:
            at = _ACT_TYPES.get(actions.dtype)
            if at is None:
                raise TypeError("actions dtype must be uint8, int32 or int64 (got %s)" % (actions.dtype,))
            if actions.device != self.device or not actions.is_contiguous() or actions.numel() != rew.numel():
                raise ValueError("actions must be a contiguous tensor of %d elements on %s" % (rew.numel(), self.device))
            ap = C.c_void_p(actions.data_ptr())
        K = rew.shape[0] if rew.dim() == 2 else 1
        if K == 0:
            return
        _lib.check(self._L.sf_eplog_update(self._h, C.c_void_p(rew.data_ptr()), C.c_void_p(done.data_ptr()),
                                           C.c_void_p(info.data_ptr()), ap, at, K, self._stream()))

    def restart(self):
        """Zero the running accumulators: the envs start new games otherwise than by `done` (reset(), edited state, loaded
        lanes).  Finished records and the histogram stay."""
        _lib.check(self._L.sf_eplog_restart(self._h, self._stream()))

    def restart_where(self, mask):
        """`restart` for the envs whose byte of `mask` (uint8 or bool [N] on this device) is not zero: SFVecEnv.reset_lanes.
        The other envs' running sums go on; no record, no histogram count.  Stream work: nothing synchronises."""
        if torch.is_tensor(mask) and mask.dtype == torch.bool:
            mask = mask.view(torch.uint8)
        if not (torch.is_tensor(mask) and mask.dtype == torch.uint8 and mask.device == self.device and mask.dim() == 1
                and mask.numel() == self.n_envs and mask.is_contiguous()):
            raise ValueError("mask must be a contiguous uint8 or bool tensor [%d] on %s" % (self.n_envs, self.device))
        _lib.check(self._L.sf_eplog_restart_where(self._h, C.c_void_p(mask.data_ptr()), self._stream()))

    def clear(self):
        """Zero everything: accumulators, ring, histogram, `total` and the row count."""
        _lib.check(self._L.sf_eplog_clear(self._h, self._stream()))
        self._drained = 0

    def read(self, records=True, histogram=True):
        """(total, rows_seen, ring as stored -- a RECORD_DTYPE array [capacity], slot s % capacity -- or None, histogram int64
        [bins] or None); synchronises the current stream."""
        total, rows = C.c_uint64(), C.c_uint64()
        ring = np.zeros(self.capacity, RECORD_DTYPE) if records else None
        hist = np.zeros(self.bins, np.int64) if histogram else None
        _lib.check(self._L.sf_eplog_read(self._h, C.byref(total), C.byref(rows),
                                         ring.ctypes.data_as(C.c_void_p) if records else None,
                                         hist.ctypes.data_as(C.c_void_p) if histogram else None, self._stream()))
        return int(total.value), int(rows.value), ring, hist

    @property
    def total(self):
        """Episodes ever logged (synchronises)."""
        return self.read(False, False)[0]

    @property
    def rows_seen(self):
        return self.read(False, False)[1]

    def histogram(self):
        """int64 [bins] (synchronises): bin b = episodes whose return was hist_lo + b; the end bins saturate."""
        return self.read(False, True)[3]

    def drain(self):
        """The records not yet drained, in sequence order ((step, env) order), as a dict of numpy arrays `env`,
        `episode_return`, `length`, `kills`, `fire_actions`, `end_row`, `seq`; `dropped`: how many more were logged since the
        last drain but overwritten before they were read (the ring holds the last `capacity`).  Synchronises."""
        total, _, ring, _ = self.read(True, False)
        new = total - self._drained
        have = min(new, self.capacity)
        seq = np.arange(total - have, total, dtype=np.int64)
        recs = ring[seq % self.capacity]
        out = {k: np.ascontiguousarray(recs[k]) for k in FIELDS}
        out["seq"] = seq
        out["dropped"] = int(new - have)
        self._drained = total
        return out

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.sf_eplog_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
