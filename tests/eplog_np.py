"""The episode log in numpy (include/sfmi.h: sf_eplog_update), and an independent plain-Python loop over (k, e): what the
kernels of csrc/sf_episode_log.hip are held to, byte for byte (tests/test_gpu_episode_log.py), without a GPU."""
import numpy as np

# sf_episode_record
RECORD = np.dtype([("env", "<i4"), ("episode_return", "<i4"), ("length", "<i4"), ("kills", "<i4"), ("fire_actions", "<i4"),
                   ("reserved", "<i4"), ("end_row", "<i8")])


class NpEpisodeLog:
    """State: acc int32 [n, 4] (return, length, kills, fire actions), ring RECORD [capacity], hist int64 [bins], total,
    rows_seen.  update() is vectorised: a segmented running sum per env and a prefix sum over the flattened `done`."""

    def __init__(self, n, capacity, hist_lo, bins, fire_action=1):
        self.n, self.capacity, self.hist_lo, self.bins, self.fire_action = n, capacity, hist_lo, bins, fire_action
        self.clear()

    def restart(self):
        self.acc = np.zeros((self.n, 4), np.int32)

    def clear(self):
        self.restart()
        self.ring = np.zeros(self.capacity, RECORD)
        self.hist = np.zeros(self.bins, np.int64)
        self.total = 0
        self.rows_seen = 0

    def update(self, rew, done, info, actions=None):
        """One [K, n] update; returns the records it emitted, in sequence order (RECORD array with a parallel `seq`)."""
        rew = np.asarray(rew, np.int64).reshape(-1, self.n)
        done = np.asarray(done).reshape(-1, self.n) != 0
        info = np.asarray(info, np.int64).reshape(-1, self.n)
        K = rew.shape[0]
        fire = (np.asarray(actions).reshape(K, self.n).astype(np.int64) == self.fire_action).astype(np.int64) \
            if actions is not None else np.zeros((K, self.n), np.int64)
        inc = np.stack([rew, np.ones_like(rew), info, fire], -1)  # [K, n, 4]
        # running sums that start over behind every done: cumsum minus the cumsum at the last done in front
        cs = np.cumsum(inc, 0) + self.acc.astype(np.int64)[None]
        at_done = np.where(done[..., None], cs, 0)
        # value of cs at the most recent done strictly before row k (0 if none: the carried accumulators are inside cs)
        last = np.zeros_like(cs)
        run = np.zeros((self.n, 4), np.int64)
        for k in range(K):
            last[k] = run
            run = np.where(done[k][:, None], at_done[k], run)
        seg = cs - last  # the accumulators after row k, before the zeroing of a done
        ks, es = np.nonzero(done)  # row-major order: the rank is the index
        m = len(ks)
        recs = np.zeros(m, RECORD)
        vals = seg[ks, es].astype(np.int32)  # (the device adds in int32: wrap like it)
        recs["env"], recs["episode_return"], recs["length"] = es, vals[:, 0], vals[:, 1]
        recs["kills"], recs["fire_actions"], recs["end_row"] = vals[:, 2], vals[:, 3], self.rows_seen + ks
        seq = self.total + np.arange(m, dtype=np.int64)
        keep = seq >= self.total + m - self.capacity
        self.ring[seq[keep] % self.capacity] = recs[keep]
        np.add.at(self.hist, np.clip(vals[:, 0].astype(np.int64) - self.hist_lo, 0, self.bins - 1), 1)
        self.acc = (cs[-1] - run).astype(np.int32)
        self.total += m
        self.rows_seen += K
        return recs, seq


class LoopEpisodeLog:
    """The same contract written as the sentence reads: for every row, for every env, in order."""

    def __init__(self, n, capacity, hist_lo, bins, fire_action=1):
        self.n, self.capacity, self.hist_lo, self.bins, self.fire_action = n, capacity, hist_lo, bins, fire_action
        self.acc = [[0, 0, 0, 0] for _ in range(n)]
        self.ring = [None] * capacity
        self.hist = [0] * bins
        self.total = 0
        self.rows_seen = 0

    def update(self, rew, done, info, actions=None):
        K = len(rew)
        for k in range(K):
            for e in range(self.n):
                a = self.acc[e]
                a[0] += int(rew[k][e])
                a[1] += 1
                a[2] += int(info[k][e])
                if actions is not None and int(actions[k][e]) == self.fire_action:
                    a[3] += 1
                if done[k][e]:
                    self.ring[self.total % self.capacity] = (e, a[0], a[1], a[2], a[3], 0, self.rows_seen + k)
                    self.hist[min(max(a[0] - self.hist_lo, 0), self.bins - 1)] += 1
                    self.total += 1
                    self.acc[e] = [0, 0, 0, 0]
        self.rows_seen += K

    def ring_array(self):
        out = np.zeros(self.capacity, RECORD)
        for i, r in enumerate(self.ring):
            if r is not None:
                out[i] = r
        return out


def make_rows(rng, K, n, density, act_dtype=np.uint8, n_actions=5):
    """Random rows in the ranges the tests use: rewards in [-40, 40], info in {0, 1}, done with the given density (0 and 1
    exactly none / all)."""
    rew = rng.integers(-40, 41, (K, n)).astype(np.int32)
    done = (rng.random((K, n)) < density).astype(np.uint8) if 0 < density < 1 else np.full((K, n), int(density >= 1), np.uint8)
    info = rng.integers(0, 2, (K, n)).astype(np.uint8)
    act = rng.integers(0, n_actions, (K, n)).astype(act_dtype) if act_dtype is not None else None
    return rew, done, info, act
