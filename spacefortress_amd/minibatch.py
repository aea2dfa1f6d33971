"""MiniBatcher -- the PPO update's minibatches on the device (include/sfmi_minibatch.h: sf_minibatch_gather).

The reference samples a minibatch with seven fancy-index launches (rl/storage.py:65-122: observations, states, actions, returns,
masks, old log-probabilities, advantages), each into a freshly allocated tensor, on a slice of the permutation that the host
picks.  Here ONE launch copies all seven columns of a minibatch into FIXED buffers, and the slice is picked by a cursor that
lives on the device and moves on with every launch: the addresses never change and the host decides nothing, so a graph that
captured one `next()` -- or one whole minibatch update, next() -> network -> ppo_loss -> backward -> optimiser -- yields
minibatch 0, 1, 2, ... on successive replays.

    adv = ro.advantages()                                  # sf_advantages: rl/train.py:107-108 in three launches
    mb = ro.batcher(adv, num_mini_batch)                   # buffers, the device permutation, the device cursor
    for _ in range(ppo_epoch):
        mb.shuffle()                                       # torch.randperm on the device, cursor = 0
        for _ in range(mb.n_batches):
            obs, states, actions, returns, masks, old_log_probs, adv_targ = mb.next()

`ro.minibatches(...)` is the same gather as a generator with the reference's tuple, the short last minibatch of
BatchSampler(drop_last=False) included; with the same permutation it equals feed_forward_generator / recurrent_generator bit
for bit.  FrameRollout keeps sf_gather_stacks for its observation: it runs on the row indices the gather wrote (idx_out) and
therefore needs no cursor of its own.  tests/minibatchref.py restates both calls in numpy.
"""
import ctypes as C

import torch

from . import _lib
from ._lib import ptr

_IDX_TYPES = {torch.int32: _lib.ACT_I32, torch.int64: _lib.ACT_I64}
NAMES = ("obs", "states", "actions", "returns", "masks", "old_log_probs", "adv_targ")


def _sources(ro, advantages, obs_dtype):
    """-> ({name: (tensor whose first T n rows are the column, row shape)}, obs dtype, is a FrameRollout).  The observation of
    a FrameRollout is no column: its stacks come from sf_gather_stacks on the gathered row indices."""
    T, n = ro.rewards.shape[0:2]
    dev = ro.env.device
    if not (torch.is_tensor(advantages) and advantages.device == dev and advantages.dtype == torch.float32
            and advantages.is_contiguous() and advantages.numel() == T * n):
        raise ValueError("advantages must be a contiguous float32 tensor of %d elements ([T, n, 1]) on %s" % (T * n, dev))
    frame = hasattr(ro, "frames")
    src = {}
    if frame:
        obs_dtype = torch.uint8 if obs_dtype is None else obs_dtype
        if obs_dtype not in (torch.uint8, torch.float16, torch.float32):
            raise TypeError("stacks come as uint8, float16 or float32 (got %s)" % (obs_dtype,))
    else:
        if obs_dtype is not None and obs_dtype != ro.observations.dtype:
            raise ValueError("obs_dtype %s: this rollout stores its observations as %s and the gather copies bytes"
                             % (obs_dtype, ro.observations.dtype))
        obs_dtype = ro.observations.dtype
        src["obs"] = (ro.observations, tuple(ro.observations.shape[2:]))
    src["states"] = (ro.states, (ro.states.shape[-1],))
    src["actions"] = (ro.actions, (1,))
    src["returns"] = (ro.returns, (1,))
    src["masks"] = (ro.masks, (1,))
    src["old_log_probs"] = (ro.action_log_probs, (1,))
    src["adv_targ"] = (advantages, (1,))
    for name, (t, shape) in src.items():
        rb = t.element_size()
        for s in shape:
            rb *= int(s)
        if not t.is_contiguous() or rb % 4 or not 4 <= rb <= _lib.MB_MAX_ROW_BYTES:
            raise ValueError("minibatch column %s: rows of %d bytes (a multiple of 4 in [4, %d], in a contiguous tensor)"
                             % (name, rb, _lib.MB_MAX_ROW_BYTES))
    return src, obs_dtype, frame


def _alloc(ro, src, rows, obs_dtype, frame):
    """Output tensors of `rows` rows with the reference tuple's shapes and dtypes, and the gathered row indices."""
    dev = ro.env.device
    out = {name: torch.empty((rows,) + shape, dtype=t.dtype, device=dev) for name, (t, shape) in src.items()}
    if frame:
        out["obs"] = torch.empty((rows, ro._S, _lib.IMAGE_OUT, _lib.IMAGE_OUT), dtype=obs_dtype, device=dev)
    out["idx"] = torch.empty(rows, dtype=torch.int64, device=dev)
    return out


def _table(src, out):
    """The sf_mb_column table of a gather from `src` into `out`."""
    tab = (_lib.MbColumn * len(src))()
    for k, (name, (t, shape)) in enumerate(src.items()):
        rb = t.element_size()
        for s in shape:
            rb *= int(s)
        tab[k] = _lib.MbColumn(t.data_ptr(), rb, out[name].data_ptr())
    return tab


def _tuple(out):
    return tuple(out[name] for name in NAMES)


class MiniBatcher:
    """Fixed minibatch buffers over a rollout: `.obs, .states, .actions, .returns, .masks, .old_log_probs, .adv_targ` (also as
    `.tuple`), the device permutation `.index` and the device cursor.  The sources are the rollout's own tensors and the
    `advantages` tensor given here, read at every next(): refill them in place (`ro.advantages(out=adv)`), do not replace them.

    recurrent=False: minibatches of T n / num_mini_batch transitions, `.index` a permutation of the T n transitions.
    recurrent=True: whole trajectories of n / num_mini_batch envs, env by env and step by step, `.index` a permutation of the
    envs.  ValueError where the minibatches would not be equal in size (the generator `minibatches` yields the short one)."""

    def __init__(self, ro, advantages, num_mini_batch, recurrent=False, obs_dtype=None):
        T, n = ro.rewards.shape[0:2]
        nmb = int(num_mini_batch)
        if nmb <= 0:
            raise ValueError("num_mini_batch must be positive")
        self.recurrent = bool(recurrent)
        if self.recurrent:
            if n % nmb:
                raise ValueError("recurrent minibatches of equal size need num_processes (%d) %% num_mini_batch (%d) == 0" % (n, nmb))
            self.n_index, self.rows, self._traj = n, (n // nmb) * T, (T, n)
        else:
            if (T * n) % nmb:
                raise ValueError("minibatches of equal size need T n (%d) %% num_mini_batch (%d) == 0" % (T * n, nmb))
            self.n_index, self.rows, self._traj = T * n, (T * n) // nmb, (0, 0)
        self.n_batches = nmb
        self._ro, self._L, self.device = ro, _lib.lib(), ro.env.device
        self._src, self.obs_dtype, self._frame = _sources(ro, advantages, obs_dtype)
        self._advantages = advantages  # (kept alive: the table holds its address)
        self._out = _alloc(ro, self._src, self.rows, self.obs_dtype, self._frame)
        for name in NAMES:
            setattr(self, name, self._out[name])
        self.idx_out = self._out["idx"]
        self.tuple = _tuple(self._out)
        self.index = torch.arange(self.n_index, dtype=torch.int64, device=self.device)
        self._cursor = torch.zeros(1, dtype=torch.int32, device=self.device)  # uint32 on the device
        self._errors = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._tab = _table(self._src, self._out)
        self._args = (self._tab, len(self._src), T * n, ptr(self.index), _lib.ACT_I64, self.n_index, self.rows, ptr(self._cursor), 0,
                      self.n_batches, self._traj[0], self._traj[1], ptr(self.idx_out), ptr(self._errors))

    def shuffle(self, perm=None):
        """Fill `.index` in place -- torch.randperm on the device, the draw the generators make, unless `perm` is given -- and
        zero the cursor.  Stream work; nothing synchronises."""
        if perm is None:
            torch.randperm(self.n_index, device=self.device, out=self.index)
        else:
            if not torch.is_tensor(perm) or perm.numel() != self.n_index or perm.dim() != 1:
                raise ValueError("perm must be a 1-D tensor of %d indices" % self.n_index)
            self.index.copy_(perm)
        self._cursor.zero_()
        return self

    def next(self):
        """The cursor's minibatch into the fixed buffers -> `.tuple`, and the cursor moves on (wrapping at n_batches): one
        gather launch and the one-thread advance behind it (FrameRollout: then sf_gather_stacks on `.idx_out` into `.obs`).
        Allocates nothing, synchronises nothing, can be captured in a graph."""
        _lib.check(self._L.sf_minibatch_gather(*self._args, _lib.raw_stream(self.device)))
        if self._frame:
            self._ro._gather(self.idx_out, self.rows, 0, self.obs)
        return self.tuple

    def errors(self, clear=False):
        """Rows the gathers wrote as zeros: an index outside the rollout, a cursor beyond n_batches.  Synchronises."""
        bad = int(self._errors.item())
        if clear and bad:
            self._errors.zero_()
        return bad

    def cursor(self):
        """The minibatch the next next() gathers.  Synchronises."""
        return int(self._cursor.item()) & 0xFFFFFFFF

    def set_cursor(self, value):
        """Point the cursor at minibatch `value` (stream work).  A value at or beyond n_batches makes next() write zero rows
        and count them."""
        v = int(value)
        if not 0 <= v < 1 << 32:
            raise ValueError("the cursor is a uint32")
        self._cursor.fill_(v - (1 << 32) if v >= 1 << 31 else v)


def minibatches(ro, advantages, num_mini_batch, recurrent=False, perm=None, reuse=False, obs_dtype=None):
    """feed_forward_generator / recurrent_generator (rl/storage.py:65-122) with ONE gather launch per minibatch (FrameRollout: and
    its sf_gather_stacks): the reference's tuple, the short last minibatch of drop_last=False included (a launch with fewer
    rows); with the same `perm` bit for bit what the generators yield.  reuse=True: every minibatch lands in the same buffers
    (kept on the rollout), so consume one before asking for the next."""
    T, n = ro.rewards.shape[0:2]
    dev = ro.env.device
    nmb = int(num_mini_batch)
    if recurrent:
        total, per_index = n, T
        step = n // nmb if nmb > 0 else 0
        if step <= 0:
            raise ValueError("recurrent minibatches need num_processes (%d) >= num_mini_batch (%d) > 0" % (n, nmb))
        traj = (T, n)
    else:
        total, per_index = T * n, 1
        if nmb <= 0 or total < nmb:
            raise ValueError("ppo req batch size to be greater than number of mini batches")
        step, traj = total // nmb, (0, 0)
    src, obs_dtype, frame = _sources(ro, advantages, obs_dtype)
    if perm is None:
        perm = torch.randperm(total, device=dev)
    if not (torch.is_tensor(perm) and perm.device == dev and perm.dim() == 1 and perm.numel() == total and perm.dtype in _IDX_TYPES):
        raise ValueError("perm must be a 1-D int32 / int64 tensor of %d indices on %s" % (total, dev))
    perm = perm.contiguous()
    it, esz = _IDX_TYPES[perm.dtype], perm.element_size()
    L = _lib.lib()
    full = None
    if reuse:
        cache = ro.__dict__.setdefault("_minibatch_buffers", {})
        key = (step * per_index, bool(recurrent), obs_dtype)
        full = cache.get(key)
        if full is None:
            cache.clear()  # (one set of buffers per rollout)
            full = cache[key] = _alloc(ro, src, step * per_index, obs_dtype, frame)
    for s in range(0, total, step):
        cnt = min(step, total - s)
        rows = cnt * per_index
        if full is None:
            out = _alloc(ro, src, rows, obs_dtype, frame)
        else:
            out = full if rows == step * per_index else {k: v[:rows] for k, v in full.items()}
        _lib.check(L.sf_minibatch_gather(_table(src, out), len(src), T * n, C.c_void_p(perm.data_ptr() + s * esz), it, cnt, rows, None,
                                         0, 1, traj[0], traj[1], ptr(out["idx"]), None, _lib.raw_stream(dev)))
        if frame:
            ro._gather(out["idx"], rows, 0, out["obs"])
        yield _tuple(out)
