"""FrameRollout -- DeviceRollout(env, T, num_stack=S) for image observations with every frame kept ONCE.

The stacked storage holds what the reference holds, the whole stack of every step: observations[T + 1, n, S, 84, 84], although
S - 1 of the S frames of step t + 1 are frames of step t.  Here a FRAME STORE holds, per env, (S - 1) + T + 1 frames -- S - 1
rows of history in front of the rollout's T + 1 -- and one start flag per stored frame (1: first observation of a new game,
i.e. masks[t] == 0).  The stack of (t, e) as the trainer builds it (`current_obs *= masks`, shift, new frame last:
rl/train.py:51-56,92-97) is a function of the store (sfmi.h: sf_gather_stacks):

    slot j of stack(t, e) = frame(t - (S-1) + j, e)  if no frame in (t - (S-1) + j, t] of env e carries a start flag, else 0

A step is sf_step_record without an observation (its done bytes ARE the new row of start flags), sf_render of the new frame once
into store row t + 1, and sf_gather_stacks of the current stack into a reused buffer; minibatches come from one sf_gather_stacks
launch on the sampled indices, as uint8, float16 or float32.  Bytes: (T + S) n 7057 against (T + 1) n 28 224.

The frames lie time-major, [rows][n][7056] (`layout="env"`: [n][rows][7056]; profiles/frame_rollout.md has both measured).
"""
import ctypes as C

import torch

from . import _lib
from ._lib import ptr
from .rollout import DeviceRollout

FRAME = _lib.IMAGE_OUT * _lib.IMAGE_OUT
_OUT_TYPES = {torch.uint8: _lib.STACK_U8, torch.float16: _lib.STACK_F16, torch.float32: _lib.STACK_F32}
_IDX_TYPES = {torch.int32: _lib.ACT_I32, torch.int64: _lib.ACT_I64}


def gather_stacks(frames_ptr, start_ptr, n_envs, rows, num_stack, env_stride, row_stride, index, n_samples, step, out, stream):
    """sf_gather_stacks on raw addresses (`index`: a contiguous int32 / int64 device tensor or None; `out`: a contiguous
    uint8 / float16 / float32 tensor of n_samples stacks)."""
    ot = _OUT_TYPES.get(out.dtype)
    if ot is None:
        raise TypeError("stacks come as uint8, float16 or float32 (got %s)" % (out.dtype,))
    it = 0
    if index is not None:
        it = _IDX_TYPES.get(index.dtype)
        if it is None:
            raise TypeError("indices must be int32 or int64 (got %s)" % (index.dtype,))
        if n_samples == 0:  # (an empty tensor has no address, and a NULL index means "one step")
            return
    _lib.check(_lib.lib().sf_gather_stacks(frames_ptr, start_ptr, n_envs, rows, num_stack, env_stride, row_stride,
                                           ptr(index), it, n_samples, step, ptr(out), ot, stream))


def gather_errors(device, clear=False):
    """Indices outside the rollout's transitions seen by sf_gather_stacks (their stacks are zero); synchronises."""
    n = C.c_uint64(0)
    _lib.lib().sf_gather_errors(C.byref(n), int(bool(clear)), _lib.raw_stream(device))
    return int(n.value)


class FrameRollout(DeviceRollout):
    def __init__(self, env, num_steps, state_size=1, num_stack=4, layout="time", time_limit_bootstrap=False):
        if hasattr(env, "venv"):
            raise ValueError("FrameRollout stores image observations: no SFVecNormalize around the env (rl/train.py:35)")
        if env.obs_type != "image" or not env.default_geometry:
            raise ValueError("FrameRollout is for obs_type='image' batches in the default geometry")
        if not 1 <= int(num_stack) <= 16:
            raise ValueError("1 <= num_stack <= 16")
        if layout not in ("time", "env"):
            raise ValueError("layout is 'time' ([rows][n][7056]) or 'env' ([n][rows][7056])")
        self.layout = layout
        self._S = int(num_stack)
        # (time_limit_bootstrap: DeviceRollout's final stack [n, S, 84, 84]; the stack a step starts from is self._cur)
        super().__init__(env, num_steps, state_size=state_size, num_stack=num_stack, time_limit_bootstrap=time_limit_bootstrap)

    def _alloc_observations(self, shape):
        T, n, S, dev = self.num_steps, self.env.num_envs, self._S, self.env.device
        R = self.rows = T + S  # S - 1 rows of history, then the rollout's T + 1
        if self.layout == "time":
            self.frames = torch.zeros((R, n, FRAME), dtype=torch.uint8, device=dev)
            self._env_stride, self._row_stride = FRAME, n * FRAME
        else:
            self.frames = torch.zeros((n, R, FRAME), dtype=torch.uint8, device=dev)
            self._env_stride, self._row_stride = R * FRAME, FRAME
        self.starts = torch.zeros((R, n), dtype=torch.uint8, device=dev)
        self._cur = torch.zeros((n, S, _lib.IMAGE_OUT, _lib.IMAGE_OUT), dtype=torch.uint8, device=dev)
        self._fp, self._sp = C.c_void_p(self.frames.data_ptr()), C.c_void_p(self.starts.data_ptr())

    def __getattr__(self, name):
        if name == "observations":
            raise AttributeError("FrameRollout keeps every frame once and has no `observations` tensor: "
                                 "stack_at(t) is what observations[t] holds in the stacked storage")
        return super().__getattr__(name)

    def nbytes(self):
        """Bytes of observation storage held on the device: the frames and their start flags."""
        return self.frames.numel() + self.starts.numel()

    def _row(self, r):
        """Store row r as [n, 7056] (row r holds the frame of step r - (S - 1))."""
        return self.frames[r] if self.layout == "time" else self.frames[:, r]

    def _gather(self, index, n_samples, step, out):
        gather_stacks(self._fp, self._sp, self.env.num_envs, self.rows, self._S, self._env_stride, self._row_stride, index,
                      n_samples, step, out, self._stream())
        return out

    def _new(self, m, dtype):
        return torch.empty((m, self._S, _lib.IMAGE_OUT, _lib.IMAGE_OUT), dtype=dtype, device=self.env.device)

    def stack_at(self, t, out=None, dtype=torch.uint8):
        """The stacked observation of step t (0 .. T), [n, S, 84, 84]: observations[t] of the stacked storage."""
        t = int(t)
        if not 0 <= t <= self.num_steps:
            raise IndexError("stack_at(%d): steps are 0 .. %d" % (t, self.num_steps))
        n = self.env.num_envs
        if out is None:
            out = self._new(n, dtype)
        elif out.shape != (n, self._S, _lib.IMAGE_OUT, _lib.IMAGE_OUT) or not out.is_contiguous() or out.device != self.env.device:
            raise ValueError("out must be a contiguous [%d, %d, 84, 84] tensor on %s" % (n, self._S, self.env.device))
        return self._gather(None, n, t, out)

    def stacks(self, index, out=None, dtype=torch.uint8):
        """The stacks of the flat transition indices t * n + e (int32 / int64 device tensor, each in [0, T n)), in ONE launch:
        observations[:-1].view(T n, S, 84, 84)[index] of the stacked storage.  An index out of range gives a zero stack and is
        counted (frame_rollout.gather_errors)."""
        if index.device != self.env.device or index.dim() != 1:
            raise ValueError("index must be a 1-D tensor on %s" % (self.env.device,))
        if not index.is_contiguous():
            index = index.contiguous()
        m = index.numel()
        if out is None:
            out = self._new(m, dtype)
        elif out.shape != (m, self._S, _lib.IMAGE_OUT, _lib.IMAGE_OUT) or not out.is_contiguous() or out.device != self.env.device:
            raise ValueError("out must be a contiguous [%d, %d, 84, 84] tensor on %s" % (m, self._S, self.env.device))
        return self._gather(index, m, 0, out)

    def reset(self):
        """obs = envs.reset(); update_current_obs on a zeroed stack (rl/train.py:43,60-62): history rows zero, start flag set."""
        e, H = self.env, self._S - 1
        e._touch()
        _lib.check(e._L.sf_reset(e._h, None, e._stream()))
        if H:
            self.frames[:H].zero_() if self.layout == "time" else self.frames[:, :H].zero_()
        self.starts[:H].zero_()
        self.starts[H].fill_(1)
        _lib.check(e._L.sf_render(e._h, _lib.OBS_TYPES["image"], C.c_void_p(self._row(H).data_ptr()), self._env_stride,
                                  e._stream()))
        return self._gather(None, e.num_envs, 0, self._cur)

    def _pointers(self):
        T, H = self.num_steps, self._S - 1
        vp = C.c_void_p
        self._ptr = {
            "row": [vp(self._row(H + t).data_ptr()) for t in range(T + 1)],
            "start": [vp(self.starts[H + t].data_ptr()) for t in range(T + 1)],
            "rew": [vp(self.rewards[t].data_ptr()) for t in range(T)],
            "mask": [vp(self.masks[t].data_ptr()) for t in range(T + 1)],
            "act": [vp(self.actions[t].data_ptr()) for t in range(T)],
            "r": vp(self._rew.data_ptr()), "i": vp(self._info.data_ptr()),
            "ep": vp(self.episode_rewards.data_ptr()), "fin": vp(self.final_rewards.data_ptr()),
            "cur": vp(self._cur.data_ptr()),
        }
        self._start_rows = [self.starts[H + t] for t in range(T + 1)]
        # what step() returns: the current stack lives in ONE reused buffer (the next step overwrites it)
        self._views = [(self._cur, self.rewards[t], self.masks[t + 1]) for t in range(T)]

    def _step_record(self, a, ap, at, step, stream):
        e, P = self.env, self._ptr
        # the step's done bytes are the start flags of frame step + 1: the kernel writes them straight into their row
        self._step_and_record(a, ap, at, step, None, self._start_rows[step + 1], P["start"][step + 1], stream)
        self._shift_final_stack(P["cur"], P["start"][step + 1], stream)  # (before the gather below overwrites the stack)
        _lib.check(self._L.sf_render(e._h, _lib.OBS_TYPES["image"], P["row"][step + 1], self._env_stride, stream))
        self._gather(None, e.num_envs, step + 1, self._cur)

    def after_update(self):
        """rl/storage.py:45-48: the last S frames and their flags become rows 0 .. S-1 (history + row 0)."""
        T, S = self.num_steps, self._S
        last = self.frames[T:] if self.layout == "time" else self.frames[:, T:]
        first = self.frames[:S] if self.layout == "time" else self.frames[:, :S]
        flags = self.starts[T:]
        if T < S:  # (source and destination rows overlap)
            last, flags = last.clone(), flags.clone()
        first.copy_(last)
        self.starts[:S].copy_(flags)
        self.states[0].copy_(self.states[-1])
        self.masks[0].copy_(self.masks[-1])

    # ------------------------------------------------------------------ PPO sampling (rl/storage.py:66-122)
    def feed_forward_generator(self, advantages, num_mini_batch, obs_dtype=torch.uint8, perm=None):
        """DeviceRollout's generator (same tuple, shapes and -- after the same torch.manual_seed -- the same sample order);
        the observation minibatch is ONE sf_gather_stacks launch on the permuted indices, as `obs_dtype`."""
        T, n = self.rewards.shape[0:2]
        batch = T * n
        assert batch >= num_mini_batch, "ppo req batch size to be greater than number of mini batches"
        mb = batch // num_mini_batch
        if perm is None:
            perm = torch.randperm(batch, device=self.env.device)
        flat = lambda t: t.reshape(batch, t.shape[-1])
        states, actions, returns, masks = flat(self.states[:-1]), flat(self.actions), flat(self.returns[:-1]), flat(self.masks[:-1])
        logp, adv = flat(self.action_log_probs), advantages.reshape(batch, 1)
        for s in range(0, batch, mb):  # BatchSampler(..., drop_last=False)
            idx = perm[s:s + mb]
            yield self.stacks(idx, dtype=obs_dtype), states[idx], actions[idx], returns[idx], masks[idx], logp[idx], adv[idx]

    def recurrent_generator(self, advantages, num_mini_batch, obs_dtype=torch.uint8, perm=None):
        """Whole trajectories of num_processes // num_mini_batch random envs per minibatch, concatenated env by env: the
        observation indices are ordered env by env, step by step, and gathered in one launch."""
        T, n = self.rewards.shape[0:2]
        per = n // num_mini_batch
        if perm is None:
            perm = torch.randperm(n, device=self.env.device)
        steps = torch.arange(T, device=self.env.device) * n
        cat = lambda t, idx: t[:, idx].transpose(0, 1).reshape(-1, *t.shape[2:])
        for s in range(0, n, per):
            idx = perm[s:s + per]
            flat_idx = (idx[:, None] + steps[None, :]).reshape(-1)
            yield (self.stacks(flat_idx, dtype=obs_dtype), cat(self.states[:-1], idx), cat(self.actions, idx),
                   cat(self.returns[:-1], idx), cat(self.masks[:-1], idx), cat(self.action_log_probs, idx),
                   cat(advantages, idx))
