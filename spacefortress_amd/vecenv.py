"""SFVecEnv -- the on-device batch that stands in for gym_vecenv.SubprocVecEnv.

The reference runs N `SSF_Env`s in N processes and the trainer talks to them as
one VecEnv (rl/train.py:30-41,60,80-85,179):

    envs.observation_space.shape, envs.action_space
    obs = envs.reset()                        -> [N, ...]
    obs, reward, done, info = envs.step(a)    -> [N, ...], [N], [N], N bools
    envs.close()

SFVecEnv keeps that surface.  The N environments are lanes of one HIP kernel
(libsfmi.so, include/sfmi.h); PyTorch only owns the I/O buffers and the stream.
`step` accepts a CUDA/HIP tensor (returns tensors, nothing leaves the device,
nothing synchronises) or a numpy array / list (returns numpy arrays, like the
reference).  Auto-reset on `done` is the worker loop's: the observation of a
finished lane is the first one of its next episode, reward/done/info belong to
the finished step.

There is no CPU fallback: without a GPU (or without libsfmi.so) construction raises.
"""
import contextlib
import ctypes as C

import numpy as np
import torch

from . import _lib
from .spaces import Box, Discrete

_ACT_TYPES = _lib.act_types()
_NP_FIELD_DTYPES = {(1, 0): np.uint8, (2, 0): np.int16, (4, 0): np.int32, (8, 0): np.int64,
                    (4, 1): np.float32, (8, 1): np.float64}
_UNSIGNED_FIELDS = {"spawn_cursor", "missile_mask", "shell_mask", "flags"}


class SFVecEnv:
    def __init__(self, num_envs, gametype="youturn", obs_type="features", action_set=1, device=None,
                 seed=1, spawn_skip=0, spawn_stride=0, obs_dtype=torch.float32, faithful_bugs=True,
                 auto_reset=True, spawn_table_len=0, reuse_buffers=False, image_geometry=None, ref_reset_obs=False,
                 frame_skip=1):
        if obs_type not in _lib.OBS_TYPES:
            raise AssertionError("obs_type %r" % (obs_type,))  # ENV:51
        # action repeat (sfmi_repeat.h: sf_step_repeat): every step / step_tensors / step_async plays its action for up to
        # frame_skip ticks in one launch; an env that finishes inside the window stops there.  The episode log then counts
        # lengths and fire actions in AGENT steps (one row per window).  1: a tick per step, the calls as they always were.
        # Fixed at construction: with K > 1 the instance's step_tensors IS the repeat (bound below), so that the plain step's
        # host path -- one Python call per launch, barely ahead of a 6 us kernel -- carries no test for it
        self.frame_skip = int(frame_skip)
        if not 1 <= self.frame_skip <= 255:
            raise ValueError("frame_skip must be in [1, 255] (got %r)" % (frame_skip,))
        if self.frame_skip > 1 and not auto_reset:
            raise ValueError("frame_skip > 1 needs auto_reset=True: a finished env of a batch without auto-reset would have to be "
                             "frozen in place for the rest of the window (sfmi_repeat.h)")
        self.last_ticks = None  # uint8 [N]: the ticks every env played in the last step_repeat call
        self._own_ticks = None
        self._final_frames = None
        if self.frame_skip > 1:
            self.step_tensors = self._step_tensors_skip
        self._L = _lib.lib()
        if not torch.cuda.is_available():
            raise _lib.SfmiError("SFVecEnv needs a HIP device (torch.cuda.is_available() is False); "
                                 "there is no CPU fallback")
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if self.device.type != "cuda":
            raise _lib.SfmiError("SFVecEnv runs on the GPU only (got device %s)" % (self.device,))
        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        self.device = torch.device("cuda", dev_index)
        if obs_dtype not in (torch.float32, torch.float64):
            raise ValueError("obs_dtype must be torch.float32 or torch.float64")
        flags = 0
        if obs_dtype == torch.float64:
            flags |= _lib.FLAG_OBS_F64
        if not faithful_bugs:
            flags |= _lib.FLAG_REAL_SHELL_COUNT
        if not auto_reset:
            flags |= _lib.FLAG_NO_AUTO_RESET
        if ref_reset_obs:  # a new game's observation as the reference's wrapper returns it: aim = vdir = ndist = 0 (sfmi.h)
            flags |= _lib.FLAG_REF_RESET_OBS
        p = _lib.CreateParams(gametype.encode(), int(num_envs), dev_index, int(action_set),
                              _lib.OBS_TYPES[obs_type], flags, int(seed) & 0xFFFFFFFF, int(spawn_skip),
                              int(spawn_stride), int(spawn_table_len))
        h = C.c_void_p()
        _lib.check(self._L.sf_create(C.byref(p), C.byref(h)))
        self._h = h
        # what a replay file needs to make this batch again (spacefortress_amd/replay.py)
        self._create = {"action_set": int(action_set), "seed": int(seed) & 0xFFFFFFFF, "spawn_skip": int(spawn_skip),
                        "spawn_stride": int(spawn_stride), "auto_reset": bool(auto_reset)}
        self.default_geometry = True
        self._durations = None
        self._episodes = None
        self._fresh = True  # nothing has changed the state sf_create left: a recording may start here
        self._rec = None
        self.num_envs = int(num_envs)
        self.gametype = gametype
        self.obs_type = obs_type
        self.obs_dtype = obs_dtype
        self.obs_dim = self._L.sf_obs_dim(h)
        # 'image': what the trainer's VecEnv yields, WrapPyTorch's [1, 84, 84] uint8 (rl/envs.py:19-30);
        # 'image-raw': SSF_Env's own [92, 90] grey frame (ENV:171)
        self.is_image = obs_type in ("image", "image-raw")
        self.image_w, self.image_h = _lib.IMAGE_W, _lib.IMAGE_H
        self.obs_shape = {"image": (1, _lib.IMAGE_OUT, _lib.IMAGE_OUT),
                          "image-raw": (self.image_h, self.image_w)}.get(obs_type, (self.obs_dim,))
        self.n_actions = self._L.sf_n_actions(h)
        self.tickdur = self._L.sf_tick_ms(h)      # ENV:61
        self.max_ticks = self._L.sf_max_ticks(h)  # ENV:165
        self.action_space = Discrete(self.n_actions)  # ENV:90
        # ENV:175 declares dtype uint8 for the feature Box; the values are floats
        if self.is_image:
            self.obs_dtype = torch.uint8
            self.observation_space = Box(0, 255, self.obs_shape, np.uint8)  # rl/envs.py:22-26
        else:
            self.observation_space = Box(-np.inf, np.inf, (self.obs_dim,),
                                         np.float32 if obs_dtype == torch.float32 else np.float64)
        self.reuse_buffers = reuse_buffers
        self._bufs = None
        self._buf_ptrs = None
        self._pending = None
        self._fields = None
        # SSF_Env(scale, viewport, ls) (ENV:50-60): the frames' geometry; None = the reference's default (.2, (130, 80, 450, 460), 3)
        if image_geometry is not None:
            try:
                self.set_image_geometry(*image_geometry)
            except Exception:
                self.close()
                raise

    # ------------------------------------------------------------------ buffers
    def _stream(self):
        return _lib.raw_stream(self.device)

    def _alloc(self):
        if self.reuse_buffers and self._bufs is not None:
            return self._bufs
        n = self.num_envs
        # reward, done and info share one allocation (4 n + n + n bytes): the host API brings them over in ONE copy
        rdi = torch.empty(6 * n, dtype=torch.uint8, device=self.device)
        bufs = (torch.empty((n,) + self.obs_shape, dtype=self.obs_dtype, device=self.device),
                rdi[:4 * n].view(torch.int32), rdi[4 * n:5 * n], rdi[5 * n:])
        if self.reuse_buffers:
            self._bufs = bufs
            self._buf_ptrs = tuple(C.c_void_p(t.data_ptr()) for t in bufs)
        return bufs

    # ------------------------------------------------------------------ VecEnv API
    def reset(self, numpy=False):
        """env.reset() in every lane (ENV:163-178): new games; returns obs [N, obs_dim]."""
        obs = self._alloc()[0]
        self._touch()  # (new Games: a recording ends, the duration log's vectors start empty)
        _lib.check(self._L.sf_reset(self._h, C.c_void_p(obs.data_ptr()), self._stream()))
        return obs.cpu().numpy() if numpy else obs

    def _lane_mask(self, lanes, mask):
        """The uint8 [N] device mask of reset_lanes from exactly one of `lanes` (indices) or `mask` (used as it is)."""
        n = self.num_envs
        if (lanes is None) == (mask is None):
            raise ValueError("reset_lanes: give exactly one of `lanes` and `mask`")
        if mask is not None:
            if not (torch.is_tensor(mask) and mask.dtype in (torch.uint8, torch.bool) and mask.device == self.device
                    and mask.dim() == 1 and mask.numel() == n and mask.is_contiguous()):
                raise ValueError("reset_lanes: mask must be a contiguous uint8 or bool tensor [%d] on %s" % (n, self.device))
            return mask.view(torch.uint8) if mask.dtype == torch.bool else mask
        if torch.is_tensor(lanes):
            if lanes.dtype not in (torch.int32, torch.int64):
                raise ValueError("reset_lanes: lanes must be int32 or int64 indices (got %s)" % (lanes.dtype,))
            idx = lanes.reshape(-1).to(self.device, torch.int64)
        else:
            a = np.asarray(lanes)
            if a.size and a.dtype.kind not in "iu":
                raise ValueError("reset_lanes: lanes must be integer indices (got %s)" % (a.dtype,))
            idx = torch.from_numpy(np.ascontiguousarray(a.reshape(-1), np.int64)).to(self.device)
        if idx.numel() and (int(idx.min()) < 0 or int(idx.max()) >= n):  # (synchronises; the mask form does not)
            raise ValueError("reset_lanes: lane index outside [0, %d)" % n)
        m = torch.zeros(n, dtype=torch.uint8, device=self.device)
        m[idx] = 1
        return m

    def reset_lanes(self, lanes=None, mask=None, out=None):
        """env.reset() in the chosen lanes only (ENV:163-178; sfmi.h: sf_reset_lanes): new games there -- the next entry of the
        lane's own spawn stream, prev_vlner kept --, every other lane plays on untouched.  Exactly one of `lanes` (an index
        list or tensor, turned into a mask on the device; checked against the batch, which synchronises) or `mask` (uint8 or
        bool device tensor [N], any non-zero byte; used as it is: nothing synchronises, graph capture works with `out`).
        Returns the observation buffer, `out` or the env's own: for features only the reset rows are written; image batches
        get every lane's frame of its current state.  Not a finished episode: episode_stats() and check_state() do not
        change.  A recording is dropped (RuntimeError) as with reset(), the duration log starts over and an enabled episode
        log starts the reset lanes' running sums over."""
        m = self._lane_mask(lanes, mask)
        if out is None:
            obs = self._alloc()[0]
        else:
            obs = out
            if not (torch.is_tensor(obs) and obs.device == self.device and obs.dtype == self.obs_dtype and obs.is_contiguous()
                    and tuple(obs.shape) == (self.num_envs,) + tuple(self.obs_shape)):
                raise ValueError("reset_lanes: out must be a contiguous %s tensor %s on %s"
                                 % (self.obs_dtype, (self.num_envs,) + tuple(self.obs_shape), self.device))
        self._touch(restart=m)  # (the episode log follows the mask: the other lanes' running sums go on)
        _lib.check(self._L.sf_reset_lanes(self._h, C.c_void_p(m.data_ptr()), C.c_void_p(obs.data_ptr()), self._stream()))
        return obs

    def step_tensors(self, actions, out=None):
        """Device fast path: `actions` is a contiguous uint8/int32/int64 tensor on this device.
        Returns (obs, reward int32, done uint8, info uint8) tensors; nothing synchronises.
        (_act_type, _outputs and _step_into written out: this is the call bench.py times at one Python call per launch, barely
        ahead of a 6 us kernel; the helper form measured no slower on an MI355X, but three more Python frames come out of
        that margin -- profiles/step_paths.md.)"""
        if actions.device != self.device or not actions.is_contiguous() or actions.numel() != self.num_envs:
            raise ValueError("actions must be a contiguous tensor of %d elements on %s" % (self.num_envs, self.device))
        at = _ACT_TYPES.get(actions.dtype)
        if at is None:
            raise TypeError("actions dtype must be uint8, int32 or int64 (got %s)" % (actions.dtype,))
        if out is None and self._bufs is not None and self.reuse_buffers:  # the addresses of the reused outputs, made once
            bufs, ptrs = self._bufs, self._buf_ptrs
        else:
            bufs = out if out is not None else self._alloc()
            ptrs = tuple(C.c_void_p(t.data_ptr()) for t in bufs)
        self._before_step(actions)
        _lib.check(self._L.sf_step(self._h, C.c_void_p(actions.data_ptr()), at, ptrs[0], ptrs[1], ptrs[2], ptrs[3],
                                   self._stream()))
        self._stepped(actions, bufs[1], bufs[2], bufs[3])
        return bufs

    def _step_tensors_skip(self, actions, out=None):
        """step_tensors of a batch made with frame_skip > 1: the action repeated for frame_skip ticks (step_repeat)."""
        return self.step_repeat(actions, self.frame_skip, out=out)

    def _ticks_buffer(self, ticks_out=None):
        """The uint8 [N] tensor a step_repeat call writes the played ticks into: `ticks_out`, or the env's own (made once)."""
        if ticks_out is None:
            if self._own_ticks is None:
                self._own_ticks = torch.zeros(self.num_envs, dtype=torch.uint8, device=self.device)
            return self._own_ticks
        if not (torch.is_tensor(ticks_out) and ticks_out.device == self.device and ticks_out.dtype == torch.uint8
                and ticks_out.is_contiguous() and ticks_out.numel() == self.num_envs):
            raise ValueError("ticks_out must be a contiguous uint8 tensor of %d elements on %s" % (self.num_envs, self.device))
        return ticks_out

    def step_repeat(self, actions, repeat, out=None, ticks_out=None):
        """One agent step that plays `actions` for up to `repeat` ticks in ONE launch (sfmi_repeat.h: sf_step_repeat; image
        batches: and one frame).  Returns (obs, reward, done, info) like `step_tensors`: the observation of the state the window
        leaves (a finished env's: its new game's first one), the int32 sum of the played ticks' rewards, done, the OR of the
        ticks' info.  An env whose game ends inside the window stops there -- its new game is not played on with the old
        action -- and `self.last_ticks` (uint8 [N]; `ticks_out` if given) says how many ticks each env played.  With events
        enabled `self.events` holds the OR of the played ticks' masks.  The episode log gets ONE row per call: lengths and fire
        actions in agent steps.  1 <= repeat <= 255; repeat == 1 is step_tensors.  ValueError on an auto_reset=False batch;
        RuntimeError for repeat > 1 while a duration log is enabled (it follows single ticks) or during a recording (a replay
        file has no field for it)."""
        at = self._act_type(actions)
        bufs, ptrs = self._outputs(out)
        self._step_into(actions, at, ptrs, bufs[1], bufs[2], bufs[3], repeat=int(repeat), ticks_out=ticks_out)
        return bufs

    def step_where(self, actions, active, out=None, ticks_out=None):
        """The masked step (sfmi_hold.h: sf_step_where): the envs whose element of `active` (bool or uint8 device tensor [N],
        any non-zero byte) is set play `actions` for `self.frame_skip` ticks exactly as step_tensors would have them play;
        the others HOLD: not a byte of their state changes (save_lanes rows, counters, spawn stream), they add nothing to
        episode_stats() and do not touch the final-observation buffer.  Returns (obs, reward, done, info) like step_tensors;
        a held env reads reward 0, done 0, info 0, the observation (image batches: the frame) of its unchanged state, event
        word 0, and 0 in `self.last_ticks` (uint8 [N]; `ticks_out` if given), where an active env reads the ticks it played.
        Which envs are held does not change what the active ones do.  Batches made with auto_reset=False are accepted: hold
        the finished envs and they stay at their game over while the others play on.  Nothing synchronises and the host never
        reads the mask; the first call on a batch allocates, later ones can be captured in a graph (with `out`).  ValueError
        for a mask that is not a contiguous bool / uint8 tensor [N] on this device, during a recording (a replay file holds one
        action per env and step) and while a duration log or an episode log is enabled (they count rows, not ticks).  The
        wrappers (FrameStack, SFVecNormalize, DeviceRollout) have no masked form."""
        n = self.num_envs
        if not (torch.is_tensor(active) and active.dtype in (torch.uint8, torch.bool) and active.device == self.device
                and active.dim() == 1 and active.numel() == n and active.is_contiguous()):
            raise ValueError("step_where: active must be a contiguous uint8 or bool tensor [%d] on %s" % (n, self.device))
        if self._final_frames is not None:
            raise ValueError("step_where() while final frames are enabled (enable_final_frames): the masked step has no "
                             "final-frame output yet; enable_final_frames(False) first")
        if self._rec is not None:
            raise ValueError("step_where() during a recording: a replay file holds one action per env and step, and a held "
                             "env plays none")
        if self._durations is not None:
            raise ValueError("step_where() while a duration log is enabled (enable_durations): the log counts rows, not the "
                             "ticks an env played")
        if self._episodes is not None:
            raise ValueError("step_where() while an episode log is enabled (enable_episode_log): the log counts rows, not the "
                             "ticks an env played; filter (reward, done, info) by the mask yourself")
        at = self._act_type(actions)
        bufs, ptrs = self._outputs(out)
        ticks = self._ticks_buffer(ticks_out)
        m = active.view(torch.uint8) if active.dtype == torch.bool else active
        self._touch()
        _lib.check(self._L.sf_step_where(self._h, C.c_void_p(m.data_ptr()), C.c_void_p(actions.data_ptr()), at, self.frame_skip,
                                         ptrs[0], ptrs[1], ptrs[2], ptrs[3], C.c_void_p(ticks.data_ptr()), self._stream()))
        self.last_ticks = ticks
        return bufs

    def _act_type(self, actions, rows=False):
        """THE check of an action tensor in front of a launch: contiguous, on this device, [N] (rows: [K, N]), uint8 / int32 /
        int64.  Returns the C ABI's act type."""
        if rows:
            if actions.device != self.device or not actions.is_contiguous() or actions.dim() != 2 \
                    or actions.shape[1] != self.num_envs:
                raise ValueError("actions must be a contiguous [K, %d] tensor on %s" % (self.num_envs, self.device))
        elif actions.device != self.device or not actions.is_contiguous() or actions.numel() != self.num_envs:
            raise ValueError("actions must be a contiguous tensor of %d elements on %s" % (self.num_envs, self.device))
        at = _ACT_TYPES.get(actions.dtype)
        if at is None:
            raise TypeError("actions dtype must be uint8, int32 or int64 (got %s)" % (actions.dtype,))
        return at

    def _outputs(self, out=None):
        """((obs, reward, done, info), their addresses) of a step: `out`, else the env's own -- reused ones with addresses made
        once (reuse_buffers), or fresh ones."""
        if out is None and self._bufs is not None and self.reuse_buffers:
            return self._bufs, self._buf_ptrs
        bufs = out if out is not None else self._alloc()
        return bufs, tuple(C.c_void_p(t.data_ptr()) for t in bufs)

    def _step_into(self, actions, at, ptrs, rew, done, info, repeat=None, ticks_out=None):
        """THE agent step for callers that own their buffers -- step_repeat and every wrapper (FrameStack, DeviceRollout,
        FrameRollout): checked `actions` of act type `at` (_act_type), `ptrs` the addresses of (obs or None, reward, done,
        info), the three tensors for the hooks.  repeat None: what the batch was made for -- frame_skip == 1 is sf_step
        between _before_step and _stepped, frame_skip > 1 the action repeat.  A repeat given (step_repeat) is always
        sf_step_repeat, which also says the ticks.  No wrapper calls sf_step or sf_step_repeat itself."""
        if repeat is None and self.frame_skip == 1:
            self._before_step(actions)
            _lib.check(self._L.sf_step(self._h, C.c_void_p(actions.data_ptr()), at, ptrs[0], ptrs[1], ptrs[2], ptrs[3],
                                       self._stream()))
        else:
            if repeat is None:
                repeat = self.frame_skip
            if repeat > 1 and self._final_frames is not None:
                raise ValueError("step_repeat() while final frames are enabled (enable_final_frames): an action repeat has no "
                                 "final-frame output yet; enable_final_frames(False) first, or step with repeat 1")
            if repeat != 1:
                self._no_duration_log("step_repeat()")
            if self._rec is not None and repeat > 1:
                raise RuntimeError("step_repeat() during a recording: a replay file has no field for an action repeat")
            ticks = self._ticks_buffer(ticks_out)
            if repeat == 1:
                self._before_step(actions)  # (sf_step itself: a duration log follows it)
            _lib.check(self._L.sf_step_repeat(self._h, C.c_void_p(actions.data_ptr()), at, repeat, ptrs[0], ptrs[1], ptrs[2],
                                              ptrs[3], C.c_void_p(ticks.data_ptr()), self._stream()))
            self.last_ticks = ticks
        self._stepped(actions, rew, done, info)

    def _rollout_outputs(self, K, want_obs):
        """(obs [K, N, ...] or None, reward int32, done uint8, info uint8 [K, N]) of a fused launch"""
        n, dev = self.num_envs, self.device
        return (torch.empty((K, n) + self.obs_shape, dtype=self.obs_dtype, device=dev) if want_obs else None,
                torch.empty((K, n), dtype=torch.int32, device=dev), torch.empty((K, n), dtype=torch.uint8, device=dev),
                torch.empty((K, n), dtype=torch.uint8, device=dev))

    @contextlib.contextmanager
    def _rollout_events(self, K):
        """A fused launch stores one row of event masks PER TICK (a.events[step * n_envs + i], sf_kernels.hip): with
        events enabled it gets a [K, N] buffer of its own for the duration of the launch (`self.rollout_events`);
        `self.events` holds one tick's row and would be overrun by K - 1 rows."""
        ev = None
        if getattr(self, "events", None) is not None:
            ev = torch.zeros((K, self.num_envs), dtype=torch.int32, device=self.device)
            _lib.check(self._L.sf_set_event_output(self._h, C.c_void_p(ev.data_ptr())))
        self.rollout_events = ev
        try:
            yield
        finally:
            if ev is not None:
                _lib.check(self._L.sf_set_event_output(self._h, C.c_void_p(self.events.data_ptr())))

    def rollout(self, actions, out=None, want_obs=True):
        """K steps whose actions are all known up front, fused into one launch (sfmi.h: sf_rollout).
        `actions`: contiguous uint8/int32/int64 tensor [K, N] on this device.  Returns
        (obs [K, N, obs_dim] or None, reward int32 [K, N], done uint8 [K, N], info uint8 [K, N]);
        bit-identical to K `step_tensors` calls.  (An image batch with want_obs gets its frames [K, N, h, w] from K step
        launches each followed by its frames -- the fused launch keeps the state in registers --, in the one call.)"""
        at = self._act_type(actions, rows=True)
        K = actions.shape[0]
        obs, rew, done, info = out if out is not None else self._rollout_outputs(K, want_obs)
        self._no_duration_log("rollout()")
        with self._rollout_events(K):
            _lib.check(self._L.sf_rollout(self._h, C.c_void_p(actions.data_ptr()), at, int(K), _lib.ptr(obs), _lib.ptr(rew),
                                          _lib.ptr(done), _lib.ptr(info), self._stream()))
        self._stepped(actions, rew, done, info)
        return obs, rew, done, info

    # ------------------------------------------------------------------ replay files (spacefortress_amd/replay.py)
    def _before_step(self, actions):
        """THE hook in FRONT of every single-step launch with given actions -- step_tensors, _step_into and the two fused
        launches of the wrappers (DeviceRollout's sf_step_record, SFVecNormalize's sf_step_normalize): the duration log reads the flags,
        timers and vulnerability the tick's key calls meet (durations.py) before the launch changes them."""
        if self._durations is not None:
            self._durations.before(actions)

    def _no_duration_log(self, what):
        """Launches that play several ticks, or actions nobody has seen yet (rollout, the *_sampled calls), give the duration
        log nothing to read between the ticks: refused while one is enabled, rather than leaving its vectors stale."""
        if self._durations is not None:
            raise RuntimeError("%s while a duration log is enabled (enable_durations): the log follows single steps with "
                               "given actions -- step / step_tensors and the wrappers built on them" % what)

    def _stepped(self, actions, rew, done, info):
        """THE hook behind every launch that steps the batch -- step_tensors / _step_into / rollout / the *_sampled calls
        above, and the two fused launches of the wrappers (sf_step_record, sf_step_normalize): the state is
        no longer the one sf_create left, the duration log appends what the tick pushed (and empties the vectors of an env
        whose episode ended), and a recording gets the actions with the engine's own (unnormalised) reward, done and info of
        the step(s): [N] or [K, N] device tensors, not synchronised.  The episode log (enable_episode_log) follows the same rows."""
        self._fresh = False
        if self._durations is not None:
            self._durations.after(done)
        if self._episodes is not None:
            self._episodes.update(rew, done, info, actions)
        if self._rec is not None:
            self._rec.add(actions.to(torch.uint8), rew, done, info)

    def _touch(self, restart=None):
        """The state is about to change otherwise than by a recorded step: a recording cannot go on, and the duration log starts
        over (its vectors belong to the Games the batch held: reset() makes new ones, set_field / load_state_dict put the batch
        somewhere the log has not followed).  The episode log drops its running sums -- of EVERY lane, also when only some were
        loaded (load_lanes / copy_lanes); of the lanes of the mask `restart` when reset_lanes gives one -- and keeps its
        finished records and the histogram."""
        self._fresh = False
        if self._durations is not None:
            self._durations.reset()
        if self._episodes is not None:
            self._episodes.restart() if restart is None else self._episodes.restart_where(restart)
        if self._rec is not None:
            self._rec = None
            if restart is not None:
                raise RuntimeError("reset_lanes() during a recording: a replay file cannot express a manual reset; "
                                   "the recording was dropped")
            raise RuntimeError("reset() / set_field() during a recording: a replay file is the game from a NEW batch on; "
                               "the recording was dropped")

    def start_recording(self):
        """From here on every action played is kept (device tensors, no synchronisation); save_replay() writes them out with
        what they produced.  Only on a batch nothing has stepped or reset since it was made: a replay starts from the state
        sf_create leaves (the reference has no way to put a Game into a given state either)."""
        from .replay import Recorder

        if self.frame_skip > 1:
            raise RuntimeError("start_recording() on a batch with frame_skip > 1: a replay file has no field for an action repeat")
        if not self._fresh:
            raise RuntimeError("start_recording() needs a new batch (nothing stepped, reset or edited since SFVecEnv(...))")
        self._rec = Recorder(self)

    def save_replay(self, path):
        """Write the recording so far (gametype, action set, seed, spawn offsets, build id, uint8 [T, N] actions, per-env
        returns / kills / episode ends, digest of the state now) to `path`; the recording goes on."""
        if self._rec is None:
            raise RuntimeError("save_replay(): no recording (start_recording() on a new batch first)")
        rp = self._rec.replay(self)
        rp.save(path)
        return rp

    @staticmethod
    def load_replay(path):
        """The file as a spacefortress_amd.replay.Replay: `.run()` plays it on the device and verifies it."""
        from .replay import Replay

        return Replay.load(path)

    def seed_actions(self, seed, first_lane=0):
        """Restart the on-device action sampler of `step_sampled` at tick 0 (sfmi.h: sf_seed_actions): lane i then plays
        Philox4x32-10(key = seed, counter = (first_lane + i, tick)) scaled to [0, n_actions).  `first_lane` = this shard's
        first lane in a job of several batches, so that shards draw what the one big batch would."""
        _lib.check(self._L.sf_seed_actions(self._h, int(seed) & 0xFFFFFFFFFFFFFFFF, int(first_lane) & 0xFFFFFFFF, self._stream()))

    def step_sampled(self, out=None, actions_out=None):
        """One step on actions the lanes draw themselves inside the launch (sfmi.h: sf_step_sampled) -- the random-action
        rollout without an action tensor.  Returns (obs, reward, done, info) like `step_tensors`; `actions_out` (uint8 [N]
        on this device, optional) receives what was played."""
        bufs, ptrs = self._outputs(out)
        ao = None
        if actions_out is None and (self._rec is not None or self._episodes is not None):  # a recording / the episode log wants to know what was drawn
            actions_out = torch.empty(self.num_envs, dtype=torch.uint8, device=self.device)
        if actions_out is not None:
            if actions_out.device != self.device or actions_out.dtype != torch.uint8 or not actions_out.is_contiguous() \
                    or actions_out.numel() != self.num_envs:
                raise ValueError("actions_out must be a contiguous uint8 tensor of %d elements on %s" % (self.num_envs, self.device))
            ao = C.c_void_p(actions_out.data_ptr())
        self._no_duration_log("step_sampled()")
        _lib.check(self._L.sf_step_sampled(self._h, ao, ptrs[0], ptrs[1], ptrs[2], ptrs[3], self._stream()))
        self._stepped(actions_out, bufs[1], bufs[2], bufs[3])
        return bufs

    def rollout_sampled(self, n_steps, want_obs=True, want_actions=True):
        """`rollout` on sampled actions: K ticks in one launch.  Returns (obs, reward, done, info, actions uint8 [K, N])."""
        K, n = int(n_steps), self.num_envs
        self._no_duration_log("rollout_sampled()")
        obs, rew, done, info = self._rollout_outputs(K, want_obs)
        acts = torch.empty((K, n), dtype=torch.uint8, device=self.device) if (want_actions or self._rec is not None or self._episodes is not None) else None
        with self._rollout_events(K):
            _lib.check(self._L.sf_rollout_sampled(self._h, K, _lib.ptr(acts), _lib.ptr(obs), _lib.ptr(rew), _lib.ptr(done),
                                                  _lib.ptr(info), self._stream()))
        self._stepped(acts, rew, done, info)
        return obs, rew, done, info, acts

    def step_async(self, actions):
        if torch.is_tensor(actions):
            self._pending = (self.step_tensors(actions), False)
            return
        a = np.asarray(actions)
        if a.shape != (self.num_envs,):
            a = a.reshape(self.num_envs)
        if a.size and (a.min() < 0 or a.max() >= self.n_actions):
            # ENV:211-212: actions_taken[action] / action_combinations[action]
            raise IndexError("action out of range for Discrete(%d)" % self.n_actions)
        t = torch.from_numpy(np.ascontiguousarray(a, np.int64)).to(self.device)
        self._pending = (self.step_tensors(t), True)

    def step_wait(self):
        (obs, rew, done, info), as_numpy = self._pending
        self._pending = None
        if not as_numpy:
            return obs, rew, done.view(torch.bool), info.view(torch.bool)  # 0 / 1 bytes: views, not kernels
        # np.stack of per-env python ints / bools, as the subprocess vec-env returns them
        base, n = done._base, self.num_envs
        if base is not None and info._base is base and base.numel() == 6 * n and rew.data_ptr() == base.data_ptr():
            h = base.cpu().numpy()  # one transfer for the three small results (_alloc)
            return (obs.cpu().numpy(), h[:4 * n].view(np.int32).astype(np.int64), h[4 * n:5 * n].astype(bool),
                    h[5 * n:].astype(bool))
        return (obs.cpu().numpy(), rew.cpu().numpy().astype(np.int64), done.cpu().numpy().astype(bool),
                info.cpu().numpy().astype(bool))

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._L.sf_destroy(self._h)
            self._h = None
        self._final_obs = None
        self._final_frames = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_image_geometry(self, scale=.2, viewport=(130, 80, 450, 460), ls=3):
        """The geometry of this batch's frames, as SSF_Env's constructor takes it (ENV:50-60; sfmi.h: sf_set_image_geometry).
        The default has the fast frame kernel; any other one the general renderer (surface width and height in [84, 251])."""
        vx, vy, vw, vh = (float(v) for v in viewport)
        _lib.check(self._L.sf_set_image_geometry(self._h, float(scale), vx, vy, vw, vh, float(ls)))
        w, h = C.c_int32(), C.c_int32()
        _lib.check(self._L.sf_image_size(self._h, C.byref(w), C.byref(h)))
        self.image_w, self.image_h = int(w.value), int(h.value)
        # (the default geometry's frame kernel also shifts a frame stack in the same launch -- sf_render_shift; the general
        #  renderer draws into one slot: DeviceRollout asks)
        self.default_geometry = bool(self._L.sf_image_geometry_is_default(self._h))  # the library's word, not a second predicate
        if self.obs_type == "image-raw":
            self.obs_shape = (self.image_h, self.image_w)
            self.obs_dim = self._L.sf_obs_dim(self._h)
            self.observation_space = Box(0, 255, self.obs_shape, np.uint8)
            self._bufs = self._buf_ptrs = None

    def set_score_glyphs(self, alpha=None, layout=None, x0=None):
        """The glyph atlas the score text is drawn from in the batch's CURRENT geometry (sfmi.h: sf_set_score_glyphs; how one is
        taken from a box's cairo: tests/golden/frames/make_score_golden.py).  alpha uint8 [11, gh, gw] ('0'..'9', '-'), layout
        (gw, gh, advance, y0), x0 int [11, 10] (or one int).  alpha=None: the seven-segment fallback, by name.  The default
        geometry starts with the built-in atlas (= the reference's frames on this image), any other geometry with none."""
        if alpha is None:
            _lib.check(self._L.sf_set_score_glyphs(self._h, None, None))
            return
        g, a = _lib.score_glyphs(alpha, layout, x0)
        _lib.check(self._L.sf_set_score_glyphs(self._h, C.byref(g), a.ctypes.data_as(C.c_void_p)))

    def score_glyphs(self):
        """The atlas in use: dict(alpha, layout, x0), or None while the seven-segment fallback draws the text."""
        has, g = C.c_int32(), _lib.ScoreGlyphs()
        a = np.zeros(11 * 24 * 24, np.uint8)
        _lib.check(self._L.sf_get_score_glyphs(self._h, C.byref(has), C.byref(g), a.ctypes.data_as(C.c_void_p), a.size))
        if not has.value:
            return None
        return dict(alpha=a[:11 * g.gw * g.gh].reshape(11, g.gh, g.gw).copy(), layout=(g.gw, g.gh, g.advance, g.y0),
                    x0=np.array([[g.x0[i][j] for j in range(10)] for i in range(11)], np.int16))

    def render(self, mode="image-raw", out=None):
        """Frames of the CURRENT state of every env, whatever obs_type the batch steps with (the
        reference's `render()`, ENV:180-198): uint8 [N, 92, 90] ('image-raw') or [N, 1, 84, 84] ('image')."""
        if mode not in ("image", "image-raw"):
            raise ValueError("mode must be 'image' or 'image-raw'")
        shape = (1, _lib.IMAGE_OUT, _lib.IMAGE_OUT) if mode == "image" else (self.image_h, self.image_w)
        if out is None:
            out = torch.empty((self.num_envs,) + shape, dtype=torch.uint8, device=self.device)
        # `out` may be a view whose env stride is larger than a frame (one slot of a frame stack)
        if out.shape != (self.num_envs,) + shape or out.dtype != torch.uint8 or not out[0].is_contiguous():
            raise ValueError("out must be uint8 %s with contiguous frames" % (((self.num_envs,) + shape),))
        stride = out.stride(0) if self.num_envs > 1 else 0
        _lib.check(self._L.sf_render(self._h, _lib.OBS_TYPES[mode], C.c_void_p(out.data_ptr()), stride, self._stream()))
        return out

    def render_view(self, width=-1, height=-1, viewport=(0, 0, -1, -1), lw=2.0, grayscale=False, format="bgrx", lanes=None, out=None,
                    glyphs=None):
        """Frames of the CURRENT state in a VIEW (sfmi.h: sf_render_view): what the reference's Game(config, lw, grayscale, width,
        height, viewport).draw() leaves in pb_pixels, with its defaults (viewport size -1: the config's 710 x 626; width /
        height -1: the viewport's size), up to 1.0 pixel per user unit.  format "bgrx": uint8 [n, H, W, 4] (pb_pixels' bytes),
        "rgb": [n, H, W, 3] (video tools, gym's rgb_array), "gray": [n, H, W] (grey views only).  lanes: None (all), an int or
        a range of consecutive lanes.  glyphs: dict(alpha, layout, x0) as score_glyphs() gives, the atlas of this view; None: the
        built-in one at 1.0 pixel per unit and a whole viewport offset, else the seven-segment fallback.  Reads the state only."""
        if format not in _lib.VIEW_FORMATS:
            raise ValueError("format must be one of %s" % (sorted(_lib.VIEW_FORMATS),))
        if lanes is None:
            first, n = 0, self.num_envs
        elif isinstance(lanes, range):
            if lanes.step != 1 and len(lanes) > 1:
                raise ValueError("lanes must be consecutive")
            first, n = lanes.start, len(lanes)
        else:
            first, n = int(lanes), 1
        v = _lib.View(int(width), int(height), float(viewport[0]), float(viewport[1]), float(viewport[2]), float(viewport[3]), float(lw),
                      1 if grayscale else 0, _lib.VIEW_FORMATS[format])
        keep = None
        if glyphs is not None:
            g, a = _lib.score_glyphs(glyphs["alpha"], glyphs["layout"], glyphs["x0"])
            v.glyphs, v.glyph_alpha, keep = C.pointer(g), a.ctypes.data_as(C.c_void_p), (g, a)
        w, h = C.c_int32(), C.c_int32()
        _lib.check(self._L.sf_view_size(self._h, C.byref(v), C.byref(w), C.byref(h)))  # (the batch's config)
        shape = (h.value, w.value) + ((4,) if format == "bgrx" else (3,) if format == "rgb" else ())
        if out is None:
            out = torch.empty((n,) + shape, dtype=torch.uint8, device=self.device)
        if tuple(out.shape) != (n,) + shape or out.dtype != torch.uint8 or out.device != self.device or (n and not out[0].is_contiguous()):
            raise ValueError("out must be uint8 %s on %s with contiguous frames" % (((n,) + shape), self.device))
        stride = out.stride(0) if n > 1 else 0
        _lib.check(self._L.sf_render_view(self._h, C.byref(v), first, n, C.c_void_p(out.data_ptr()), stride, self._stream()))
        del keep
        return out

    def draw_records(self, from_state=False):
        """Diagnostics: the envs' draw records (sfmi.h: sf_draw_records) as uint8 [N, 432] -- what the frame kernel reads
        instead of the state.  from_state=True rebuilds them from the state first (what a frame does after reset() /
        set_field()); False returns what the last step launch of an image batch left."""
        out = np.empty((self.num_envs, 432), np.uint8)
        _lib.check(self._L.sf_draw_records(self._h, out.ctypes.data_as(C.c_void_p), out.nbytes, int(bool(from_state))))
        return out

    def enable_durations(self, capacity=512):
        """The reference's four telemetry vectors (SRC/game.hh:98-101; getters SRC/pymodule.cpp:143-181) for every env of the
        batch: `thrust_durations`, `shot_durations`, `shot_intervals_invul`, `shot_intervals_vul`, kept on the device by
        `step_tensors` / `step` from here on (durations.py).  Returns the log: `log.get(name)` -> (values [N, capacity],
        counts [N]).  Off by default: four small gathers and a handful of elementwise kernels per step."""
        from .durations import DurationLog
        self._durations = DurationLog(self, capacity)
        return self._durations

    def enable_episode_log(self, capacity=65536, hist=(-256, 512), fire_action=1):
        """One record per finished episode (env, return, length, kills, fire actions, the row it ended on) in a ring of `capacity`,
        and a histogram of the returns (`hist` = (lowest return, bins); the end bins saturate), kept on the device by every
        stepping path from here on (episodes.py; sfmi.h: sf_eplog_*) -- what the trainer's mean / median / min / max line and the
        evaluator's per-episode line are made of (rl/train.py:158-165, rl/evaluate.py:82-99).  Returns the log: `log.drain()`,
        `log.histogram()`, `log.total`.  reset(), set_field() and loaded lanes start the running sums of every lane over;
        finished records stay.  Off by default: three small launches per step."""
        from .episodes import EpisodeLog
        self._episodes = EpisodeLog(self.num_envs, self.device, capacity, hist, fire_action)
        return self._episodes

    def enable_events(self, on=True):
        """Per-tick event bitmasks (sfmi.h SF_EV_*; `_lib.EVENT_NAMES`): after every step `self.events` holds
        uint32 [N] for that tick.  Off by default: it is one more 4-byte store per env and step."""
        self.events = torch.zeros(self.num_envs, dtype=torch.int32, device=self.device) if on else None
        _lib.check(self._L.sf_set_event_output(self._h, C.c_void_p(self.events.data_ptr()) if on else None))
        return self.events

    def enable_final_obs(self, out=None):
        """The LAST observation of every game that ends (sfmi.h: sf_set_final_obs_output): from here on every stepping path
        writes, for each env whose `done` it sets, the row SSF_Env.step returned for that tick -- the one the auto-reset
        replaces with the new game's first observation -- into a [N, obs_dim] tensor of the env's dtype, and leaves the other
        rows alone.  What gymnasium calls `final_observation`: every episode here ends by the clock, so the target at `done`
        bootstraps with V(that row) (DeviceRollout(time_limit_bootstrap=True)).  Allocates a zeroed tensor or adopts `out`,
        returns it (also `self.final_obs`); enable_final_obs(False) switches it off.  Off by default: with it on the step
        leaves the split launch (profiles/final_obs.md).  ValueError for image batches and auto_reset=False."""
        if out is False:
            _lib.check(self._L.sf_set_final_obs_output(self._h, None))
            self._final_obs = None
            return None
        if self.is_image or self.obs_type == "none":
            raise ValueError("enable_final_obs: image batches have no final-observation rows; their finished games' last "
                             "frames come from enable_final_frames()")
        if out is None:
            out = torch.zeros((self.num_envs, self.obs_dim), dtype=self.obs_dtype, device=self.device)
        elif not (torch.is_tensor(out) and out.device == self.device and out.dtype == self.obs_dtype and out.is_contiguous()
                  and tuple(out.shape) == (self.num_envs, self.obs_dim)):
            raise ValueError("enable_final_obs: out must be a contiguous %s tensor [%d, %d] on %s"
                             % (self.obs_dtype, self.num_envs, self.obs_dim, self.device))
        _lib.check(self._L.sf_set_final_obs_output(self._h, C.c_void_p(out.data_ptr())))  # (refuses auto_reset=False, misalignment)
        self._final_obs = out
        return out

    @property
    def final_obs(self):
        """The tensor enable_final_obs() handed to the library, or None."""
        return getattr(self, "_final_obs", None)

    def enable_final_frames(self, out=None):
        """The LAST frame of every game that ends, for image batches (sfmi_final.h: sf_set_final_frame_output): from here on
        step / step_tensors / step_sampled / rollout / rollout_sampled and DeviceRollout's sf_step_record write, for each env
        whose `done` they set, the frame of the finished game after its last tick -- the one the auto-reset replaces with the
        new game's first frame -- into a uint8 tensor [N, 1, 84, 84] ('image') or [N, h, w] ('image-raw', the batch's
        geometry), and leave the other rows alone.  Everything else the step does stays byte for byte what it was.  Allocates
        a zeroed tensor or adopts `out` (frames contiguous; the env stride may be larger: the last slot of a [N, S, 84, 84]
        stack), returns it (also `self.final_frames`); enable_final_frames(False) switches it off.  Off by default: with it on
        a step is the general step launch and three more launches that leave at once unless an env finishes (+16.5 us per step
        at 16 384 envs, +5 us at 256: profiles/final_frames.md).  ValueError for batches without image observations, auto_reset=False, frame_skip > 1 and
        a misaligned buffer; while it is on, step_repeat (repeat > 1) and step_where raise ValueError."""
        if out is False:
            _lib.check(self._L.sf_set_final_frame_output(self._h, None, 0))
            self._final_frames = None
            return None
        if not self.is_image:
            raise ValueError("enable_final_frames: this batch has no image observations; the finished games' last observation "
                             "rows come from enable_final_obs()")
        if self.frame_skip > 1:
            raise ValueError("enable_final_frames: a batch with frame_skip > 1 steps through the action repeat, which has no "
                             "final-frame output yet")
        shape = (self.num_envs,) + tuple(self.obs_shape)
        if out is None:
            out = torch.zeros(shape, dtype=torch.uint8, device=self.device)
        elif not (torch.is_tensor(out) and out.device == self.device and out.dtype == torch.uint8 and tuple(out.shape) == shape
                  and out[0].is_contiguous()):
            raise ValueError("enable_final_frames: out must be a uint8 tensor %s on %s with contiguous frames" % (shape, self.device))
        stride = out.stride(0) if self.num_envs > 1 else 0
        _lib.check(self._L.sf_set_final_frame_output(self._h, C.c_void_p(out.data_ptr()), stride))  # (refuses auto_reset=False, misalignment)
        self._final_frames = out
        return out

    @property
    def final_frames(self):
        """The tensor enable_final_frames() handed to the library, or None."""
        return self._final_frames

    # ------------------------------------------------------------------ extras
    def check_actions(self):
        """Raise IndexError if any action since the last call was out of range (device path)."""
        _lib.check(self._L.sf_check_actions(self._h, self._stream()))

    def check_state(self):
        """Raise OverflowError if a per-episode counter or key timer outgrew its packed width since the last call
        (sfmi.h: sf_check_state): only a batch with auto_reset=False that is stepped for several episodes' worth of
        ticks without reset() can get there; the reference's plain ints keep counting (SRC/game.hh:29-43)."""
        _lib.check(self._L.sf_check_state(self._h, self._stream()))

    def episode_stats(self, clear=False):
        """Device-accumulated episode statistics as an int64 tensor of 8 (see sfmi.h)."""
        out = np.zeros(_lib.EPISODE_STATS_LEN, np.int64)
        _lib.check(self._L.sf_episode_stats(self._h, out.ctypes.data_as(C.c_void_p), int(clear), self._stream()))
        return out

    def field_names(self):
        if self._fields is None:
            self._fields = {}
            d = _lib.FieldDesc()
            for f in range(self._L.sf_n_fields()):
                self._L.sf_field_info(f, C.byref(d))
                name = d.name.decode()
                dt = _NP_FIELD_DTYPES[(d.elem_size, d.is_float)]
                if name in _UNSIGNED_FIELDS:
                    dt = {1: np.uint8, 4: np.uint32}[d.elem_size]
                elif d.elem_size == 1:
                    dt = np.int8
                self._fields[name] = (f, dt, d.count)
        return list(self._fields)

    def get_field(self, name):
        """One state field as numpy: [N] or [count, N] (slot-major)."""
        self.field_names()
        if name not in self._fields:
            raise KeyError(name)
        f, dt, count = self._fields[name]
        arr = np.empty((count, self.num_envs), dt)
        _lib.check(self._L.sf_get_field(self._h, f, arr.ctypes.data_as(C.c_void_p), arr.nbytes))
        return arr[0] if count == 1 else arr

    def get_field_tensor(self, name, out=None):
        """One state field as a DEVICE tensor, [N] or [count, N], without synchronising (sfmi.h: sf_get_field_dev): ordered on
        the current stream behind the steps issued there.  Every field but missile_x / missile_y / missile_angle."""
        self.field_names()
        if name not in self._fields:
            raise KeyError(name)
        f, dt, count = self._fields[name]
        tdt = {np.dtype(np.int32): torch.int32, np.dtype(np.uint32): torch.int32, np.dtype(np.float64): torch.float64,
               np.dtype(np.float32): torch.float32, np.dtype(np.int16): torch.int16, np.dtype(np.uint8): torch.uint8,
               np.dtype(np.int8): torch.int8, np.dtype(np.uint64): torch.int64, np.dtype(np.int64): torch.int64}[np.dtype(dt)]
        if out is None:
            out = torch.empty((count, self.num_envs), dtype=tdt, device=self.device)
        _lib.check(self._L.sf_get_field_dev(self._h, f, C.c_void_p(out.data_ptr()), out.numel() * out.element_size(), self._stream()))
        return out[0] if count == 1 and out.dim() == 2 else out

    def set_field(self, name, value):
        self.field_names()
        if name not in self._fields:
            raise KeyError(name)
        f, dt, count = self._fields[name]
        arr = np.ascontiguousarray(np.asarray(value, dt).reshape(count, self.num_envs))
        self._touch()
        _lib.check(self._L.sf_set_field(self._h, f, arr.ctypes.data_as(C.c_void_p), arr.nbytes))

    def state_dict(self):
        """Every state field (checkpoint / golden replay)."""
        return {n: self.get_field(n) for n in self.field_names()}

    def load_state_dict(self, sd):
        for n in self.field_names():
            self.set_field(n, sd[n])
        # every packed field of every env has just been rewritten with values that fit (set_field range-checks): whatever had
        # wrapped is repaired, the sticky count of check_state() starts over (sfmi.h: sf_clear_state_errors)
        _lib.check(self._L.sf_clear_state_errors(self._h))

    # ------------------------------------------------------------------ lane states (sfmi.h: sf_save_lanes ...)
    def lane_state_header(self):
        """The header a row from this batch carries: numpy uint32 [4] (magic | version, preset, seed, spawn table length)."""
        h = np.zeros(4, np.uint32)
        _lib.check(self._L.sf_lane_state_header(self._h, h.ctypes.data_as(C.c_void_p)))
        return h

    def _index(self, idx, what):
        """(device tensor or None, count, idx type) for a lane / row index argument: None, a device int32 / int64 tensor (kept
        as it is: graph capture), or anything torch.as_tensor takes (copied to the device)."""
        if idx is None:
            return None, None, None
        if not (torch.is_tensor(idx) and idx.device == self.device and idx.dtype in (torch.int32, torch.int64)):
            idx = torch.as_tensor(np.asarray(idx, np.int64).reshape(-1) if not torch.is_tensor(idx) else idx.reshape(-1),
                                  dtype=torch.int64).to(self.device)
        if idx.dim() != 1 or not idx.is_contiguous():
            idx = idx.reshape(-1).contiguous()
        return idx, idx.numel(), (_lib.ACT_I32 if idx.dtype == torch.int32 else _lib.ACT_I64)

    def _obs_arg(self, obs):
        if obs is None:
            return None
        if self.is_image or self.obs_type == "none":
            raise ValueError("obs: image batches draw with render() after a load")
        if not (torch.is_tensor(obs) and obs.device == self.device and obs.dtype == self.obs_dtype and obs.is_contiguous()
                and obs.numel() == self.num_envs * self.obs_dim):
            raise ValueError("obs must be a contiguous %s tensor [%d, %d] on %s" % (self.obs_dtype, self.num_envs, self.obs_dim,
                                                                                   self.device))
        return C.c_void_p(obs.data_ptr())

    def save_lanes(self, lanes=None):
        """The states of `lanes` (None: every lane) as LaneStates: uint8 [n, LANE_STATE_BYTES] on this device, written on the
        current stream without synchronising.  A lane outside the batch gives a row no batch takes (check_lanes reports it)."""
        from .lanes import LaneStates

        idx, n, itype = self._index(lanes, "lanes")
        if idx is None:
            n, itype = self.num_envs, _lib.ACT_I32
        rows = torch.empty((n, _lib.LANE_STATE_BYTES), dtype=torch.uint8, device=self.device)
        _lib.check(self._L.sf_save_lanes(self._h, _lib.ptr(idx), itype, n, C.c_void_p(rows.data_ptr()), self._stream()))
        h = self.lane_state_header()
        return LaneStates(rows, self.gametype, int(h[2]), int(h[3]), _lib.LANE_STATE_VERSION,
                          self._L.sf_build_id().decode())

    def load_lanes(self, states, lanes=None, rows=None, obs=None, check=True):
        """Lane lanes[k] (None: lane k) takes row rows[k] (None: row k) of `states` (LaneStates or a uint8 [n, bytes] tensor on
        this device).  One row into many lanes forks it; a lane named twice takes its LAST row.  obs (symbolic types): the
        [N, obs_dim] buffer that receives the restored lanes' observations -- what the source lane's last step returned.
        check=True synchronises once and raises ValueError if a row was refused (another preset / seed / spawn table, an
        index out of range; those lanes keep their state); check=False stays asynchronous (graph capture) and leaves the
        count to check_lanes().  A recording is dropped (RuntimeError) and the duration log starts over, as with set_field."""
        table = states.rows if hasattr(states, "rows") else states
        if not (torch.is_tensor(table) and table.dtype == torch.uint8 and table.dim() == 2
                and table.shape[1] == _lib.LANE_STATE_BYTES and table.device == self.device and table.is_contiguous()):
            raise ValueError("load_lanes: the rows must be a contiguous uint8 [n, %d] tensor on %s (LaneStates.to(device))"
                             % (_lib.LANE_STATE_BYTES, self.device))
        lidx, n, itype = self._index(lanes, "lanes")
        ridx, nr, rtype = self._index(rows, "rows")
        if lidx is None and ridx is None:
            n, itype = min(self.num_envs, table.shape[0]), _lib.ACT_I32
        elif lidx is None:
            n, itype = nr, rtype
        elif ridx is not None and (nr != n or rtype != itype):
            if nr != n:
                raise ValueError("load_lanes: %d lanes and %d rows" % (n, nr))
            ridx = ridx.to(lidx.dtype)
        optr = self._obs_arg(obs)
        self._touch()
        _lib.check(self._L.sf_load_lanes(self._h, _lib.ptr(lidx), itype, n, C.c_void_p(table.data_ptr()), table.shape[0],
                                         _lib.ptr(ridx), optr, self._stream()))
        if check:
            self.check_lanes()

    def copy_lanes(self, dst_lanes, src_lanes, src=None, obs=None, check=True):
        """Lane dst_lanes[k] of this batch takes the state of lane src_lanes[k] of `src` (None: this batch), as if every source
        were read before any destination is written.  `src` must have this batch's preset, seed and spawn table (ValueError).
        obs / check as in load_lanes."""
        src = self if src is None else src
        d, n, itype = self._index(dst_lanes, "dst_lanes")
        s, ns, stype = src._index(src_lanes, "src_lanes")
        if d is None or s is None:
            raise ValueError("copy_lanes: name the lanes on both sides")
        if ns != n:
            raise ValueError("copy_lanes: %d destination and %d source lanes" % (n, ns))
        if stype != itype:
            s = s.to(d.dtype)
        optr = self._obs_arg(obs)
        self._touch()
        _lib.check(self._L.sf_copy_lanes(self._h, _lib.ptr(d), src._h, _lib.ptr(s), itype, n, optr, self._stream()))
        if check:
            self.check_lanes()

    def check_lanes(self):
        """Raise ValueError if a lane state was refused since the last call (sfmi.h: sf_check_lanes; clears the count)."""
        _lib.check(self._L.sf_check_lanes(self._h, self._stream()))
