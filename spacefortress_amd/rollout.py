"""DeviceRollout -- RolloutStorage (rl/storage.py:9-64) plus the trainer's per-step bookkeeping
(rl/train.py:74-98), resident on the device.

The reference moves every step through the host: `action.cpu().numpy()` -> SubprocVecEnv pipes ->
`torch.from_numpy(reward)`, five small tensor ops for the episode bookkeeping, `rollouts.insert(...)`.
Here ONE launch per step (`sf_step_record`) writes the next observation straight into
`observations[step + 1]` and, in the step kernel's own epilogue, `rewards[step]`, `masks[step + 1]`, the
episode / final reward accumulators and `actions[step]`; `compute_returns` is one backward-scan kernel
(`sf_compute_returns`, bit-identical to the reference's float32 arithmetic).  Tensor names and shapes are
RolloutStorage's.

time_limit_bootstrap=True: every episode of this game ends by the clock, so a zero in `masks` is a truncation and the
reference's recursion, which zeroes the value there, is the wrong target.  The rollout then keeps every env's final
observation (SFVecEnv.enable_final_obs), `final_obs()` hands the rows to the critic, and
`compute_returns(..., final_value=critic(ro.final_obs()))` adds gamma * V(final observation) to the reward of the step a
game ended on (`sf_compute_returns_tl`).  One row per env describes one finish: num_steps <= env.max_ticks + 1, the length
of an episode.  A caller who shortens episodes behind the rollout's back -- set_field("time"), load_lanes -- so that an env
finishes twice inside one rollout gets the LATER observation's value for both.

Image envs (num_stack >= 1) bootstrap the same way with the finished game's last STACK: the rollout owns a [N, S, 84, 84] final
stack, points the env's final-frame output (SFVecEnv.enable_final_frames, sfmi_final.h) at its last slot, and after every step
copies the finished envs' history -- slots 1 .. S-1 of the stack the step started from -- in front of it (sf_final_stack_shift).
"""
import ctypes as C

import torch

from . import _lib
from ._lib import ptr


class DeviceRollout:
    def __init__(self, env, num_steps, state_size=1, num_stack=1, time_limit_bootstrap=False):
        # `env`: an SFVecEnv, or an SFVecNormalize around one (the trainer's configuration for 1-D observations,
        # rl/train.py:35-36: observations and rewards reach the storage normalised)
        self.norm = env if hasattr(env, "venv") else None
        env = env.venv if self.norm is not None else env
        self.env = env
        self._L = _lib.lib()
        T, n, dev = int(num_steps), env.num_envs, env.device
        self.num_steps = T
        self.time_limit_bootstrap = bool(time_limit_bootstrap)
        self._final_stack = None
        if self.time_limit_bootstrap:
            if int(num_stack) > 1 and not env.is_image:
                raise ValueError("time_limit_bootstrap with num_stack > 1 is for obs_type='image': 1-D observations are not stacked")
            if env.is_image and self.norm is not None:
                raise ValueError("time_limit_bootstrap on image observations: no SFVecNormalize around the env (rl/train.py:35)")
            if T > env.max_ticks + 1:
                raise ValueError("time_limit_bootstrap: num_steps %d > %d, the ticks of an episode: an env would finish twice "
                                 "in a rollout and one final observation per env cannot describe both" % (T, env.max_ticks + 1))
            if not env.is_image and env.final_obs is None:
                env.enable_final_obs()
        obs_shape = tuple(env.obs_shape)
        # image observations: obs_shape = (obs_shape[0] * num_stack, ...) as in rl/train.py:38-39; every step stores
        # the whole stack (shifted by one frame, zeroed for finished envs, new frame last)
        self.num_stack = int(num_stack)
        if self.num_stack > 1:
            if env.obs_type != "image" or self.norm is not None:
                raise ValueError("num_stack > 1 is for obs_type='image' (rl/train.py:38-39)")
            obs_shape = (self.num_stack,) + obs_shape[1:]
        if self.time_limit_bootstrap and env.is_image:
            # the final stack: the env writes a finished game's last frame straight into its last slot (refuses auto_reset=False,
            # frame_skip > 1), sf_final_stack_shift fills the slots in front of it
            self._final_stack = torch.zeros((n,) + obs_shape, dtype=torch.uint8, device=dev)
            last = self._final_stack[:, self.num_stack - 1:] if env.obs_type == "image" else self._final_stack
            env.enable_final_frames(out=last)
        self._alloc_observations((T + 1, n) + obs_shape)
        self.states = torch.zeros(T + 1, n, state_size, device=dev)
        self.rewards = torch.zeros(T, n, 1, device=dev)
        self.value_preds = torch.zeros(T + 1, n, 1, device=dev)
        self.returns = torch.zeros(T + 1, n, 1, device=dev)
        self.action_log_probs = torch.zeros(T, n, 1, device=dev)
        self.actions = torch.zeros(T, n, 1, dtype=torch.long, device=dev)  # Discrete (rl/storage.py:17-23)
        self.masks = torch.ones(T + 1, n, 1, device=dev)
        self.episode_rewards = torch.zeros(n, 1, device=dev)  # rl/train.py:64-65
        self.final_rewards = torch.zeros(n, 1, device=dev)
        self._kills0 = int(env.episode_stats()[3])
        self._rew = torch.empty(n, dtype=torch.int32, device=dev)
        self._done = torch.empty(n, dtype=torch.uint8, device=dev)
        self._info = torch.empty(n, dtype=torch.uint8, device=dev)
        self._ptr = None
        self.policy = None  # the PolicyHead of step_logits, made on its first call (or by seed_policy)

    def __getattr__(self, name):
        if name == "reset_lanes":  # (not forwarded to the env: see _lib.NO_RESET_LANES)
            raise AttributeError(_lib.NO_RESET_LANES % type(self).__name__)
        raise AttributeError("%r object has no attribute %r" % (type(self).__name__, name))

    def _alloc_observations(self, shape):
        self.observations = torch.zeros(shape, dtype=self.env.obs_dtype, device=self.env.device)

    def nbytes(self):
        """Bytes of observation storage held on the device."""
        return self.observations.numel() * self.observations.element_size()

    def _stream(self):
        return _lib.raw_stream(self.env.device)

    def reset(self):
        """obs = envs.reset(); rollouts.observations[0].copy_(obs) (rl/train.py:60-62)."""
        e = self.env
        e._touch()  # (a recording cannot go on across a reset: vecenv.py)
        if self.num_stack > 1:  # update_current_obs on a zeroed stack (rl/train.py:43,60-62)
            _lib.check(e._L.sf_reset(e._h, None, e._stream()))
            self.observations[0].zero_()
            _lib.check(e._L.sf_render_stack(e._h, ptr(self.observations[0]), self.num_stack, self.num_stack - 1, None,
                                            e._stream()))
            return self.observations[0]
        _lib.check(e._L.sf_reset(e._h, ptr(self.observations[0]), e._stream()))
        if self.norm is not None:
            self.norm._filter(self.observations[0], None)  # VecNormalize.reset: update + normalise in place
        return self.observations[0]

    def _pointers(self):
        """Raw addresses of every per-step slice, made once: the step loop is host-bound otherwise
        (a tensor view and its data_ptr() cost about a microsecond each)."""
        T = self.num_steps
        vp = C.c_void_p
        self._ptr = {
            "obs": [vp(self.observations[t].data_ptr()) for t in range(T + 1)],
            "rew": [vp(self.rewards[t].data_ptr()) for t in range(T)],
            "mask": [vp(self.masks[t].data_ptr()) for t in range(T + 1)],
            "act": [vp(self.actions[t].data_ptr()) for t in range(T)],
            "r": vp(self._rew.data_ptr()), "d": vp(self._done.data_ptr()), "i": vp(self._info.data_ptr()),
            "ep": vp(self.episode_rewards.data_ptr()), "fin": vp(self.final_rewards.data_ptr()),
        }
        # what step() returns, as views made once
        self._views = [(self.observations[t + 1], self.rewards[t], self.masks[t + 1]) for t in range(T)]

    def step(self, step, action, value_pred=None, action_log_prob=None, state=None):
        """envs.step(action) + the bookkeeping + rollouts.insert(...) of rl/train.py:79-98.
        `action`: [N] or [N, 1] integer tensor on the device."""
        e, z = self.env, self.norm
        a = action
        if a.dtype not in (torch.uint8, torch.int32, torch.int64):
            a = a.long()
        if not a.is_contiguous():
            a = a.contiguous()
        at = e._act_type(a)
        if z is not None and not (z.ob and z.ret_on):
            raise NotImplementedError("DeviceRollout drives VecNormalize(ob=True, ret=True), the trainer's configuration")
        if self._ptr is None:
            self._pointers()
        P = self._ptr
        stream = self._stream()
        ap = C.c_void_p(a.data_ptr())
        if z is None:
            self._step_record(a, ap, at, step, stream)
        else:
            # observation and reward through the normaliser (SFVecNormalize._step_into), then the bookkeeping on the normalised
            # reward; the hooks see the engine's own int reward, whatever VecNormalize makes of it
            z._step_into(a, at, self._views[step][0], (P["obs"][step + 1], P["r"], P["d"], P["i"]), self._rew, self._done,
                         self._info)
            self._record(self._L.sf_record_step_f32, ptr(z._rew), P["d"], ap, at, step, stream)
        if value_pred is not None:
            self.value_preds[step].copy_(value_pred)
        if action_log_prob is not None:
            self.action_log_probs[step].copy_(action_log_prob)
        if state is not None:
            self.states[step + 1].copy_(state)
        return self._views[step]

    def _policy_head(self):
        """The rollout's PolicyHead (policy.py), made on first use from the env's n_actions, with what it writes per step: the
        actions [N] uint8 that the step then plays, `policy_entropy` [N], and the rows of action_log_probs."""
        if self.policy is None:
            from .policy import PolicyHead
            e = self.env
            self.policy = PolicyHead(e.num_envs, e.n_actions, device=e.device)
            self._policy_actions = torch.zeros(e.num_envs, dtype=torch.uint8, device=e.device)
            self.policy_entropy = torch.zeros(e.num_envs, device=e.device)
            self._logp_rows = [self.action_log_probs[t] for t in range(self.num_steps)]
        return self.policy

    def seed_policy(self, seed, first_lane=0):
        """Restart the policy head's stream (PolicyHead.seed): `first_lane` is the global index of this rollout's env 0."""
        self._policy_head().seed(seed, first_lane)

    def step_logits(self, step, logits, value_pred=None, state=None, deterministic=False):
        """step() on the policy's logits [N, n_actions] instead of an action: ONE launch (sfmi_policy.h: sf_policy_sample) draws
        every env's action from its row -- deterministic=True: takes the first maximum -- and writes the log-probabilities
        straight into action_log_probs[step]; the rows' entropies are in `self.policy_entropy` [N] until the next call.  Then
        step() with those actions, in every configuration it serves; returns what it returns.  `self.policy` is the head
        (check() counts the rows that held a NaN, a +inf or nothing but -inf; they play action 0)."""
        head = self._policy_head()
        head.sample(logits, deterministic=deterministic, out=(self._policy_actions, self._logp_rows[step], self.policy_entropy))
        return self.step(step, self._policy_actions, value_pred=value_pred, state=state)

    def _record(self, fn, rew, done, ap, at, step, stream):
        """The trainer's float32 bookkeeping as a launch of its own (sf_record_step on the engine's int reward at `rew`,
        sf_record_step_f32 on a normalised one): the same arithmetic on the same values as sf_step_record's epilogue."""
        P = self._ptr
        _lib.check(fn(self.env.num_envs, rew, done, P["rew"][step], P["mask"][step + 1], P["ep"], P["fin"], ap, at, P["act"][step],
                      stream))

    def _step_and_record(self, a, ap, at, step, obs, done, dp, stream):
        """The agent step into `obs` (an address or None) and the done bytes `done` (at `dp`), with the bookkeeping."""
        e, P = self.env, self._ptr
        if e.frame_skip > 1:  # the env's action repeat has no epilogue for the bookkeeping: two launches
            e._step_into(a, at, (obs, P["r"], dp, P["i"]), self._rew, done, self._info)
            self._record(self._L.sf_record_step, P["r"], dp, ap, at, step, stream)
        else:  # one launch: the step kernel's epilogue does the trainer's bookkeeping (sfmi.h: sf_step_record)
            e._before_step(a)
            _lib.check(self._L.sf_step_record(e._h, ap, at, obs, P["r"], dp, P["i"], P["rew"][step], P["mask"][step + 1], P["ep"],
                                              P["fin"], P["act"][step], stream))
            e._stepped(a, self._rew, done, self._info)

    def _advance_stack(self, step, stream):
        """observations[step + 1] from observations[step]: shift by a frame, zero the finished envs, new frame last"""
        e, P = self.env, self._ptr
        if e.default_geometry:  # ONE render launch does all three
            _lib.check(self._L.sf_render_shift(e._h, P["obs"][step], P["obs"][step + 1], self.num_stack, P["d"], stream))
        else:
            # the general renderer (another surface geometry) draws into ONE slot: the shift is a copy here, then the new
            # frame into the last slot with the finished envs' older slots zeroed by the same launch (sf_render_stack)
            self.observations[step + 1][:, :-1].copy_(self.observations[step][:, 1:])
            _lib.check(self._L.sf_render_stack(e._h, P["obs"][step + 1], self.num_stack, self.num_stack - 1, P["d"], stream))

    def _shift_final_stack(self, prev, done, stream):
        """The finished envs' history into the final stack: slots 1 .. S-1 of `prev` (the address of the stack the step started
        from) in front of the final frame the step wrote into the last slot (sfmi_final.h: sf_final_stack_shift)."""
        fs = self._final_stack
        if fs is not None and self.num_stack > 1:
            _lib.check(self._L.sf_final_stack_shift(prev, ptr(fs), self.num_stack, fs[0, 0].numel(), done, self.env.num_envs, stream))

    def _step_record(self, a, ap, at, step, stream):
        P = self._ptr
        if self.num_stack > 1:  # the step without an observation, then the stack
            self._step_and_record(a, ap, at, step, None, self._done, P["d"], stream)
            self._shift_final_stack(P["obs"][step], P["d"], stream)
            self._advance_stack(step, stream)
        else:
            self._step_and_record(a, ap, at, step, P["obs"][step + 1], self._done, P["d"], stream)

    @property
    def num_destruction(self):
        """num_destruction += sum(info) of rl/train.py:81, from the step kernel's own accumulator (synchronises)."""
        return int(self.env.episode_stats()[3]) - self._kills0

    def final_obs(self):
        """[N, obs_dim]: every env's final observation as the agent sees observations -- through the normaliser when there is
        one (a copy, statistics as they stand: SFVecNormalize.final_obs), else the env's own rows; image envs: the rollout's
        final stack [N, S, 84, 84].  For the critic: compute_returns(..., final_value=critic(ro.final_obs()))."""
        if not self.time_limit_bootstrap:
            raise ValueError("final_obs(): this rollout was made without time_limit_bootstrap=True")
        if self._final_stack is not None:
            return self._final_stack
        return self.norm.final_obs() if self.norm is not None else self.env.final_obs

    def compute_returns(self, next_value, use_gae, gamma, tau, final_value=None):
        """rl/storage.py:50-63 in one launch.  final_value ([N] or [N, 1], the critic's value of final_obs()): the recursion
        with gamma * final_value added to the reward of every step whose mask is 0 (sfmi.h: sf_compute_returns_tl); required
        with time_limit_bootstrap=True -- there is no silent fall-back to the recursion that zeroes the value there."""
        n = self.env.num_envs
        nv = next_value.reshape(n).float().contiguous()
        if final_value is None and self.time_limit_bootstrap:
            raise ValueError("compute_returns: this rollout was made with time_limit_bootstrap=True: pass "
                             "final_value=critic(ro.final_obs())")
        if final_value is not None:
            fv = final_value.detach().reshape(n).float().contiguous()
            _lib.check(self._L.sf_compute_returns_tl(self.num_steps, n, ptr(self.rewards), ptr(self.value_preds), ptr(self.masks),
                                                     ptr(nv), ptr(fv), ptr(self.returns), int(bool(use_gae)), float(gamma),
                                                     float(tau), self._stream()))
            return
        _lib.check(self._L.sf_compute_returns(self.num_steps, n, ptr(self.rewards), ptr(self.value_preds), ptr(self.masks),
                                              ptr(nv), ptr(self.returns), int(bool(use_gae)), float(gamma), float(tau),
                                              self._stream()))

    def after_update(self):
        """rl/storage.py:45-48."""
        self.observations[0].copy_(self.observations[-1])
        self.states[0].copy_(self.states[-1])
        self.masks[0].copy_(self.masks[-1])

    # ------------------------------------------------------------------ advantages and minibatches on the device
    def advantages(self, eps=1e-5, out=None):
        """rl/train.py:107-108 -- returns[:-1] - value_preds[:-1], minus its mean, over its unbiased std + eps -- as [T, n, 1]
        float32 in three launches with a fixed arithmetic (sfmi_minibatch.h: sf_advantages; float64 sums in a fixed order: equal
        inputs give equal bits).  `out`: a contiguous float32 tensor of T n elements to fill in place.  `self.advantage_stats`
        holds the mean and the std as two doubles on the device.  Nothing synchronises."""
        T, n = self.rewards.shape[0:2]
        M, dev = T * n, self.env.device
        if out is None:
            out = torch.empty(T, n, 1, dtype=torch.float32, device=dev)
        elif not (torch.is_tensor(out) and out.device == dev and out.dtype == torch.float32 and out.is_contiguous() and out.numel() == M):
            raise ValueError("advantages: out must be a contiguous float32 tensor of %d elements on %s" % (M, dev))
        if self.__dict__.get("advantage_stats") is None:
            self.advantage_stats = torch.zeros(2, dtype=torch.float64, device=dev)
            self._adv_ws = torch.empty(max(1, int(self._L.sf_advantages_workspace_bytes(M)) // 8), dtype=torch.float64, device=dev)
        _lib.check(self._L.sf_advantages(ptr(self.returns), ptr(self.value_preds), M, float(eps), ptr(out), None,
                                         ptr(self.advantage_stats), ptr(self._adv_ws), self._stream()))
        return out.view(T, n, 1)

    def batcher(self, advantages, num_mini_batch, recurrent=False, obs_dtype=None):
        """A MiniBatcher (minibatch.py) over this rollout: fixed minibatch buffers, the permutation and the cursor on the
        device; next() is one gather launch and can be captured in a graph."""
        from .minibatch import MiniBatcher
        return MiniBatcher(self, advantages, num_mini_batch, recurrent=recurrent, obs_dtype=obs_dtype)

    def minibatches(self, advantages, num_mini_batch, recurrent=False, perm=None, reuse=False, obs_dtype=None):
        """feed_forward_generator / recurrent_generator with one gather launch per minibatch (minibatch.py: minibatches): the
        same tuple, with the same `perm` the same bits; reuse=True yields the same buffers every time."""
        from .minibatch import minibatches
        return minibatches(self, advantages, num_mini_batch, recurrent=recurrent, perm=perm, reuse=reuse, obs_dtype=obs_dtype)

    # ------------------------------------------------------------------ PPO sampling (rl/storage.py:66-122)
    def feed_forward_generator(self, advantages, num_mini_batch):
        """Random minibatches over the T x N transitions; same tuple and shapes as the reference's generator."""
        T, n = self.rewards.shape[0:2]
        batch = T * n
        assert batch >= num_mini_batch, "ppo req batch size to be greater than number of mini batches"
        mb = batch // num_mini_batch
        perm = torch.randperm(batch, device=self.env.device)
        obs = self.observations[:-1].reshape(batch, *self.observations.shape[2:])
        flat = lambda t: t.reshape(batch, t.shape[-1])
        states, actions, returns, masks = flat(self.states[:-1]), flat(self.actions), flat(self.returns[:-1]), flat(self.masks[:-1])
        logp, adv = flat(self.action_log_probs), advantages.reshape(batch, 1)
        for s in range(0, batch, mb):  # BatchSampler(..., drop_last=False)
            idx = perm[s:s + mb]
            yield obs[idx], states[idx], actions[idx], returns[idx], masks[idx], logp[idx], adv[idx]

    def recurrent_generator(self, advantages, num_mini_batch):
        """Whole trajectories of num_processes // num_mini_batch random envs per minibatch, concatenated env by env."""
        n = self.rewards.shape[1]
        per = n // num_mini_batch
        perm = torch.randperm(n, device=self.env.device)
        cat = lambda t, idx: t[:, idx].transpose(0, 1).reshape(-1, *t.shape[2:])
        for s in range(0, n, per):
            idx = perm[s:s + per]
            yield (cat(self.observations[:-1], idx), cat(self.states[:-1], idx), cat(self.actions, idx),
                   cat(self.returns[:-1], idx), cat(self.masks[:-1], idx), cat(self.action_log_probs, idx),
                   cat(advantages, idx))
