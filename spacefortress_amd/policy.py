"""PolicyHead -- the step between the network and the env, on the device (include/sfmi_policy.h: sf_policy_sample).

The reference's trainer turns logits into an action with softmax, log_softmax, multinomial(1) or max(1)[1], and gather
(rl/networks.py:65-76) and takes the result through the host (rl/train.py:79); a loop on torch.distributions.Categorical does
the same in about ten small launches.  Here ONE launch over the [N, A] logits writes the actions, the log-probabilities PPO
stores and the entropies the trainer logs.  The draws come from a Philox4x32-10 stream of the head's own -- key = seed, counter
= (first_lane + env, tick, 0x504F4C, 0), a tick per 64 envs kept on the device -- so a captured graph draws new actions at every
replay, and a shard that passes its first env's global index as `first_lane` draws what the whole batch draws for its envs.

The semantics, operation by operation, are in the header; tests/policyref.py restates them in numpy.  The outputs are not
differentiable: the PPO update evaluates its actions with torch as before (DESIGN 8d names the follow-up).
"""
import ctypes as C

import torch

from . import _lib
from ._lib import ptr

_ACT_TYPES = _lib.act_types()


class PolicyHead:
    def __init__(self, n_envs, n_actions, seed=0, first_lane=0, device="cuda"):
        n, A = int(n_envs), int(n_actions)
        if n <= 0:
            raise ValueError("PolicyHead: n_envs must be positive")
        if not 1 <= A <= _lib.POLICY_MAX_ACTIONS:
            raise ValueError("PolicyHead: n_actions %d outside [1, %d]" % (A, _lib.POLICY_MAX_ACTIONS))
        self.n_envs, self.n_actions = n, A
        self.device = torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._L = _lib.lib()
        self.ticks = torch.zeros((n + 63) // 64, dtype=torch.int32, device=self.device)  # uint32 on the device: one per wave
        self.bad_rows = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._tp, self._bp = C.c_void_p(self.ticks.data_ptr()), C.c_void_p(self.bad_rows.data_ptr())
        self._seed, self.first_lane = 0, 0
        self.seed(seed, first_lane)

    def seed(self, seed, first_lane=0):
        """Restart the stream: key `seed` (64 bits), this shard's first global env `first_lane` (32 bits), every tick 0."""
        seed, first_lane = int(seed), int(first_lane)
        if not 0 <= seed < 1 << 64 or not 0 <= first_lane < 1 << 32:
            raise ValueError("PolicyHead.seed: seed is 64 bits, first_lane 32 bits, both unsigned")
        self._seed, self.first_lane = seed, first_lane
        self.ticks.zero_()

    def _logits(self, logits):
        n, A = self.n_envs, self.n_actions
        if not torch.is_tensor(logits) or logits.device != self.device or logits.dim() != 2 or tuple(logits.shape) != (n, A):
            raise ValueError("PolicyHead: logits must be a [%d, %d] tensor on %s" % (n, A, self.device))
        if logits.dtype != torch.float32:
            logits = logits.float()
        if logits.stride(1) != 1 or (n > 1 and logits.stride(0) < A):
            logits = logits.contiguous()
        return logits, (logits.stride(0) if n > 1 else A)

    def _out(self, t, dtypes, what):
        if not (torch.is_tensor(t) and t.device == self.device and t.dtype in dtypes and t.is_contiguous()
                and t.numel() == self.n_envs):
            raise ValueError("PolicyHead: out %s must be a contiguous tensor of %d elements on %s, dtype %s"
                             % (what, self.n_envs, self.device, " / ".join(str(d) for d in dtypes)))
        return t

    def sample(self, logits, deterministic=False, out=None):
        """(actions [N, 1], log_probs [N, 1] float32, entropy [N] float32) of `logits` [N, A] in ONE launch; nothing
        synchronises.  deterministic=True plays the first index of the maximum and leaves the ticks alone.

        float32 logits whose rows are dense (any row stride) pass through untouched; anything else is `.float()`-ed (and made
        contiguous) first, which costs a launch.  `out` = (actions, log_probs, entropy): contiguous tensors of N elements on
        this device -- actions uint8, int32 or int64 (int64 when made here, like Categorical.sample), the other two float32 or
        None for an output nobody needs (None comes back in its place).  They are written in place and returned as views of
        the shapes above.  A row with a NaN, a +inf or nothing but -inf plays action 0, reads NaN in both outputs and is
        counted: check()."""
        x, stride = self._logits(logits)
        n = self.n_envs
        if out is None:
            act = torch.empty(n, dtype=torch.int64, device=self.device)
            logp = torch.empty(n, dtype=torch.float32, device=self.device)
            ent = torch.empty(n, dtype=torch.float32, device=self.device)
        else:
            act, logp, ent = out
            self._out(act, tuple(_ACT_TYPES), "actions")
            if logp is not None:
                self._out(logp, (torch.float32,), "log_probs")
            if ent is not None:
                self._out(ent, (torch.float32,), "entropy")
        mode = _lib.POLICY_ARGMAX if deterministic else _lib.POLICY_SAMPLE
        _lib.check(self._L.sf_policy_sample(C.c_void_p(x.data_ptr()), n, self.n_actions, stride, mode, self._seed, self.first_lane,
                                            self._tp, C.c_void_p(act.data_ptr()), _ACT_TYPES[act.dtype], ptr(logp), ptr(ent),
                                            self._bp, _lib.raw_stream(self.device)))
        return act.view(n, 1), (logp.view(n, 1) if logp is not None else None), (ent.view(n) if ent is not None else None)

    def check(self):
        """The number of bad rows (a NaN, a +inf, nothing but -inf) seen since the last check(); clears it.  Synchronises."""
        bad = int(self.bad_rows.item())
        if bad:
            self.bad_rows.zero_()
        return bad

    def state_dict(self):
        """The stream's position: seed, first_lane and every wave's tick (synchronises)."""
        return {"seed": self._seed, "first_lane": self.first_lane, "ticks": self.ticks.cpu().numpy().view("uint32").copy()}

    def load_state_dict(self, sd):
        import numpy as np

        ticks = np.ascontiguousarray(sd["ticks"], dtype=np.uint32)
        if ticks.shape != (self.ticks.numel(),):
            raise ValueError("PolicyHead.load_state_dict: %d ticks for a head of %d envs (%d waves)"
                             % (ticks.size, self.n_envs, self.ticks.numel()))
        self.seed(sd["seed"], sd["first_lane"])
        self.ticks.copy_(torch.from_numpy(ticks.view(np.int32)))
