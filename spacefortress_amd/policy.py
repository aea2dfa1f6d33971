"""PolicyHead -- the step between the network and the env, on the device (include/sfmi_policy.h: sf_policy_sample).

The reference's trainer turns logits into an action with softmax, log_softmax, multinomial(1) or max(1)[1], and gather
(rl/networks.py:65-76) and takes the result through the host (rl/train.py:79); a loop on torch.distributions.Categorical does
the same in about ten small launches.  Here ONE launch over the [N, A] logits writes the actions, the log-probabilities PPO
stores and the entropies the trainer logs.  The draws come from a Philox4x32-10 stream of the head's own -- key = seed, counter
= (first_lane + env, tick, 0x504F4C, 0), a tick per 64 envs kept on the device -- so a captured graph draws new actions at every
replay, and a shard that passes its first env's global index as `first_lane` draws what the whole batch draws for its envs.

The semantics, operation by operation, are in the header; tests/policyref.py restates them in numpy.  The outputs of
PolicyHead.sample are not differentiable: the PPO update evaluates its actions with the two functions below.

evaluate_actions / ppo_loss -- the update side (include/sfmi_ppo.h).  Where the reference's update runs softmax, log_softmax,
gather and the entropy (rl/networks.py:78-86), then exp, two products, clamp, min, three means and the weighted sum
(rl/train.py:123-129), and autograd walks back through all of it, these are torch.autograd.Functions over one launch each way
(the loss's forward: two).  They use the sampling head's arithmetic: the log-probability a rollout stored through
PolicyHead.sample and the one the first update recomputes from the same logits are the same bits, so the first ratio is 1.
tests/policyevalref.py restates them in numpy.
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


# ---------------------------------------------------------------------------------------------------------------
# the update side: include/sfmi_ppo.h
_EVAL_STATE = {}  # device -> {"bad": int64 [1], "ws": {M: float64 workspace of sf_ppo_loss}}


def _eval_state(device):
    st = _EVAL_STATE.get(device)
    if st is None:
        st = _EVAL_STATE[device] = {"bad": torch.zeros(1, dtype=torch.int64, device=device), "ws": {}}
    return st


def _workspace(device, M):
    """sf_ppo_loss's partial sums: allocated once per (device, M).  Calls that share it must be ordered on one stream."""
    ws = _eval_state(device)["ws"]
    w = ws.get(M)
    if w is None:
        w = ws[M] = torch.empty(max(1, int(_lib.lib().sf_ppo_loss_workspace_bytes(M)) // 8), dtype=torch.float64, device=device)
    return w


def check(device=None):
    """The number of bad rows (a NaN, a +inf, nothing but -inf, an action outside the set) evaluate_actions and ppo_loss have
    seen on `device` (default: the current one) since the last check(); clears it.  Synchronises.  Also reachable as
    evaluate_actions.check / ppo_loss.check."""
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    st = _EVAL_STATE.get(device)
    if st is None:
        return 0
    bad = int(st["bad"].item())
    if bad:
        st["bad"].zero_()
    return bad


def _eval_logits(logits, who):
    """[M, A] logits -> (float32 tensor with dense rows, row stride, M, A): PolicyHead._logits without a fixed shape"""
    if not torch.is_tensor(logits) or logits.dim() != 2 or logits.device.type != "cuda":
        raise ValueError("%s: logits must be a [M, A] tensor on the GPU" % who)
    M, A = logits.shape
    if M <= 0 or not 1 <= A <= _lib.POLICY_MAX_ACTIONS:
        raise ValueError("%s: logits [%d, %d]: need at least one row and 1 .. %d actions" % (who, M, A, _lib.POLICY_MAX_ACTIONS))
    x = logits.detach()
    if x.dtype != torch.float32:
        x = x.float()
    if x.stride(1) != 1 or (M > 1 and x.stride(0) < A):
        x = x.contiguous()
    return x, (x.stride(0) if M > 1 else A), M, A


def _eval_actions(actions, M, device, who):
    if not torch.is_tensor(actions) or actions.device != device or actions.dtype not in _ACT_TYPES or actions.numel() != M:
        raise ValueError("%s: actions must be a uint8 / int32 / int64 tensor of %d elements ([M, 1] or [M]) on %s" % (who, M, device))
    return actions.detach().contiguous().view(-1)


def _eval_column(t, M, device, what, who):
    """[M, 1] or [M] -> a dense float32 [M]"""
    if not torch.is_tensor(t) or t.device != device or t.numel() != M:
        raise ValueError("%s: %s must be a tensor of %d elements ([M, 1] or [M]) on %s" % (who, what, M, device))
    t = t.detach()
    if t.dtype != torch.float32:
        t = t.float()
    return t.contiguous().view(-1)


class _EvaluateActions(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, actions):
        who = "evaluate_actions"
        x, stride, M, A = _eval_logits(logits, who)
        a = _eval_actions(actions, M, x.device, who)
        logp = torch.empty(M, dtype=torch.float32, device=x.device)
        ent = torch.empty(M, dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().sf_policy_evaluate(ptr(x), M, A, stride, ptr(a), _ACT_TYPES[a.dtype], ptr(logp), ptr(ent),
                                                ptr(_eval_state(x.device)["bad"]), _lib.raw_stream(x.device)))
        ctx.save_for_backward(x, a)
        ctx.stride, ctx.logits_dtype = stride, logits.dtype
        ctx.set_materialize_grads(False)
        return logp.view(M, 1), ent

    @staticmethod
    def backward(ctx, g_logp, g_ent):
        x, a = ctx.saved_tensors
        M, A = x.shape
        g_logp = None if g_logp is None else _eval_column(g_logp, M, x.device, "the gradient of log_probs", "evaluate_actions")
        g_ent = None if g_ent is None else _eval_column(g_ent, M, x.device, "the gradient of entropy", "evaluate_actions")
        grad = torch.empty(M, A, dtype=torch.float32, device=x.device)
        _lib.check(_lib.lib().sf_policy_evaluate_backward(ptr(x), M, A, ctx.stride, ptr(a), _ACT_TYPES[a.dtype], ptr(g_logp), ptr(g_ent),
                                                         ptr(grad), A, _lib.raw_stream(x.device)))
        return (grad if ctx.logits_dtype == torch.float32 else grad.to(ctx.logits_dtype)), None


class _PPOLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, values, actions, old_log_probs, adv_targ, returns, clip_param, value_loss_coeff, entropy_coeff):
        who = "ppo_loss"
        x, stride, M, A = _eval_logits(logits, who)
        dev = x.device
        a = _eval_actions(actions, M, dev, who)
        v = _eval_column(values, M, dev, "values", who)
        old = _eval_column(old_log_probs, M, dev, "old_log_probs", who)
        adv = _eval_column(adv_targ, M, dev, "adv_targ", who)
        ret = _eval_column(returns, M, dev, "returns", who)
        # float32(1 - clip), float32(1 + clip), rounded from the double: what torch.clamp makes of a Python scalar
        coef = (C.c_float(1.0 - float(clip_param)), C.c_float(1.0 + float(clip_param)), C.c_float(float(value_loss_coeff)),
                C.c_float(float(entropy_coeff)))
        sums = torch.empty(4, dtype=torch.float32, device=dev)
        _lib.check(_lib.lib().sf_ppo_loss(ptr(x), ptr(v), ptr(a), ptr(old), ptr(adv), ptr(ret), M, A, stride, _ACT_TYPES[a.dtype], *coef,
                                         None, ptr(sums), ptr(_workspace(dev, M)), ptr(_eval_state(dev)["bad"]), _lib.raw_stream(dev)))
        ctx.save_for_backward(x, v, a, old, adv, ret)
        ctx.stride, ctx.coef, ctx.values_like = stride, coef, (values.shape, values.dtype)
        ctx.logits_dtype = logits.dtype
        loss, action_loss, value_loss, entropy = sums[3], sums[0], sums[1], sums[2]
        ctx.mark_non_differentiable(action_loss, value_loss, entropy)
        ctx.set_materialize_grads(False)  # (no zero tensors made for the three on the way back)
        return loss, action_loss, value_loss, entropy

    @staticmethod
    def backward(ctx, g, *_unused):
        if g is None:
            return (None,) * 9
        x, v, a, old, adv, ret = ctx.saved_tensors
        M, A = x.shape
        dev = x.device
        g = g.detach()
        if g.dtype != torch.float32:
            g = g.float()
        g = g.contiguous()
        grad = torch.empty(M, A, dtype=torch.float32, device=dev)
        gv = torch.empty(M, dtype=torch.float32, device=dev) if ctx.needs_input_grad[1] else None
        _lib.check(_lib.lib().sf_ppo_loss_backward(ptr(x), ptr(v), ptr(a), ptr(old), ptr(adv), ptr(ret), M, A, ctx.stride,
                                                  _ACT_TYPES[a.dtype], *ctx.coef, ptr(g), ptr(grad), A, ptr(gv), _lib.raw_stream(dev)))
        if ctx.logits_dtype != torch.float32:
            grad = grad.to(ctx.logits_dtype)
        if gv is not None:
            shape, dtype = ctx.values_like
            gv = gv.view(shape) if dtype == torch.float32 else gv.view(shape).to(dtype)
        return (grad, gv) + (None,) * 7


def evaluate_actions(logits, actions):
    """(log_probs [M, 1], entropy [M]) of `actions` ([M, 1] or [M]; uint8, int32 or int64) under `logits` [M, A]: what
    rl/networks.py:78-86 computes with softmax, log_softmax and gather -- `entropy.mean()` is its dist_entropy --, in ONE launch,
    differentiable with respect to `logits` in one more.  Serves the PPO branch and the A2C branch (rl/train.py:134-146) alike.

    float32 logits whose rows are dense (any row stride) pass through untouched; anything else is `.float()`-ed (and made
    contiguous) first, which costs a launch, and the gradient comes back in the logits' own dtype.  A row with a NaN, a +inf,
    nothing but -inf, or an action outside [0, A) reads NaN in both outputs and in its gradient row, and is counted: check()."""
    return _EvaluateActions.apply(logits, actions)


def ppo_loss(logits, values, actions, old_log_probs, adv_targ, returns, clip_param, value_loss_coeff, entropy_coeff):
    """The clipped-surrogate loss of rl/train.py:123-129 on a minibatch, from the network's `logits` [M, A] and `values`, and the
    generator's `actions`, `old_log_probs`, `adv_targ`, `returns` (each [M, 1] or [M]):

        (loss, action_loss, value_loss, dist_entropy)      four 0-dim float32 tensors on the device

    loss = action_loss + value_loss_coeff * value_loss - entropy_coeff * dist_entropy is differentiable with respect to `logits`
    and `values`; the other three are detached, for the log line.  Two launches forward, one backward; the means are float64 sums
    in a fixed order (equal inputs give equal bits).  The workspace between the forward's two launches is kept per (device, M):
    calls of one M must be ordered on one stream.  Bad rows (see evaluate_actions) make all four NaN and are counted: check()."""
    return _PPOLoss.apply(logits, values, actions, old_log_probs, adv_targ, returns, clip_param, value_loss_coeff, entropy_coeff)


evaluate_actions.check = ppo_loss.check = check
