"""DeviceAdam -- the two lines that end a PPO update on the device (include/sfmi_optim.h: sf_adam_step).

The reference ends every minibatch with

    torch.nn.utils.clip_grad_norm_(self.actor.parameters(), self.args.max_grad_norm)      # rl/train.py:131
    self.actor_optimizer.step()                                                             # rl/train.py:132  (optim.Adam)

which is a dozen or more _foreach launches and several temporaries.  DeviceAdam.step() is three launches for all parameters
together: the chunks' sums of squares, one block that finishes the norm and the step's scalars, the update.  The step count,
the bias corrections and a skipped step live in a 128-byte state block on the device, so step() decides nothing on the host:
it can be captured in a graph, and every replay of the one captured step performs step t, t + 1, t + 2, ...

    opt = DeviceAdam(net.parameters(), lr=7e-4, max_grad_norm=0.5)       # a torch.optim.Optimizer: zero_grad, schedulers
    loss.backward()
    opt.step()                                                            # no clip_grad_norm_ in front: it is inside
    opt.last_norm(), opt.last_coef(), opt.check()                         # what clip_grad_norm_ returned; skipped steps

A step whose gradients hold a NaN or an inf is SKIPPED and counted (check()); torch would write NaN into every parameter.
The grads themselves are never written.  state_dict() / load_state_dict() use torch.optim.Adam's layout, so a checkpoint moves
between the two either way.  tests/adamref.py restates the call in numpy.
"""
import torch

from . import _lib
from ._lib import ptr

# the state block's fields as indices of its float64 / int64 view (sfmi_optim.h: THE STATE BLOCK)
_T, _B1POW, _B2POW, _LR, _B1, _B2, _EPS, _NORM, _COEF, _SKIPPED = range(10)


def beta_powers(beta1, beta2, t):
    """(beta1^t, beta2^t) as the device holds them: running float64 products, one multiplication per step."""
    p1 = p2 = 1.0
    for _ in range(int(t)):
        p1 *= beta1
        p2 *= beta2
    return p1, p2


STATE_KEYS = ("step", "exp_avg", "exp_avg_sq")  # a parameter's entry in state_dict()["state"]: torch.optim.Adam's


# torch.optim.Adam's own param-group keys at their defaults (foreach, capturable, fused, ... whatever the installed torch has),
# read ONCE from a throw-away instance over one CPU element: a state_dict of DeviceAdam then loads into torch's optimiser, whose
# step() looks every one of them up
_TORCH_ADAM_DEFAULTS = dict(torch.optim.Adam([torch.zeros(1)]).defaults)


def group_defaults(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None):
    """The param group's keys: torch.optim.Adam's own, so that a state_dict of DeviceAdam loads into torch's optimiser and steps
    there, and max_grad_norm."""
    d = dict(_TORCH_ADAM_DEFAULTS, lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps))
    d["max_grad_norm"] = None if max_grad_norm is None else float(max_grad_norm)
    return d


class DeviceAdam(torch.optim.Optimizer):
    """torch.optim.Adam with clip_grad_norm_ in front, as one C call.  One parameter group of float32, contiguous parameters on
    one HIP device; weight_decay, amsgrad and maximize are refused.  max_grad_norm None (or <= 0): no clipping; the norm is
    computed all the same.  The hyper-parameters live in param_groups[0] like torch's; `lr` is uploaded to the device when it
    has changed since the last upload -- at the next step(), or at once by sync_lr() (the way to change it under a replayed
    graph, where no step() runs).  max_grad_norm is an argument of the call: a captured step keeps the one it was captured with."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, max_grad_norm=None, weight_decay=0, amsgrad=False,
                 maximize=False):
        if torch.is_tensor(lr):
            raise ValueError("lr must be a number: the device holds it as a float64")
        defaults = group_defaults(lr, betas, eps, max_grad_norm)
        defaults.update(weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize)
        super().__init__(params, defaults)
        self._refuse(self.param_groups)
        ps = self.param_groups[0]["params"]
        if not 1 <= len(ps) <= _lib.OPT_MAX_TENSORS:
            raise ValueError("DeviceAdam takes 1 to %d parameter tensors (got %d)" % (_lib.OPT_MAX_TENSORS, len(ps)))
        self.device = ps[0].device
        if self.device.type != "cuda":
            raise ValueError("DeviceAdam needs its parameters on a HIP device (got %s): there is no CPU path" % (self.device,))
        for k, p in enumerate(ps):
            self._check_param(k, p)
        self._L = _lib.lib()
        for p in ps:
            self.state[p] = {"step": torch.tensor(0.0), "exp_avg": torch.zeros_like(p, memory_format=torch.contiguous_format),
                             "exp_avg_sq": torch.zeros_like(p, memory_format=torch.contiguous_format)}
        chunks = sum(int(self._L.sf_adam_chunks(p.numel())) for p in ps)
        self._workspace = torch.empty(int(self._L.sf_adam_workspace_bytes(chunks)) // 8, dtype=torch.float64, device=self.device)
        self._state = torch.zeros(_lib.ADAM_STATE_BYTES // 8, dtype=torch.float64, device=self.device)
        self._state_i64 = self._state.view(torch.int64)
        self._errors = torch.zeros(1, dtype=torch.int64, device=self.device)
        self._table = (_lib.OptTensor * len(ps))()
        g = self.param_groups[0]
        _lib.check(self._L.sf_adam_state_init(ptr(self._state), g["lr"], g["betas"][0], g["betas"][1], g["eps"],
                                              _lib.raw_stream(self.device)))
        self._lr_uploaded = float(g["lr"])

    # ------------------------------------------------------------------------------------------------------------ refusals
    @staticmethod
    def _refuse(groups):
        if len(groups) != 1:
            raise ValueError("DeviceAdam takes one parameter group (got %d)" % len(groups))
        g = groups[0]
        if g.get("weight_decay", 0) != 0 or g.get("amsgrad", False) or g.get("maximize", False):
            raise ValueError("DeviceAdam has no weight_decay, amsgrad or maximize (got %r, %r, %r)"
                             % (g.get("weight_decay", 0), g.get("amsgrad", False), g.get("maximize", False)))
        if torch.is_tensor(g["lr"]):
            raise ValueError("lr must be a number: the device holds it as a float64")

    def add_param_group(self, param_group):
        if self.param_groups:
            raise ValueError("DeviceAdam takes one parameter group")
        super().add_param_group(param_group)

    def _check_param(self, k, p):
        if p.dtype != torch.float32 or not p.is_contiguous() or p.device != self.device or p.numel() == 0:
            raise ValueError("parameter %d: DeviceAdam needs non-empty, contiguous float32 tensors on %s (got %s, %s, %s)"
                             % (k, self.device, p.dtype, "contiguous" if p.is_contiguous() else "not contiguous", p.device))

    # ---------------------------------------------------------------------------------------------------------------- step
    def sync_lr(self):
        """Upload param_groups[0]['lr'] to the state block if it has changed since the last upload (one small copy on the
        current stream; nothing synchronises).  step() does this itself; call it after a scheduler's step where the optimiser
        step is a replayed graph.  Not during capture: a copy captured there would be replayed with the old value."""
        lr = float(self.param_groups[0]["lr"])
        if lr != self._lr_uploaded and not torch.cuda.is_current_stream_capturing():
            if not (lr >= 0.0 and lr != float("inf")):
                raise ValueError("lr %r: need a finite, non-negative number" % (lr,))
            self._state[_LR:_LR + 1].fill_(lr)
            self._lr_uploaded = lr

    @torch.no_grad()
    def step(self, closure=None):
        """clip_grad_norm_ and the Adam step for every parameter, three launches (sf_adam_step).  ValueError -- and nothing
        launched -- for a parameter without a .grad or one that is not contiguous float32 on the optimiser's device."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        g = self.param_groups[0]
        ps = g["params"]
        tab = self._table
        for k, p in enumerate(ps):
            self._check_param(k, p)
            gr = p.grad
            if gr is None:
                raise ValueError("parameter %d has no .grad: DeviceAdam steps all of its parameters or none" % k)
            if gr.dtype != torch.float32 or gr.layout != torch.strided or not gr.is_contiguous() or gr.device != self.device:
                raise ValueError("parameter %d: its .grad must be a dense, contiguous float32 tensor on %s" % (k, self.device))
            st = self.state[p]
            e = tab[k]
            e.param, e.grad, e.exp_avg, e.exp_avg_sq, e.numel = p.data_ptr(), gr.data_ptr(), st["exp_avg"].data_ptr(), \
                st["exp_avg_sq"].data_ptr(), p.numel()
        self.sync_lr()
        mgn = g.get("max_grad_norm")
        _lib.check(self._L.sf_adam_step(tab, len(ps), 0.0 if mgn is None else float(mgn), ptr(self._state), ptr(self._workspace),
                                        ptr(self._errors), _lib.raw_stream(self.device)))
        return loss

    # --------------------------------------------------------------------------------------------------------- state block
    def device_state(self):
        """The state block as a dict (sfmi_optim.h: THE STATE BLOCK).  Synchronises."""
        f = self._state.cpu()
        i = f.view(torch.int64)
        return {"t": int(i[_T]), "beta1_pow": float(f[_B1POW]), "beta2_pow": float(f[_B2POW]), "lr": float(f[_LR]),
                "beta1": float(f[_B1]), "beta2": float(f[_B2]), "eps": float(f[_EPS]), "norm": float(f[_NORM]),
                "coef": float(f[_COEF]), "skipped": int(i[_SKIPPED])}

    def last_norm(self):
        """The gradients' total 2-norm at the last step(): what clip_grad_norm_ returned.  Synchronises."""
        return float(self._state[_NORM].item())

    def last_coef(self):
        """The factor the last step() scaled the gradients by (1.0: not clipped; 0.0: the step was skipped).  Synchronises."""
        return float(self._state[_COEF].item())

    def check(self):
        """Steps skipped so far because a gradient was not finite.  Synchronises."""
        return int(self._state_i64[_SKIPPED].item())

    def steps(self):
        """Steps taken so far (skipped ones not counted).  Synchronises."""
        return int(self._state_i64[_T].item())

    # ---------------------------------------------------------------------------------------------------------- checkpoints
    def state_dict(self):
        """torch.optim.Adam's layout: per parameter `step` (the device's t), `exp_avg`, `exp_avg_sq`; max_grad_norm travels in
        the param group.  Synchronises."""
        t = float(self.steps())
        for p in self.param_groups[0]["params"]:
            self.state[p]["step"] = torch.tensor(t)
        return super().state_dict()

    def load_state_dict(self, state_dict):
        """A state_dict of this class or of torch.optim.Adam over the same parameters.  t is the loaded `step` (equal for every
        parameter, or ValueError); beta1^t and beta2^t are rebuilt by t float64 multiplications on the host, the bits the device
        would hold after t steps; the skip counter is kept.  The loaded moments are copied INTO this optimiser's own exp_avg /
        exp_avg_sq tensors and the state block stays where it is, so a graph that captured step() before the load goes on
        from the loaded state at its next replay."""
        self._refuse(state_dict["param_groups"])
        keep = self.param_groups[0].get("max_grad_norm")
        own = {p: (st["exp_avg"], st["exp_avg_sq"]) for p, st in self.state.items()}
        super().load_state_dict(state_dict)
        g = self.param_groups[0]
        g.setdefault("max_grad_norm", keep)
        ps = g["params"]
        ts = set()
        for k, p in enumerate(ps):
            st = self.state.get(p)
            if not st or "exp_avg" not in st or "exp_avg_sq" not in st or "step" not in st:
                if st:
                    raise ValueError("parameter %d: the loaded state needs step, exp_avg and exp_avg_sq" % k)
                st = self.state[p] = {"step": torch.tensor(0.0), "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.zeros_like(p)}
            for name, mine in zip(("exp_avg", "exp_avg_sq"), own.get(p, (None, None))):
                if st[name].shape != p.shape:
                    raise ValueError("parameter %d: %s has shape %s, the parameter %s" % (k, name, tuple(st[name].shape), tuple(p.shape)))
                if mine is None:
                    mine = torch.empty_like(p, memory_format=torch.contiguous_format)
                mine.copy_(st[name])  # (in place: a captured step holds this tensor's address)
                st[name] = mine
            ts.add(float(st["step"]))
            st["step"] = torch.tensor(float(st["step"]))
        if len(ts) != 1 or min(ts) < 0 or min(ts) != int(min(ts)):
            raise ValueError("DeviceAdam keeps one step count for all parameters (the loaded ones: %s)" % sorted(ts))
        t = int(ts.pop())
        b1, b2 = float(g["betas"][0]), float(g["betas"][1])
        p1, p2 = beta_powers(b1, b2, t)
        skipped = self.check()
        _lib.check(self._L.sf_adam_state_init(ptr(self._state), float(g["lr"]), b1, b2, float(g["eps"]), _lib.raw_stream(self.device)))
        self._state[_B1POW:_B2POW + 1].copy_(torch.tensor([p1, p2], dtype=torch.float64))
        self._state_i64[_T].fill_(t)
        self._state_i64[_SKIPPED].fill_(skipped)
        self._lr_uploaded = float(g["lr"])


__all__ = ["DeviceAdam", "beta_powers", "group_defaults", "STATE_KEYS"]
