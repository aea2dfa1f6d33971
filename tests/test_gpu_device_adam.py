"""include/sfmi_optim.h on the device: sf_adam_step held to tests/adamref.py byte for byte -- parameters, both moments and the
state block -- at every size where the kernels take another path, on the wide and on the narrow access path, with clipping on,
off and idle, at zero and subnormal gradients, at steps 1, 2 and 1000; the skip rule; DeviceAdam under a captured graph,
against torch on the device, through checkpoints both ways; the example's new flags.

Byte equality needs the device's float32 division and square root (and the float64 ones of the finishing block) to be correctly
rounded under the build's flags: every case below makes one square root and two divisions per element and compares all bits, so
a device that rounded otherwise would fail here first.

Every tensor of a call lies inside a sentinel-filled buffer."""
import copy
import ctypes as C
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import adamref as AR
import trainerref as TR
from lockstep import sfa  # noqa: F401  (the fixture)

f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64


def dev():
    return torch.device("cuda", torch.cuda.current_device())


class Buf:
    """n float32 elements inside a sentinel-filled allocation, `shift` floats beyond a 16-byte boundary (0: all paths may move
    16 bytes; 1: 4-byte aligned only)."""

    def __init__(self, data, shift):
        n = data.size
        self.base = torch.empty(n + 2 * GUARD + 4, dtype=torch.float32, device=dev())
        assert self.base.data_ptr() % 16 == 0
        self.base.view(torch.uint8).fill_(TR.SENTINEL_BYTE)
        self.lo, self.n = GUARD + shift, n
        self.view = self.base[self.lo:self.lo + n]
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(data, f32)))
        assert self.view.data_ptr() % 16 == 4 * shift

    def host(self):
        return self.view.cpu().numpy()

    def margins_intact(self):
        u = self.base.view(torch.uint8)
        return bool((u[:4 * self.lo] == TR.SENTINEL_BYTE).all()) and bool((u[4 * (self.lo + self.n):] == TR.SENTINEL_BYTE).all())


class Case:
    """The buffers of one sf_adam_step table.  shifts: per tensor 0 / 1, or one value for all."""

    def __init__(self, sizes, seed=0, kind="normal", shifts=0, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, t=0, zero_moments=False):
        from spacefortress_amd import _lib
        self.lib, self.L = _lib, _lib.lib()
        self.sizes = tuple(sizes)
        shifts = [shifts] * len(sizes) if isinstance(shifts, int) else list(shifts)
        P, G, M, V = AR.gen_tensors(self.sizes, seed, kind)
        if zero_moments:
            M, V = [np.zeros_like(m) for m in M], [np.zeros_like(v) for v in V]
        self.P, self.G, self.M, self.V = ([Buf(x, s) for x, s in zip(X, shifts)] for X in (P, G, M, V))
        self.state = torch.zeros(AR.STATE_BYTES // 8 + 2 * 8, dtype=torch.float64, device=dev())
        self.state.view(torch.uint8).fill_(TR.SENTINEL_BYTE)
        self.state_view = self.state[8:8 + AR.STATE_BYTES // 8]
        self.ws = TR.guarded(AR.total_chunks(self.sizes), torch.float64, dev())
        assert int(self.L.sf_adam_workspace_bytes(AR.total_chunks(self.sizes))) == 8 * self.ws.numel()
        self.errors = TR.guarded(1, torch.int64, dev())
        self.errors.zero_()
        self.model_state = AR.new_state(lr, betas[0], betas[1], eps, t)
        if t == 0:
            assert self.L.sf_adam_state_init(C.c_void_p(self.state_view.data_ptr()), lr, betas[0], betas[1], eps, self.stream()) == 0
        else:  # a loaded state: the block as load_state_dict builds it
            self.state_view.view(torch.uint8).copy_(torch.from_numpy(AR.state_bytes(self.model_state)))

    def stream(self):
        return self.lib.raw_stream(dev())

    def table(self):
        tab = (self.lib.OptTensor * len(self.sizes))()
        for k in range(len(self.sizes)):
            tab[k] = self.lib.OptTensor(self.P[k].view.data_ptr(), self.G[k].view.data_ptr(), self.M[k].view.data_ptr(),
                                        self.V[k].view.data_ptr(), self.sizes[k])
        return tab

    def call(self, max_grad_norm):
        return self.L.sf_adam_step(self.table(), len(self.sizes), 0.0 if max_grad_norm is None else max_grad_norm,
                                   C.c_void_p(self.state_view.data_ptr()), C.c_void_p(self.ws.data_ptr()),
                                   C.c_void_p(self.errors.data_ptr()), self.stream())

    def host(self):
        """-> (P, G, M, V as numpy lists, the parsed state block, errors); checks every sentinel."""
        torch.cuda.synchronize()
        for b in self.P + self.G + self.M + self.V:
            assert b.margins_intact()
        TR.margins_intact(self.ws, self.errors)
        u = self.state.view(torch.uint8)
        assert bool((u[:64] == TR.SENTINEL_BYTE).all()) and bool((u[64 + AR.STATE_BYTES:] == TR.SENTINEL_BYTE).all())
        st = AR.parse_state(self.state_view.view(torch.uint8).cpu().numpy())
        assert not st["tail"].any()
        return ([b.host() for b in self.P], [b.host() for b in self.G], [b.host() for b in self.M], [b.host() for b in self.V], st,
                int(self.errors.item()))

    def set_grads(self, G):
        for b, g in zip(self.G, G):
            b.view.copy_(torch.from_numpy(np.ascontiguousarray(g, f32)))


def _same(got, want, what):
    for k, (a, b) in enumerate(zip(got, want)):
        TR.assert_bits_equal(a, b, (what, k))


def _hold_step(c, max_grad_norm, what, expect_step=True):
    """One call on the device against the model, from whatever the buffers hold; the grads stay as they were."""
    P, G, M, V, st0, e0 = c.host()
    ms, PW, MW, VW, stepped = AR.adam_step(c.model_state, P, G, M, V, max_grad_norm)
    assert stepped == expect_step, what
    assert c.call(max_grad_norm) == 0, c.lib.last_error()
    P2, G2, M2, V2, st, e1 = c.host()
    _same(G2, G, (what, "grads are only read"))
    _same(P2, PW, (what, "param"))
    _same(M2, MW, (what, "exp_avg"))
    _same(V2, VW, (what, "exp_avg_sq"))
    ok, field = AR.states_equal(st, ms)
    assert ok, (what, field, st, ms)
    assert e1 - e0 == (0 if stepped else 1), what
    c.model_state = ms
    return st


SHAPES = [(1,), (63, 64, 65), (255, 256, 257), (1023, 1024, 1025), (AR.CHUNK - 1, AR.CHUNK, AR.CHUNK + 1), (3 * AR.CHUNK + 5,),
          (7, 3 * AR.CHUNK + 5, 1, AR.CHUNK + 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("shift", (0, 1))
@pytest.mark.parametrize("sizes", SHAPES)
def test_every_size_on_the_wide_and_on_the_narrow_path_equals_the_model_byte_for_byte(sfa, sizes, shift):
    c = Case(sizes, seed=1, shifts=shift)
    st = _hold_step(c, 0.5, "step 1 %s shift %d" % (sizes, shift))
    assert st["t"] == 1 and st["apply"] == 1 and st["skipped"] == 0
    st = _hold_step(c, 0.5, "step 2 %s shift %d" % (sizes, shift))  # from the moments step 1 left, the same grads
    assert st["t"] == 2
    # determinism: a second case with equal inputs gives equal bytes
    d = Case(sizes, seed=1, shifts=shift)
    assert d.call(0.5) == 0 and d.call(0.5) == 0
    for a, b in zip(c.host()[:4], d.host()[:4]):
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
    assert AR.states_equal(c.host()[4], d.host()[4])[0]


@pytest.mark.gpu
def test_mixed_alignment_in_one_table_moves_each_tensor_by_its_own_rule(sfa):
    sizes = (AR.CHUNK + 5, 300, AR.CHUNK + 5, 300)
    c = Case(sizes, seed=2, shifts=(0, 1, 1, 0))
    _hold_step(c, 0.5, "mixed")
    # only ONE of a tensor's four pointers off the boundary: still the narrow path, the same bytes
    d = Case(sizes, seed=2, shifts=0)
    g = d.G[2]
    d.G[2] = Buf(g.host(), 1)
    _hold_step(d, 0.5, "one pointer narrow")
    for a, b in zip(c.host()[0], d.host()[0]):
        assert a.tobytes() == b.tobytes()


@pytest.mark.gpu
def test_a_full_table_steps_and_one_tensor_more_is_refused(sfa):
    r = np.random.default_rng(5)
    sizes = tuple(int(x) for x in r.choice(AR.SIZES[:-1], AR.MAX_TENSORS))
    c = Case(sizes, seed=3, shifts=[k % 2 for k in range(AR.MAX_TENSORS)])
    _hold_step(c, 1.0, "full table")
    before = c.host()
    tab = (c.lib.OptTensor * (AR.MAX_TENSORS + 1))()
    for k in range(AR.MAX_TENSORS + 1):
        tab[k] = c.table()[k % AR.MAX_TENSORS]
    rc = c.L.sf_adam_step(tab, AR.MAX_TENSORS + 1, 1.0, C.c_void_p(c.state_view.data_ptr()), C.c_void_p(c.ws.data_ptr()), None, c.stream())
    assert rc == c.lib.SF_ERR_ARG and "n_tensors" in c.lib.last_error()
    after = c.host()
    for a, b in zip(before[:4], after[:4]):
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
    assert AR.states_equal(before[4], after[4])[0]


@pytest.mark.gpu
@pytest.mark.parametrize("kind,max_grad_norm,coef_one", [("small", 0.5, True), ("large", 0.5, False), ("normal", 0.5, False),
                                                         ("large", None, True), ("large", 0.0, True), ("zero", 0.5, True),
                                                         ("subnormal", 0.5, True), ("subnormal", None, True)])
@pytest.mark.parametrize("t0", (0, 1, 999))
def test_clipping_on_idle_and_off_zero_and_subnormal_grads_at_steps_1_2_and_1000(sfa, kind, max_grad_norm, coef_one, t0):
    sizes = (65, AR.CHUNK + 1, 257)
    c = Case(sizes, seed=4 + t0, kind=kind, shifts=(0, 1, 0), t=t0, zero_moments=(t0 == 0))
    st = _hold_step(c, max_grad_norm, "%s max %s t0 %d" % (kind, max_grad_norm, t0))
    assert st["t"] == t0 + 1
    assert (st["coef"] == 1.0) == coef_one and st["scalars"][0] == f32(st["coef"])
    if kind == "zero":
        assert st["norm"] == 0.0
    if kind == "subnormal":
        assert 0 < st["norm"] < 1e-35  # (the squares are exact in float64: the norm of subnormals is not zero)
    if t0 == 999:
        p1, p2 = AR.new_state(t=1000)["beta1_pow"], AR.new_state(t=1000)["beta2_pow"]
        assert st["beta1_pow"] == p1 and st["beta2_pow"] == p2


@pytest.mark.gpu
@pytest.mark.parametrize("bad", (np.inf, np.nan, -np.inf))
@pytest.mark.parametrize("where", (0, 2, 4))
def test_a_non_finite_gradient_skips_the_step_byte_for_byte_and_is_counted(sfa, bad, where):
    sizes = (65, AR.CHUNK + 1, 3 * AR.CHUNK + 5, 1, 300)
    c = Case(sizes, seed=6, shifts=(0, 1, 0, 0, 1))
    _hold_step(c, 0.5, "the step before")
    P, G, M, V, st, e = c.host()
    G2 = [g.copy() for g in G]
    G2[where][sizes[where] // 2] = bad
    c.set_grads(G2)
    st2 = _hold_step(c, 0.5, "skipped", expect_step=False)
    assert st2["t"] == 1 and st2["skipped"] == 1 and st2["apply"] == 0 and st2["coef"] == 0.0 and not np.isfinite(st2["norm"])
    assert st2["beta1_pow"] == st["beta1_pow"] and st2["beta2_pow"] == st["beta2_pow"]
    P2, _, M2, V2, _, e2 = c.host()
    for a, b in zip(P + M + V, P2 + M2 + V2):
        assert a.tobytes() == b.tobytes()
    assert e2 == e + 1
    # errors_dev may be NULL: the block's own counter still counts
    assert c.L.sf_adam_step(c.table(), len(sizes), 0.5, C.c_void_p(c.state_view.data_ptr()), C.c_void_p(c.ws.data_ptr()), None,
                            c.stream()) == 0
    c.model_state = dict(c.model_state, skipped=2)
    P3, _, M3, V3, st3, e3 = c.host()
    assert st3["skipped"] == 2 and e3 == e2 and st3["t"] == 1
    for a, b in zip(P + M + V, P3 + M3 + V3):
        assert a.tobytes() == b.tobytes()
    # the next finite step proceeds from the old state
    c.set_grads(G)
    st4 = _hold_step(c, 0.5, "the step after")
    assert st4["t"] == 2 and st4["skipped"] == 2 and st4["apply"] == 1


# ------------------------------------------------------------------------------------------------------------------ DeviceAdam
def _params(sizes, seed, device=None):
    r = np.random.default_rng([seed, 4242])
    return [torch.nn.Parameter(torch.from_numpy(r.standard_normal(n).astype(f32)).to(device or dev())) for n in sizes]


def _opt_state(opt):
    return AR.parse_state(opt._state.view(torch.uint8).cpu().numpy())


def _snapshot(opt, ps):
    return ([p.detach().cpu().numpy().reshape(-1) for p in ps], [opt.state[p]["exp_avg"].cpu().numpy().reshape(-1) for p in ps],
            [opt.state[p]["exp_avg_sq"].cpu().numpy().reshape(-1) for p in ps])


def _model_steps(state, P, M, V, grads_per_step, max_grad_norm, lrs=None):
    for k, G in enumerate(grads_per_step):
        if lrs is not None:
            state = dict(state, lr=f64(lrs[k]))
        state, P, M, V, ok = AR.adam_step(state, P, G, M, V, max_grad_norm)
        assert ok
    return state, P, M, V


@pytest.mark.gpu
def test_one_captured_step_replayed_three_times_is_three_model_steps_and_reads_a_new_lr(sfa):
    sizes = (65, AR.CHUNK + 1, 300)
    ps = _params(sizes, 1)
    opt = sfa.DeviceAdam(ps, lr=1e-3, max_grad_norm=0.5)
    grads = [[AR.gen_grad("normal", n, 10 * s + k) for k, n in enumerate(sizes)] for s in range(3)]
    for p in ps:
        p.grad = torch.zeros_like(p)
    P, M, V = _snapshot(opt, ps)
    state0 = _opt_state(opt)
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            opt.step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    assert _opt_state(opt)["t"] == 0  # capturing stepped nothing
    lrs = (1e-3, 1e-3, 2.5e-4)
    for s in range(3):
        for p, g in zip(ps, grads[s]):
            p.grad.copy_(torch.from_numpy(g))  # refilled in place: the graph holds these addresses
        if lrs[s] != opt.param_groups[0]["lr"]:
            opt.param_groups[0]["lr"] = lrs[s]  # what a scheduler does
            opt.sync_lr()
        graph.replay()
    torch.cuda.synchronize()
    ms, PW, MW, VW = _model_steps(state0, P, M, V, grads, 0.5, lrs)
    P2, M2, V2 = _snapshot(opt, ps)
    _same(P2, PW, "param after three replays")
    _same(M2, MW, "exp_avg")
    _same(V2, VW, "exp_avg_sq")
    st = _opt_state(opt)
    assert st["t"] == 3 and st["lr"] == 2.5e-4 and AR.states_equal(st, ms)[0], (st, ms)
    assert opt.steps() == 3 and opt.check() == 0 and opt.last_norm() == float(ms["norm"]) and opt.last_coef() == float(ms["coef"])
    # an eager step uploads a changed lr by itself
    opt.param_groups[0]["lr"] = 5e-4
    opt.step()
    assert _opt_state(opt)["lr"] == 5e-4 and opt.steps() == 4


@pytest.mark.gpu
def test_what_device_adam_refuses(sfa):
    d = dev()
    with pytest.raises(ValueError):
        sfa.DeviceAdam([torch.nn.Parameter(torch.zeros(8, dtype=torch.float16, device=d))])
    with pytest.raises(ValueError):
        sfa.DeviceAdam([torch.nn.Parameter(torch.zeros(4, 6, device=d).t())])
    with pytest.raises(ValueError):
        sfa.DeviceAdam([{"params": _params((4,), 1)}, {"params": _params((5,), 2)}])
    with pytest.raises(ValueError):
        sfa.DeviceAdam(_params((4,), 1), weight_decay=0.1)
    with pytest.raises(ValueError):
        sfa.DeviceAdam(_params((4,), 1), amsgrad=True)
    with pytest.raises(ValueError):
        sfa.DeviceAdam([torch.nn.Parameter(torch.zeros(4))])  # a CPU parameter: there is no CPU path
    ps = _params((4, 9), 3)
    opt = sfa.DeviceAdam(ps)
    with pytest.raises(ValueError):
        opt.add_param_group({"params": _params((3,), 4)})
    ps[0].grad = torch.ones_like(ps[0])
    before = _snapshot(opt, ps)
    with pytest.raises(ValueError):  # a None grad: no silent partial step
        opt.step()
    after = _snapshot(opt, ps)
    for a, b in zip(before, after):
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
    assert opt.steps() == 0
    ps[1].grad = torch.ones_like(ps[1])
    opt.step()
    assert opt.steps() == 1 and opt.check() == 0
    ps[1].grad[3] = float("nan")
    opt.step()
    assert opt.steps() == 1 and opt.check() == 1 and opt.last_coef() == 0.0
    opt.zero_grad()  # the base class's, as written
    assert ps[0].grad is None


def _example():
    spec = importlib.util.spec_from_file_location("ppo_loop_example", os.path.join(ROOT, "examples", "ppo_loop.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _train(net, opt, clip, batches):
    """Five minibatch updates of the example's loss on fixed batches -> the grads of every update (float32 numpy, unclipped)."""
    rec = []
    for obs, act, ret, old_logp, adv in batches:
        dist, value = net(obs)
        ratio = torch.exp(dist.log_prob(act.squeeze(1)).unsqueeze(1) - old_logp)
        loss = (-torch.min(ratio * adv, torch.clamp(ratio, 0.9, 1.1) * adv).mean() + 0.5 * (value - ret).pow(2).mean()
                - 0.01 * dist.entropy().mean())
        opt.zero_grad()
        loss.backward()
        rec.append([p.grad.detach().cpu().numpy().reshape(-1).copy() for p in net.parameters()])
        if clip is not None:
            torch.nn.utils.clip_grad_norm_(net.parameters(), clip)
        opt.step()
    return rec


@pytest.mark.gpu
def test_the_examples_network_trains_as_under_clip_grad_norm_and_torch_adam(sfa):
    """Each run is held to Adam in float64 under ITS OWN recorded gradients within the bound of tests/test_adam_model.py
    (torch's side with one extra term, its float32 norm); the two runs then differ by no more than both bounds and the distance of the two float64 trajectories."""
    ex = _example()
    d = dev()
    torch.manual_seed(11)
    net_a = ex.ActorCritic(15, 3).to(d)
    net_b = ex.ActorCritic(15, 3).to(d)
    net_b.load_state_dict(net_a.state_dict())
    r = torch.Generator(device="cpu").manual_seed(5)
    batches = []
    for _ in range(5):
        obs = torch.randn(256, 15, generator=r)
        batches.append(tuple(x.to(d) for x in (obs, torch.randint(0, 3, (256, 1), generator=r), torch.randn(256, 1, generator=r),
                                               -1.1 + 0.1 * torch.randn(256, 1, generator=r), torch.randn(256, 1, generator=r))))
    lr, clip = 7e-4, 0.5
    start = [p.detach().cpu().numpy().reshape(-1).copy() for p in net_a.parameters()]
    shapes = [p.shape for p in start]
    N = sum(p.size for p in start)
    grads_a = _train(net_a, torch.optim.Adam(net_a.parameters(), lr=lr), clip, batches)
    opt_b = sfa.DeviceAdam(net_b.parameters(), lr=lr, max_grad_norm=clip)
    grads_b = _train(net_b, opt_b, None, batches)
    assert opt_b.steps() == 5 and opt_b.check() == 0
    ends, bounds, exact = [], [], []
    for net, grads, kw in ((net_a, grads_a, dict(g_rel=AR.torch_norm_rel(N))), (net_b, grads_b, {})):
        tb = AR.TrajectoryBound(shapes, **kw)
        for clipped, before, after, p64, sb, step in AR.float64_trajectory(start, grads, lr, 0.9, 0.999, 1e-8, clip):
            ep = [tb.step(k, clipped[k], before[k][0], before[k][1], after[k][0], after[k][1], p64[k], 0.9, 0.999, 1e-8, sb, step)
                  for k in range(len(shapes))]
        end = [p.detach().cpu().numpy().reshape(-1).astype(f64) for p in net.parameters()]
        worst = max(float((np.abs(e - x) / b).max()) for e, x, b in zip(end, p64, ep))
        print("worst |error| / bound against float64 Adam: %.3f" % worst)
        assert worst <= 1.0
        ends.append(end), bounds.append(ep), exact.append(p64)
    for k in range(len(shapes)):
        assert (np.abs(ends[0][k] - ends[1][k]) <= bounds[0][k] + bounds[1][k] + np.abs(exact[0][k] - exact[1][k])).all()
    moved = max(float(np.abs(e - s).max()) for e, s in zip(ends[1], start))
    assert moved > 1e-3  # (five steps of lr 7e-4: the parameters did move)


@pytest.mark.gpu
def test_a_checkpoint_moves_between_torch_adam_and_device_adam_either_way(sfa):
    sizes = (65, AR.CHUNK + 1, 7)
    ps = _params(sizes, 7)
    ta = torch.optim.Adam(ps, lr=3e-4, betas=(0.8, 0.99), eps=1e-6)
    for s in range(3):
        for k, p in enumerate(ps):
            p.grad = torch.from_numpy(AR.gen_grad("normal", sizes[k], 50 * s + k)).to(dev())
        ta.step()
    sd = ta.state_dict()
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    opt = sfa.DeviceAdam(qs, lr=1e-3, max_grad_norm=0.5)
    opt.load_state_dict(sd)
    g = opt.param_groups[0]
    assert (g["lr"], tuple(g["betas"]), g["eps"], g["max_grad_norm"]) == (3e-4, (0.8, 0.99), 1e-6, 0.5)
    st = _opt_state(opt)
    want = AR.new_state(3e-4, 0.8, 0.99, 1e-6, t=3)
    assert AR.states_equal(st, want)[0], (st, want)
    P, M, V = _snapshot(opt, qs)
    _same(M, [ta.state[p]["exp_avg"].cpu().numpy().reshape(-1) for p in ps], "loaded exp_avg")
    G = [AR.gen_grad("normal", n, 900 + k) for k, n in enumerate(sizes)]
    for q, gr in zip(qs, G):
        q.grad = torch.from_numpy(gr).to(dev())
    opt.step()
    ms, PW, MW, VW = _model_steps(want, P, M, V, [G], 0.5)
    P2, M2, V2 = _snapshot(opt, qs)
    _same(P2, PW, "param, one step after the load")
    _same(M2, MW, "exp_avg")
    _same(V2, VW, "exp_avg_sq")
    assert AR.states_equal(_opt_state(opt), ms)[0]
    # and back: torch's layout and keys, step = 4, loadable by torch.optim.Adam, which steps from it
    back = opt.state_dict()
    assert sorted(back["state"]) == [0, 1, 2]
    for k, e in back["state"].items():
        assert sorted(e) == ["exp_avg", "exp_avg_sq", "step"] and float(e["step"]) == 4.0
    assert back["param_groups"][0]["max_grad_norm"] == 0.5
    tb = torch.optim.Adam(qs)
    tb.load_state_dict(copy.deepcopy(back))  # (torch keeps the dict's own `step` tensors and counts in them)
    assert tb.param_groups[0]["lr"] == 3e-4
    tb.step()
    assert float(tb.state[qs[0]]["step"]) == 5.0
    # a step captured BEFORE a load goes on from the loaded state: the moments are loaded in place
    rs = [torch.nn.Parameter(q.detach().clone()) for q in qs]
    cap = sfa.DeviceAdam(rs, max_grad_norm=0.5)
    for r_, gr in zip(rs, G):
        r_.grad = torch.from_numpy(gr).to(dev())
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            cap.step()
    torch.cuda.current_stream().wait_stream(side)
    addresses = [cap.state[r_]["exp_avg"].data_ptr() for r_ in rs]
    cap.load_state_dict(copy.deepcopy(back))
    assert [cap.state[r_]["exp_avg"].data_ptr() for r_ in rs] == addresses
    P0, M0, V0 = _snapshot(cap, rs)
    graph.replay()
    torch.cuda.synchronize()
    ms5, PW5, MW5, VW5 = _model_steps(AR.new_state(3e-4, 0.8, 0.99, 1e-6, t=4), P0, M0, V0, [G], 0.5)
    P5, M5, V5 = _snapshot(cap, rs)
    _same(P5, PW5, "param, a replay after the load")
    _same(M5, MW5, "exp_avg")
    _same(V5, VW5, "exp_avg_sq")
    assert AR.states_equal(_opt_state(cap), ms5)[0] and cap.steps() == 5
    # DeviceAdam -> DeviceAdam
    again = sfa.DeviceAdam([torch.nn.Parameter(q.detach().clone()) for q in qs])
    again.load_state_dict(back)
    assert again.steps() == 4 and again.param_groups[0]["max_grad_norm"] == 0.5
    assert AR.states_equal(dict(_opt_state(again), norm=f64(0), coef=f64(0), apply=0, scalars=np.zeros(8, f32)),
                           AR.new_state(3e-4, 0.8, 0.99, 1e-6, t=4))[0]


@pytest.mark.gpu
def test_the_example_runs_with_the_device_optimizer_under_a_captured_update(sfa):
    cmd = [sys.executable, os.path.join(ROOT, "examples", "ppo_loop.py"), "--device-optimizer", "--max-grad-norm", "0.5", "--graph-update",
           "--envs", "256", "--steps", "8", "--iters", "2"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    m = re.findall(r"device optimizer: last grad norm ([0-9.eE+-]+), coef ([0-9.eE+-]+), skipped steps (\d+)", out.stdout)
    assert m, out.stdout[-2000:]
    assert int(m[-1][2]) == 0 and float(m[-1][0]) > 0 and 0 < float(m[-1][1]) <= 1
    assert "replays of the one captured update" in out.stdout
