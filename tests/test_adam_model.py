"""The numpy model of include/sfmi_optim.h (tests/adamref.py) held to torch on the CPU: the norm and coef against a float64
evaluation of clip_grad_norm_'s expression, 50 steps against clip_grad_norm_ + torch.optim.Adam in float64 within a bound
derived from the model's own float32 roundings (profiles/device_adam.md), the skip rule, the running products, and the
checkpoint layout against torch.optim.Adam's."""
import math
import os
import re

import numpy as np
import pytest
import torch

import adamref as AR

f32, f64 = np.float32, np.float64
U64 = 2.0 ** -53


def _sum_depth(sizes):
    """The most float64 additions one square goes through: 8 in its lane, 6 in the tree, 3 among the waves, one per chunk."""
    return 8 + 6 + 3 + AR.total_chunks(sizes)


@pytest.mark.parametrize("sizes", [(1,), (65,), (257, 1), (AR.CHUNK + 1, 63), (3 * AR.CHUNK + 5, 1024, 7)])
@pytest.mark.parametrize("max_grad_norm", (0.5, 1e6, None, 0.0))
def test_norm_and_coef_equal_a_float64_evaluation_of_clip_grad_norms_expression(sizes, max_grad_norm):
    _, G, _, _ = AR.gen_tensors(sizes, 3)
    S = AR.sum_squares(G)
    exact = math.fsum(float(x) * float(x) for g in G for x in g.astype(f64))  # (each product exact, the sum exactly rounded)
    assert abs(S - exact) <= _sum_depth(sizes) * U64 * exact
    norm, coef = AR.norm_coef(S, max_grad_norm)
    # torch's own float64 evaluation
    ts = [torch.from_numpy(g.astype(f64)).requires_grad_() for g in G]
    for t in ts:
        t.grad = t.detach().clone()
    total = float(torch.nn.utils.clip_grad_norm_(ts, max_grad_norm if max_grad_norm else float("inf")))
    rel = (0.5 * _sum_depth(sizes) + sum(sizes) + 2) * U64
    assert abs(norm - total) <= rel * total
    want = min(1.0, max_grad_norm / (math.sqrt(exact) + 1e-6)) if max_grad_norm else 1.0
    assert abs(coef - want) <= (rel + 3 * U64) * want
    if not max_grad_norm or max_grad_norm > 2 * total:
        assert coef == 1.0  # exactly: the grads go through unscaled
        for t, g in zip(ts, G):
            assert np.array_equal(t.grad.numpy(), g.astype(f64))
    else:
        for t, g in zip(ts, G):  # what torch multiplied the grads by
            np.testing.assert_allclose(t.grad.numpy(), g.astype(f64) * float(coef), rtol=1e-12, atol=0)


def test_the_sum_follows_the_headers_order_not_another():
    """A case where the order shows: the lane's own adds come first, then the tree, the waves and the chunks."""
    g = np.zeros(AR.CHUNK + 3, f32)
    g[0], g[1], g[4], g[1024], g[AR.CHUNK] = 2.0 ** 30, 1.0, 1.0, 1.0, 1.0
    # lane 0 holds elements 0-3 and 1024-1027: (2^60 + 1) + 1 rounds to 2^60 twice; lane 1's 1.0 meets lane 0 in the tree
    # (2^60 + 1 = 2^60) and the second chunk's 1.0 the total: every 1.0 is lost, one at a time
    assert AR.sum_squares([g]) == 2.0 ** 60
    parts = AR.chunk_partials(g)
    assert parts.tolist() == [2.0 ** 60, 1.0]
    h = np.zeros(300, f32)
    h[:] = 1.0
    assert AR.sum_squares([h, h]) == 600.0


def _torch_run(P, grads_per_step, lr, betas, eps, max_grad_norm):
    """clip_grad_norm_ + torch.optim.Adam in float64 on the CPU from float32 start values; yields per step the clipped grads,
    the moments before and after and the parameters after, as float64 numpy lists."""
    ps = [torch.from_numpy(p.astype(f64)).requires_grad_() for p in P]
    opt = torch.optim.Adam(ps, lr=lr, betas=betas, eps=eps)
    for G in grads_per_step:
        before = [(opt.state[p]["exp_avg"].numpy().copy(), opt.state[p]["exp_avg_sq"].numpy().copy()) if opt.state[p] else
                  (np.zeros(p.shape), np.zeros(p.shape)) for p in ps]
        for p, g in zip(ps, G):
            p.grad = torch.from_numpy(g.astype(f64))
        if max_grad_norm:
            torch.nn.utils.clip_grad_norm_(ps, max_grad_norm)
        clipped = [p.grad.numpy().copy() for p in ps]
        opt.step()
        yield (clipped, before, [(opt.state[p]["exp_avg"].numpy().copy(), opt.state[p]["exp_avg_sq"].numpy().copy()) for p in ps],
               [p.detach().numpy().copy() for p in ps])


@pytest.mark.parametrize("max_grad_norm", (0.5, None))
def test_fifty_steps_stay_within_the_derived_bound_of_float64_adam(max_grad_norm):
    sizes, steps = (1, 65, 300, AR.CHUNK + 1), 50
    lr, betas, eps = 7e-4, (0.9, 0.999), 1e-8
    P, _, _, _ = AR.gen_tensors(sizes, 5)
    kinds = ("normal", "small", "large")
    grads = [[AR.gen_grad(kinds[(s + k) % 3], n, 100 * s + k) for k, n in enumerate(sizes)] for s in range(steps)]
    state = AR.new_state(lr, betas[0], betas[1], eps)
    M, V = [np.zeros(n, f32) for n in sizes], [np.zeros(n, f32) for n in sizes]
    bound = AR.TrajectoryBound([(n,) for n in sizes])
    worst = 0.0
    for s, (clipped, before, after, p64) in enumerate(_torch_run(P, grads, lr, betas, eps, max_grad_norm)):
        state, P, M, V, stepped = AR.adam_step(state, P, grads[s], M, V, max_grad_norm)
        assert stepped and state["t"] == s + 1
        bc1, bc2 = 1 - betas[0] ** (s + 1), 1 - betas[1] ** (s + 1)
        for k in range(len(sizes)):
            ep = bound.step(k, clipped[k], before[k][0], before[k][1], after[k][0], after[k][1], p64[k], betas[0], betas[1], eps,
                            math.sqrt(bc2), lr / bc1)
            err = np.abs(P[k].astype(f64) - p64[k])
            assert (err <= ep).all(), (s, k, float((err / ep).max()))
            worst = max(worst, float((err / ep).max()))
            assert (np.abs(M[k].astype(f64) - after[k][0]) <= bound.em[k]).all() and (np.abs(V[k].astype(f64) - after[k][1]) <= bound.ev[k]).all()
    print("max_grad_norm %s: worst |error| / bound over %d steps: %.3f; largest bound %.3g" % (
        max_grad_norm, steps, worst, max(float(e.max()) for e in bound.ep)))
    assert worst > 0.01  # (the bound is of the error's own size, not a blanket)


def test_the_float64_replay_of_adamref_is_torchs_float64_adam():
    """float64_trajectory (what the device tests hold both optimisers to) against clip_grad_norm_ + torch.optim.Adam in float64."""
    sizes = (3, 65, 300)
    P, _, _, _ = AR.gen_tensors(sizes, 8)
    grads = [[AR.gen_grad(("normal", "large")[s % 2], n, 31 * s + k) for k, n in enumerate(sizes)] for s in range(12)]
    ours = AR.float64_trajectory(P, grads, 7e-4, 0.9, 0.999, 1e-8, 0.5)
    for (clipped, before, after, p64), (c2, b2, a2, q64, _, _) in zip(_torch_run(P, grads, 7e-4, (0.9, 0.999), 1e-8, 0.5), ours):
        for k in range(len(sizes)):
            np.testing.assert_allclose(c2[k], clipped[k], rtol=1e-13, atol=0)
            # (absolute: torch's lerp form m + w (g - m) cancels where ours adds; gradients here reach 100, squares 1e4)
            np.testing.assert_allclose(a2[k][0], after[k][0], rtol=0, atol=1e-13)
            np.testing.assert_allclose(a2[k][1], after[k][1], rtol=0, atol=1e-11)
            np.testing.assert_allclose(q64[k], p64[k], rtol=0, atol=1e-13)


def test_a_non_finite_gradient_skips_the_step_and_the_next_one_proceeds_from_the_old_state():
    sizes = (65, AR.CHUNK + 1, 7)
    P, G, M, V = AR.gen_tensors(sizes, 9)
    state = AR.new_state(1e-3, 0.9, 0.999, 1e-8)
    state, P, M, V, ok = AR.adam_step(state, P, G, M, V, 0.5)
    assert ok and state["t"] == 1 and state["skipped"] == 0
    for bad, where in ((np.inf, 0), (np.nan, 1), (-np.inf, 2)):
        G2 = [g.copy() for g in G]
        G2[where][-1] = bad
        s2, P2, M2, V2, ok = AR.adam_step(state, P, G2, M, V, 0.5)
        assert not ok and s2["t"] == 1 and s2["skipped"] == state["skipped"] + 1 and s2["apply"] == 0 and s2["coef"] == 0
        assert s2["beta1_pow"] == state["beta1_pow"] and s2["beta2_pow"] == state["beta2_pow"]
        assert not np.isfinite(s2["norm"])
        for a, b in zip(P + M + V, P2 + M2 + V2):
            assert a.tobytes() == b.tobytes()
        # the next finite step: as if the skipped call had not been made
        s3, P3, M3, V3, ok = AR.adam_step(s2, P2, G, M2, V2, 0.5)
        w3, PW, MW, VW, _ = AR.adam_step(state, P, G, M, V, 0.5)
        assert ok and s3["t"] == 2 and s3["skipped"] == s2["skipped"]
        for a, b in zip(PW + MW + VW, P3 + M3 + V3):
            assert a.tobytes() == b.tobytes()
        assert AR.states_equal(dict(w3, skipped=s3["skipped"]), s3)[0]
    # a sum of squares beyond float64 is not finite either
    huge = [np.full(4, 3e38, f32)] * 3
    assert np.isfinite(AR.sum_squares(huge))  # (float32's largest squares fit float64 with room: no such case from float32 grads)


def test_t_and_the_running_products_are_what_load_state_dict_rebuilds():
    from spacefortress_amd.optim import beta_powers

    state = AR.new_state(1e-3, 0.9, 0.999, 1e-8)
    P, G, M, V = AR.gen_tensors((5,), 1)
    for t in range(1, 41):
        state, P, M, V, _ = AR.adam_step(state, P, G, M, V, None)
        p1, p2 = beta_powers(0.9, 0.999, t)
        assert state["t"] == t and float(state["beta1_pow"]) == p1 and float(state["beta2_pow"]) == p2
        assert abs(p1 - 0.9 ** t) <= 2 * t * U64 * 0.9 ** t and abs(p2 - 0.999 ** t) <= 2 * t * U64
        assert state["scalars"][5] == f32(math.sqrt(1.0 - p2)) and state["scalars"][7] == f32(1e-3 / (1.0 - p1))
    loaded = AR.new_state(1e-3, 0.9, 0.999, 1e-8, t=40)
    assert loaded["t"] == 40 and loaded["beta1_pow"] == state["beta1_pow"] and loaded["beta2_pow"] == state["beta2_pow"]
    s1000 = AR.new_state(1e-3, 0.9, 0.999, 1e-8, t=1000)
    assert beta_powers(0.9, 0.999, 1000) == (float(s1000["beta1_pow"]), float(s1000["beta2_pow"]))
    assert 0 < s1000["beta1_pow"] < 1e-45 and abs(s1000["beta2_pow"] - 0.999 ** 1000) < 1e-12


def test_the_checkpoint_layout_is_torch_adams():
    """CPU tensors on torch's side; DeviceAdam itself needs a device (tests/test_gpu_device_adam.py swaps real checkpoints)."""
    from spacefortress_amd import optim

    ps = [torch.nn.Parameter(torch.randn(3, 2)), torch.nn.Parameter(torch.randn(5))]
    ta = torch.optim.Adam(ps, lr=7e-4)
    for p in ps:
        p.grad = torch.randn_like(p)
    ta.step()
    sd = ta.state_dict()
    assert sorted(sd) == ["param_groups", "state"] and sorted(sd["state"]) == [0, 1]
    for st in sd["state"].values():
        assert tuple(sorted(st)) == tuple(sorted(optim.STATE_KEYS))
        assert float(st["step"]) == 1.0
    group = optim.group_defaults(7e-4, (0.9, 0.999), 1e-8, 0.5)
    assert set(group) == (set(sd["param_groups"][0]) - {"params"}) | {"max_grad_norm"}
    for k, v in sd["param_groups"][0].items():
        if k != "params":
            assert group[k] == v, k
    assert group["max_grad_norm"] == 0.5
    # a dict in DeviceAdam's layout (torch's keys and max_grad_norm in the group) loads into torch.optim.Adam and steps there
    mine = {"state": {k: {"step": torch.tensor(3.0), "exp_avg": torch.zeros_like(p), "exp_avg_sq": torch.ones_like(p)}
                      for k, p in enumerate(ps)}, "param_groups": [dict(group, params=[0, 1])]}
    tb = torch.optim.Adam(ps)
    tb.load_state_dict(mine)
    tb.step()
    assert float(tb.state[ps[0]]["step"]) == 4.0 and tb.param_groups[0]["lr"] == 7e-4


def test_the_binding_declares_what_the_header_declares():
    import spacefortress_amd
    from spacefortress_amd import _lib

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "sfmi_optim.h")).read(), flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(sf_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", hdr)}
    assert set(decl) == set(_lib.OPTIM_SYMBOLS)
    for name, args in decl.items():
        n_args = len([a for a in args.split(",") if a.strip() and a.strip() != "void"])
        assert len(_lib.OPTIM_SYMBOLS[name][1]) == n_args, name
        assert hasattr(_lib.lib(), name), name
    for macro, value in (("SF_OPT_MAX_TENSORS", _lib.OPT_MAX_TENSORS), ("SF_OPT_CHUNK", _lib.OPT_CHUNK),
                         ("SF_ADAM_STATE_BYTES", _lib.ADAM_STATE_BYTES)):
        assert re.search(r"#define\s+%s\s+%d\b" % (macro, value), hdr), macro
    assert (AR.MAX_TENSORS, AR.CHUNK, AR.STATE_BYTES) == (_lib.OPT_MAX_TENSORS, _lib.OPT_CHUNK, _lib.ADAM_STATE_BYTES)
    assert _lib.OPT_MAX_TENSORS >= 32
    import ctypes
    assert ctypes.sizeof(_lib.OptTensor) == 40
    L = _lib.lib()
    assert L.sf_adam_state_bytes() == 128 and L.sf_adam_chunks(1) == 1 and L.sf_adam_chunks(AR.CHUNK + 1) == 2
    assert L.sf_adam_workspace_bytes(7) == 56
    assert "DeviceAdam" in spacefortress_amd.__all__ and issubclass(spacefortress_amd.DeviceAdam, torch.optim.Optimizer)
    for name in ("step", "sync_lr", "last_norm", "last_coef", "check", "state_dict", "load_state_dict"):
        assert callable(getattr(spacefortress_amd.DeviceAdam, name))


def test_argument_errors_come_back_as_sf_err_arg_without_a_device():
    """Every refusal of sf_adam_step and sf_adam_state_init is decided on the host before anything is launched."""
    import ctypes as C

    from spacefortress_amd import _lib

    L = _lib.lib()
    good = dict(param=0x1000, grad=0x2000, exp_avg=0x3000, exp_avg_sq=0x4000, numel=5)

    def call(entries, n=None, state=0x10000, ws=0x20000, errors=0x30000):
        tab = (_lib.OptTensor * max(1, len(entries)))()
        for k, e in enumerate(entries):
            tab[k] = _lib.OptTensor(e["param"], e["grad"], e["exp_avg"], e["exp_avg_sq"], e["numel"])
        return L.sf_adam_step(tab, len(entries) if n is None else n, 0.5, C.c_void_p(state), C.c_void_p(ws), C.c_void_p(errors), None)

    for field in ("param", "grad", "exp_avg", "exp_avg_sq"):
        for value in (0, good[field] + 2):  # NULL; misaligned
            assert call([good, dict(good, **{field: value})]) == _lib.SF_ERR_ARG, (field, value)
            assert "tensor 1" in _lib.last_error()
    for numel in (0, -1):
        assert call([dict(good, numel=numel)]) == _lib.SF_ERR_ARG
    assert call([good] * (_lib.OPT_MAX_TENSORS + 1)) == _lib.SF_ERR_ARG and "n_tensors" in _lib.last_error()
    assert call([good], n=0) == _lib.SF_ERR_ARG
    assert call([good], state=0) == _lib.SF_ERR_ARG and call([good], state=0x10008) == _lib.SF_ERR_ARG
    assert call([good], ws=0) == _lib.SF_ERR_ARG and call([good], ws=0x20004) == _lib.SF_ERR_ARG
    assert call([good], errors=0x30004) == _lib.SF_ERR_ARG
    assert L.sf_adam_step(None, 1, 0.5, C.c_void_p(0x10000), C.c_void_p(0x20000), None, None) == _lib.SF_ERR_ARG
    assert call([dict(good, numel=1 << 62)]) == _lib.SF_ERR_ARG and "chunks" in _lib.last_error()
    assert L.sf_adam_state_init(None, 1e-3, 0.9, 0.999, 1e-8, None) == _lib.SF_ERR_ARG
    assert L.sf_adam_state_init(C.c_void_p(0x10008), 1e-3, 0.9, 0.999, 1e-8, None) == _lib.SF_ERR_ARG
    for lr, b1, b2, eps in ((-1.0, 0.9, 0.999, 1e-8), (float("nan"), 0.9, 0.999, 1e-8), (1e-3, 1.0, 0.999, 1e-8),
                            (1e-3, 0.9, -0.1, 1e-8), (1e-3, 0.9, 0.999, float("inf"))):
        assert L.sf_adam_state_init(C.c_void_p(0x10000), lr, b1, b2, eps, None) == _lib.SF_ERR_ARG, (lr, b1, b2, eps)
