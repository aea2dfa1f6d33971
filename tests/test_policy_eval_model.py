"""The numpy model of the policy head's update side (tests/policyevalref.py), held to what it restates.  No GPU.

  * its closed forms are torch's float64 autograd of the reference's literal expressions -- log_softmax / gather / the entropy
    (rl/networks.py:78-86), the loss of rl/train.py:123-129, the A2C loss of rl/train.py:140-144 -- to float64's precision;
  * the model lies within the derived bounds (profiles/policy_eval.md) of the closed forms, masked logits and actions on masked
    logits included;
  * its log-probabilities and entropies are policyref.policy_head's, bit for bit, for that head's own actions;
  * its rule for ties and the clip's closed range is torch's;
  * its fixed summation order sums what math.fsum sums;
  * no case of the GPU tests has a ratio within the derived margin of a clip bound;
  * the header declares what the binding binds, and the built library exports it.
"""
import math
import os
import re

import numpy as np
import pytest
import torch

import policyevalref as ER
import policyref as PR

LO, HI = ER.clip_bounds(ER.CLIP)
VC, EC = ER.VALUE_COEF, ER.ENTROPY_COEF


def _t(x, grad=False):
    return torch.from_numpy(np.asarray(x)).double().requires_grad_(grad)


def _plain_rows(n, A, scale, seed):
    """rows without -inf: the reference's literal -(log_probs * probs) is NaN at a masked logit"""
    return (np.random.default_rng([seed, n, A]).standard_normal((n, A)) * scale).astype(np.float32)


def _reference_evaluate(xt, a):
    """rl/networks.py:82-85 without the final mean"""
    probs, log_probs = torch.softmax(xt, dim=1), torch.log_softmax(xt, dim=1)
    return log_probs.gather(1, torch.from_numpy(a)[:, None]), -(log_probs * probs).sum(-1)


@pytest.mark.parametrize("A", [1, 3, 5, 16, 32])
@pytest.mark.parametrize("scale", [0.1, 1.0, 10.0])
def test_closed_forms_are_torchs_float64_autograd_of_the_literal_expressions(A, scale):
    n = 300
    x = _plain_rows(n, A, scale, 1)
    a, old, adv, v, ret = ER.ppo_columns(x, 2)
    r = np.random.default_rng(A)
    gl, gH = r.standard_normal(n).astype(np.float32), r.standard_normal(n).astype(np.float32)
    # evaluate_actions and its gradient under arbitrary upstream gradients
    xt = _t(x, True)
    logp, ent = _reference_evaluate(xt, a)
    (logp[:, 0] * _t(gl) + ent * _t(gH)).sum().backward()
    E = ER.exact_row(x, a)
    assert np.allclose(E["logp"], logp[:, 0].detach().numpy(), rtol=1e-12, atol=1e-13)
    assert np.allclose(E["H"], ent.detach().numpy(), rtol=1e-12, atol=1e-13)
    assert np.allclose(ER.exact_grad(E, gl, gH), xt.grad.numpy(), rtol=1e-11, atol=1e-13)
    # the PPO loss, rl/train.py:123-129, with the float32 clip bounds and coefficients the call gets
    xt, vt = _t(x, True), _t(v, True)
    action_log_probs, ent = _reference_evaluate(xt, a)
    dist_entropy = ent.mean()
    ratio = torch.exp(action_log_probs - _t(old)[:, None])
    surr1 = ratio * _t(adv)[:, None]
    surr2 = torch.clamp(ratio, float(LO), float(HI)) * _t(adv)[:, None]
    action_loss = -torch.min(surr1, surr2).mean()
    value_loss = (vt[:, None] - _t(ret)[:, None]).pow(2).mean()
    loss = action_loss + float(np.float32(VC)) * value_loss - float(np.float32(EC)) * dist_entropy
    g = 0.75
    (loss * g).backward()
    X = ER.exact_ppo(x, v, a, old, adv, ret, LO, HI, VC, EC, g)
    want = [action_loss.item(), value_loss.item(), dist_entropy.item(), loss.item()]
    assert np.allclose(X["sums"], want, rtol=1e-12, atol=1e-14)
    assert np.allclose(X["grad_logits"], xt.grad.numpy(), rtol=1e-10, atol=1e-15)
    assert np.allclose(X["grad_values"], vt.grad.numpy(), rtol=1e-12, atol=1e-16)
    # the A2C loss, rl/train.py:140-144: evaluate_actions' gradient under g_logp = -adv / M, g_entropy = -entropy_coeff / M
    xt, vt = _t(x, True), _t(v, True)
    action_log_probs, ent = _reference_evaluate(xt, a)
    advantages = _t(ret)[:, None] - vt[:, None]
    a2c = -(advantages.detach() * action_log_probs).mean() + VC * advantages.pow(2).mean() - EC * ent.mean()
    a2c.backward()
    adv_a2c = (ret.astype(np.float64) - v.astype(np.float64))
    assert np.allclose(ER.exact_grad(E, -adv_a2c / n, np.full(n, -EC / n)), xt.grad.numpy(), rtol=1e-10, atol=1e-15)


def _within(got, want, bound, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    both_inf = np.isinf(got) & (got == want)
    with np.errstate(invalid="ignore"):
        err = np.where(both_inf, 0.0, np.abs(got - want))
    assert np.isfinite(err).all() and (err <= bound).all(), (what, float(np.nanmax(err - bound)))


@pytest.mark.parametrize("A", [1, 3, 4, 5, 8, 9, 16, 17, 32])
@pytest.mark.parametrize("scale", ER.SCALES)
def test_the_model_lies_within_the_bounds_of_the_closed_forms(A, scale):
    n = 1000
    x = PR.general_rows(n, A, scale, 3)  # a quarter of the entries -inf
    a, old, adv, v, ret = ER.ppo_columns(x, 4)
    assert A == 1 or (~np.isfinite(np.take_along_axis(x, a[:, None], 1))).any()  # some actions sit on a masked logit
    r = np.random.default_rng(A)
    gl, gH = r.standard_normal(n).astype(np.float32), r.standard_normal(n).astype(np.float32)
    E = ER.exact_row(x, a)
    logp, ent, bad = ER.evaluate(x, a)
    assert not bad.any()
    xa, dlt = ER.ratio_inputs(x, a, old)
    _within(logp, E["logp"], PR.logp_bound(A, xa), "logp")
    _within(ent, E["H"], PR.entropy_bound(A), "entropy")
    grad = ER.evaluate_backward(x, a, gl, gH)
    _within(grad, ER.exact_grad(E, gl, gH), ER.grad_bound(E, A, gl, gH), "grad")
    assert (grad[x == -np.inf] == 0).all()
    # the exact rows sum to 0 -- but for an action on a masked logit, whose own entry is held at 0: those sum to -g_logp
    assert (np.abs(grad.astype(np.float64).sum(1) - ER.exact_row_sum(E, gl)) <= ER.grad_bound(E, A, gl, gH).sum(1)).all()
    g = 1.0
    terms, sums, bad, _ = ER.ppo_loss(x, v, a, old, adv, ret, LO, HI, VC, EC)
    X = ER.exact_ppo(x, v, a, old, adv, ret, LO, HI, VC, EC, g)
    er = ER.ratio_rel_bound(A, xa, dlt)
    _within(terms[:, 0], X["s"], ER.s_bound(X["r"], adv, LO, er), "s")
    _within(terms[:, 1], X["q"], 3 * ER.U * X["q"] * ER.SLACK + 2.0 ** -149, "q")
    for j in range(3):
        t = terms[:, j].astype(np.float64)
        sign = -1.0 if j == 0 else 1.0
        assert abs(float(sums[j]) - sign * t.sum() / n) <= ER.sums_bound(t, n), j
    assert sums[3] == ER.combine(sums[0], sums[1], sums[2], VC, EC)
    gL, gV = ER.ppo_loss_backward(x, v, a, old, adv, ret, LO, HI, VC, EC, g)
    bL, bV = ER.ppo_grad_bounds(X, A, adv, g, VC, xa, dlt)
    _within(gL, X["grad_logits"], bL, "loss grad_logits")
    _within(gV, X["grad_values"], bV, "loss grad_values")


@pytest.mark.parametrize("A", [1, 3, 5, 16, 32])
def test_logp_and_entropy_are_the_sampling_heads_bit_for_bit(A):
    n = 2000
    x = PR.general_rows(n, A, 1.0, 5)
    for mode in (0, 1):
        head = PR.policy_head(x, mode=mode, seed=9, first_lane=3, ticks=2)
        logp, ent, bad = ER.evaluate(x, head["action"])
        assert not bad.any()
        assert np.array_equal(logp.view(np.uint32), head["logp"].view(np.uint32))
        assert np.array_equal(ent.view(np.uint32), head["entropy"].view(np.uint32))
        # ... so the first update's ratio is exactly 1 and clipping at [1, 1] still passes the whole gradient
        adv = np.random.default_rng(A).standard_normal(n).astype(np.float32)
        z = np.zeros(n, np.float32)
        _, _, _, r = ER.ppo_loss(x, z, head["action"], head["logp"], adv, z, 1.0, 1.0, VC, EC)
        assert (r == 1).all()
        clipped = ER.ppo_loss_backward(x, z, head["action"], head["logp"], adv, z, 1.0, 1.0, VC, EC, 1.0)[0]
        free = ER.ppo_loss_backward(x, z, head["action"], head["logp"], adv, z, 0.0, np.inf, VC, EC, 1.0)[0]
        assert np.array_equal(clipped, free) and (A == 1 or (clipped != 0).any())  # (one action: nothing to learn)


def test_bad_rows_and_actions_outside_the_set():
    x = np.zeros((7, 4), np.float32)
    x[1, 2] = np.nan
    x[2, 0] = np.inf
    x[3] = -np.inf
    x[4, 1:] = -np.inf
    a = np.array([0, 1, 2, 3, 0, 4, -1], np.int64)
    logp, ent, bad = ER.evaluate(x, a)
    assert bad.tolist() == [False, True, True, True, False, True, True]
    assert np.isnan(logp[bad]).all() and np.isnan(ent[bad]).all() and logp[4] == 0 and ent[4] == 0
    g = ER.evaluate_backward(x, a, np.ones(7, np.float32), np.ones(7, np.float32))
    assert np.isnan(g[bad]).all() and not np.isnan(g[~bad]).any() and (g[4] == 0).all()
    z = np.zeros(7, np.float32)
    terms, sums, bad2, _ = ER.ppo_loss(x, z, a, z, z, z, LO, HI, VC, EC)
    assert np.array_equal(bad, bad2) and np.isnan(terms[bad]).all() and np.isnan(sums).all()
    # an action in range on a masked logit is not bad: logp = -inf, r = 0
    x = np.array([[0.0, -np.inf, 1.0]], np.float32)
    logp, ent, bad = ER.evaluate(x, [1])
    assert not bad.any() and logp[0] == -np.inf and np.isfinite(ent[0])
    terms, sums, _, r = ER.ppo_loss(x, [0.0], [1], [-1.0], [2.0], [0.0], LO, HI, VC, EC)
    assert r[0] == 0 and terms[0, 0] == 0 and np.isfinite(sums).all()
    gL, _ = ER.ppo_loss_backward(x, [0.0], [1], [-1.0], [2.0], [0.0], LO, HI, VC, 0.0, 1.0)
    assert (gL == 0).all()


def test_the_tie_and_closed_range_rule_is_torchs():
    """d min(r adv, clamp(r) adv) / dr in torch's float32 autograd against the header's bracket, at the clip bounds themselves,
    one ulp either side, inside, outside, and adv of both signs and 0."""
    lo, hi = LO, HI
    rs = [lo, hi, np.nextafter(lo, np.float32(0)), np.nextafter(lo, np.float32(2)), np.nextafter(hi, np.float32(0)),
          np.nextafter(hi, np.float32(2)), np.float32(1), np.float32(0.5), np.float32(2), np.float32(0)]
    advs = [np.float32(1.5), np.float32(-1.5), np.float32(0)]
    r = np.array([x for x in rs for _ in advs], np.float32)
    adv = np.array([y for _ in rs for y in advs], np.float32)
    rt = torch.from_numpy(r).requires_grad_(True)
    at = torch.from_numpy(adv)
    torch.min(rt * at, torch.clamp(rt, float(lo), float(hi)) * at).sum().backward()
    s1, s2 = r * adv, np.clip(r, lo, hi) * adv
    passes = (s1 < s2) | ((lo <= r) & (r <= hi))
    # One kind of row is left out of the comparison: r an ulp outside the range whose product with adv ROUNDS to the bound's --
    # a tie outside the closed range with adv != 0.  torch hands on half the gradient there, the header's rule none; such a row
    # lies inside clip_margin of the bound, where the gradient jumps anyway and no GPU case has a row.
    rounding_tie = (s1 == s2) & ~((lo <= r) & (r <= hi)) & (adv != 0)
    assert rounding_tie.sum() == 2 and (np.minimum(np.abs(r - lo), np.abs(r - hi))[rounding_tie] <= ER.clip_margin(r, 21 * ER.U)[rounding_tie]).all()
    assert np.array_equal(rt.grad.numpy()[rounding_tie], adv[rounding_tie] / 2)
    assert np.array_equal(rt.grad.numpy()[~rounding_tie], np.where(passes, adv, np.float32(0))[~rounding_tie])
    # the same through the model: logp - old = log r exactly where r is 1
    x = np.zeros((1, 2), np.float32)
    logp = ER.evaluate(x, [0])[0]
    for lo1, hi1, adv1 in ((1.0, 1.0, 2.0), (1.0, 1.0, -2.0), (1.0, 1.2, 2.0), (0.8, 1.0, -2.0)):
        gL, _ = ER.ppo_loss_backward(x, [0.0], [0], logp, [adv1], [0.0], lo1, hi1, 0.0, 0.0, 1.0)
        assert gL[0, 0] == np.float32(-adv1 * 0.5) and gL[0, 1] == np.float32(adv1 * 0.5)  # -g / M adv r (1 - p), p = 1/2 exactly


def test_the_fixed_order_sums_what_fsum_sums():
    r = np.random.default_rng(0)
    for n in (1, 63, 64, 65, 255, 256, 257, 4097):
        v = r.standard_normal(n) * 10.0 ** r.integers(-3, 4, n)
        want = math.fsum(v)
        assert abs(ER.wave_tree_sum(v, n) - want) <= n * 2.0 ** -52 * np.abs(v).sum()
    v = np.arange(1, 601, dtype=np.float64)  # integers: every order is exact
    assert ER.wave_tree_sum(v, 600) == 600 * 601 / 2


def test_the_gpu_cases_keep_every_ratio_off_the_clip_bounds():
    """The gradient jumps where r crosses clip_lo or clip_hi: a row within the derived margin of one may clip differently on the
    device.  The condition on every case of tests/test_gpu_policy_eval.py: no such row."""
    for n in ER.MS:
        for A in ER.AS:
            for scale in ER.SCALES:
                x = PR.general_rows(n, A, scale, 1)
                assert ER.ratios_off_the_clip(x, ER.ppo_columns(x, ER.COLUMN_SEED)) == 0, (n, A, scale)
    for n, A in ER.BIG_CASES:
        x = PR.general_rows(n, A, 1.0, 1)
        assert ER.ratios_off_the_clip(x, ER.ppo_columns(x, ER.COLUMN_SEED)) == 0, (n, A)


def test_header_declares_what_the_binding_binds():
    import spacefortress_amd
    from spacefortress_amd import _lib as lib
    from spacefortress_amd import build as sfbuild

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "include", "sfmi_ppo.h")
    bare = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    assert set(re.findall(r"\b(sf_[a-z_0-9]+)\s*\(", bare)) == set(lib.PPO_SYMBOLS)
    for name, (_, args) in lib.PPO_SYMBOLS.items():
        m = re.search(r"\b%s\(([^)]*)\)" % name, bare)
        assert m and len(m.group(1).split(",")) == len(args), name
    assert os.path.abspath(path) in [os.path.abspath(h) for h in sfbuild.HEADERS if os.path.isabs(h)]
    assert "sf_policy_eval.hip" in sfbuild.SOURCES
    assert "evaluate_actions" in spacefortress_amd.__all__ and "ppo_loss" in spacefortress_amd.__all__


def test_the_built_library_exports_the_calls():
    from spacefortress_amd import _lib
    from spacefortress_amd import build as sfbuild

    sfbuild.build()
    L = _lib.lib()
    assert all(hasattr(L, name) for name in _lib.PPO_SYMBOLS)
    assert L.sf_ppo_loss_workspace_bytes(1) == 24 and L.sf_ppo_loss_workspace_bytes(257) == 48 and L.sf_ppo_loss_workspace_bytes(0) == 0
