"""The policy head's update side on the device (include/sfmi_ppo.h: sf_policy_evaluate, sf_policy_evaluate_backward, sf_ppo_loss,
sf_ppo_loss_backward; spacefortress_amd.evaluate_actions / ppo_loss), held to the numpy model tests/policyevalref.py.

The device's expf and logf are not numpy's, so nothing is compared bit for bit where they enter, and nothing loosely where they
do not.  profiles/policy_eval.md derives the bounds (policyevalref.grad_bound / s_bound / ppo_grad_bounds / sums_bound, on top
of policyref.logp_bound / entropy_bound) from float32's roundings and a 1-ulp bound on the two functions:
  * log-probabilities and entropies lie within policyref's bounds of the model's;
  * gradients and surrogate terms lie within their bounds of the float64 closed form on the same float32 inputs (the model is held
    to the same bounds on the CPU, tests/test_policy_eval_model.py); entries at -inf logits are exactly 0; a row's entries sum to
    what the exact row sums to, within the row's bound;
  * (v - ret)^2, the weighted sum, everything about bad rows, refusals, streams and graphs, and every tie to sf_policy_sample are
    exact;
  * the means are the float64 sum of the device's OWN row terms, within n * 2^-52 and one float32 rounding, and two calls give
    equal bits.
Every buffer of a raw call is guarded (trainerref.guarded); a logits row's padding holds NaN and a gradient row's the sentinel.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import policyevalref as ER
import policyref as PR
import trainerref as TR
from lockstep import sfa  # noqa: F401  (the fixture)

LO, HI = ER.clip_bounds(ER.CLIP)
VC, EC = ER.VALUE_COEF, ER.ENTROPY_COEF
ACT_DTYPES = (torch.uint8, torch.int32, torch.int64)
ACT_TYPE = {torch.uint8: 1, torch.int32: 4, torch.int64: 8}
NP_ACT = {torch.uint8: np.uint8, torch.int32: np.int32, torch.int64: np.int64}
F = torch.float32


def vp(p):
    return C.c_void_p(p) if p else None


class Raw:
    """The buffers of the four raw calls for one case, all guarded: logits [n, stride] with NaN behind every row, the actions,
    the four columns, every output."""

    def __init__(self, x, cols, stride=None, gstride=None, act_dtype=torch.int64, g=1.0):
        from spacefortress_amd import _lib
        self.lib, self.L = _lib, _lib.lib()
        self.dev = torch.device("cuda", torch.cuda.current_device())
        self.n, self.A = x.shape
        n, A = x.shape
        self.stride, self.gstride = stride or A, gstride or A
        a, old, adv, v, ret = cols
        self.logits = TR.guarded((n, self.stride), F, self.dev)
        self.logits.fill_(float("nan"))
        self.logits[:, :A].copy_(torch.from_numpy(x))
        self.act = TR.guarded(n, act_dtype, self.dev, np.asarray(a).astype(NP_ACT[act_dtype]))
        self.old, self.adv = TR.guarded(n, F, self.dev, old), TR.guarded(n, F, self.dev, adv)
        self.v, self.ret = TR.guarded(n, F, self.dev, v), TR.guarded(n, F, self.dev, ret)
        self.gl, self.gH = TR.guarded(n, F, self.dev), TR.guarded(n, F, self.dev)
        self.gloss = TR.guarded(1, F, self.dev, np.array([g], np.float32))
        self.logp, self.ent = TR.guarded(n, F, self.dev), TR.guarded(n, F, self.dev)
        self.grad = TR.guarded((n, self.gstride), F, self.dev)
        self.gv = TR.guarded(n, F, self.dev)
        self.terms, self.sums = TR.guarded((n, 3), F, self.dev), TR.guarded(4, F, self.dev)
        ws = int(self.L.sf_ppo_loss_workspace_bytes(n))
        assert ws == 24 * ((n + 255) // 256)
        self.ws = TR.guarded(ws // 8, torch.float64, self.dev)
        self.bad = TR.guarded(1, torch.int64, self.dev, np.zeros(1, np.int64))
        self.outputs = (self.logp, self.ent, self.grad, self.gv, self.terms, self.sums, self.ws)
        self.all = self.outputs + (self.logits, self.act, self.old, self.adv, self.v, self.ret, self.gl, self.gH, self.gloss, self.bad)

    def _args(self, over):
        a = dict(logits=self.logits.data_ptr(), n=self.n, A=self.A, stride=self.stride, act=self.act.data_ptr(),
                 at=ACT_TYPE[self.act.dtype], logp=self.logp.data_ptr(), ent=self.ent.data_ptr(), bad=self.bad.data_ptr(),
                 gl=self.gl.data_ptr(), gH=self.gH.data_ptr(), grad=self.grad.data_ptr(), gstride=self.gstride,
                 v=self.v.data_ptr(), old=self.old.data_ptr(), adv=self.adv.data_ptr(), ret=self.ret.data_ptr(), lo=float(LO),
                 hi=float(HI), vc=VC, ec=EC, terms=self.terms.data_ptr(), sums=self.sums.data_ptr(), ws=self.ws.data_ptr(),
                 gloss=self.gloss.data_ptr(), gv=self.gv.data_ptr())
        a.update(over)
        return a

    def evaluate(self, **over):
        a = self._args(over)
        return self.L.sf_policy_evaluate(vp(a["logits"]), a["n"], a["A"], a["stride"], vp(a["act"]), a["at"], vp(a["logp"]),
                                         vp(a["ent"]), vp(a["bad"]), self.lib.raw_stream(self.dev))

    def evaluate_backward(self, **over):
        a = self._args(over)
        return self.L.sf_policy_evaluate_backward(vp(a["logits"]), a["n"], a["A"], a["stride"], vp(a["act"]), a["at"], vp(a["gl"]),
                                                  vp(a["gH"]), vp(a["grad"]), a["gstride"], self.lib.raw_stream(self.dev))

    def _ppo_in(self, a):
        return (vp(a["logits"]), vp(a["v"]), vp(a["act"]), vp(a["old"]), vp(a["adv"]), vp(a["ret"]), a["n"], a["A"], a["stride"],
                a["at"], a["lo"], a["hi"], a["vc"], a["ec"])

    def loss(self, **over):
        a = self._args(over)
        return self.L.sf_ppo_loss(*self._ppo_in(a), vp(a["terms"]), vp(a["sums"]), vp(a["ws"]), vp(a["bad"]),
                                  self.lib.raw_stream(self.dev))

    def loss_backward(self, **over):
        a = self._args(over)
        return self.L.sf_ppo_loss_backward(*self._ppo_in(a), vp(a["gloss"]), vp(a["grad"]), a["gstride"], vp(a["gv"]),
                                           self.lib.raw_stream(self.dev))

    def host(self, *views):
        torch.cuda.synchronize()
        TR.margins_intact(*self.all)
        assert bool(torch.isnan(self.logits[:, self.A:]).all()) and TR.untouched(self.grad[:, self.A:])
        out = [t.cpu().numpy() for t in views]
        return out[0] if len(out) == 1 else out

    def grads(self):
        return self.host(self.grad)[:, :self.A]


def within(got, want, bound, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    same_inf = np.isinf(got) & (got == want)
    with np.errstate(invalid="ignore"):
        err = np.where(same_inf, 0.0, np.abs(got - want))
    assert np.isfinite(err).all(), (what, "not finite")
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    print("%s: largest error / bound %.3f" % (what, float(ratio.max())))
    assert (err <= bound).all(), (what, float(ratio.max()))


def hold_to_model(x, cols, raw, what, g=1.0):
    """All four calls of a case against the model, the closed forms and the bounds."""
    n, A = x.shape
    a, old, adv, v, ret = cols
    E = ER.exact_row(x, a)
    xa, dlt = ER.ratio_inputs(x, a, old)
    # sf_policy_evaluate
    assert raw.evaluate() == 0
    logp, ent = raw.host(raw.logp, raw.ent)
    m_logp, m_ent, m_bad = ER.evaluate(x, a)
    assert not m_bad.any() and int(raw.bad.item()) == 0
    within(logp, m_logp, PR.logp_bound(A, xa), (what, "logp"))
    within(ent, m_ent, PR.entropy_bound(A), (what, "entropy"))
    # sf_policy_evaluate_backward under arbitrary upstream gradients
    r = np.random.default_rng([n, A, 5])
    gl, gH = r.standard_normal(n).astype(np.float32), r.standard_normal(n).astype(np.float32)
    raw.gl.copy_(torch.from_numpy(gl))
    raw.gH.copy_(torch.from_numpy(gH))
    assert raw.evaluate_backward() == 0
    grad = raw.grads()
    bound = ER.grad_bound(E, A, gl, gH)
    within(grad, ER.exact_grad(E, gl, gH), bound, (what, "evaluate grad"))
    assert (grad[x == -np.inf] == 0).all(), what
    assert (np.abs(grad.astype(np.float64).sum(1) - ER.exact_row_sum(E, gl)) <= bound.sum(1)).all(), (what, "row sums")
    # sf_ppo_loss: the per-row terms against the model and the closed form, the means against the device's own terms
    TR.refill(raw.grad)
    assert raw.loss() == 0
    terms, sums = raw.host(raw.terms, raw.sums)
    m_terms, m_sums, _, _ = ER.ppo_loss(x, v, a, old, adv, ret, LO, HI, VC, EC)
    X = ER.exact_ppo(x, v, a, old, adv, ret, LO, HI, VC, EC, g)
    er = ER.ratio_rel_bound(A, xa, dlt)
    within(terms[:, 0], X["s"], ER.s_bound(X["r"], adv, LO, er), (what, "s"))
    TR.assert_bits_equal(terms[:, 1], m_terms[:, 1], "q: no expf or logf in it")
    within(terms[:, 2], m_terms[:, 2], PR.entropy_bound(A), (what, "H"))
    assert np.array_equal(terms[:, 2].view(np.uint32), ent.view(np.uint32)), (what, "H is sf_policy_evaluate's entropy")
    for j, sign in enumerate((-1.0, 1.0, 1.0)):
        t = terms[:, j].astype(np.float64)
        assert abs(float(sums[j]) - sign * t.sum() / n) <= ER.sums_bound(t, n), (what, "mean", j)
    assert sums[3] == ER.combine(sums[0], sums[1], sums[2], VC, EC), what
    assert int(raw.bad.item()) == 0
    TR.refill(raw.sums, raw.terms, raw.ws)
    assert raw.loss() == 0
    terms2, sums2 = raw.host(raw.terms, raw.sums)
    assert np.array_equal(sums2.view(np.uint32), sums.view(np.uint32)) and np.array_equal(terms2.view(np.uint32), terms.view(np.uint32))
    # sf_ppo_loss_backward
    assert raw.loss_backward() == 0
    grad, gv = raw.grads(), raw.host(raw.gv)
    bL, bV = ER.ppo_grad_bounds(X, A, adv, g, VC, xa, dlt)
    within(grad, X["grad_logits"], bL, (what, "loss grad_logits"))
    within(gv, X["grad_values"], bV, (what, "loss grad_values"))
    assert (grad[x == -np.inf] == 0).all(), what
    assert (np.abs(grad.astype(np.float64).sum(1) - ER.exact_row_sum(E, X["cl"])) <= bL.sum(1)).all(), (what, "row sums")


@pytest.mark.gpu
@pytest.mark.parametrize("n", ER.MS)
@pytest.mark.parametrize("A", ER.AS)
def test_general_rows_equal_the_model_and_the_closed_forms(sfa, n, A):
    for j, scale in enumerate(ER.SCALES):
        x = PR.general_rows(n, A, scale, 1)
        cols = ER.ppo_columns(x, ER.COLUMN_SEED)
        raw = Raw(x, cols, stride=A + (0, 3, 1)[j], gstride=A + (2, 0, 5)[j], act_dtype=ACT_DTYPES[(j + A + n) % 3])
        hold_to_model(x, cols, raw, (n, A, scale))


@pytest.mark.gpu
@pytest.mark.parametrize("n,A", ER.BIG_CASES)
def test_many_blocks(sfa, n, A):
    x = PR.general_rows(n, A, 1.0, 1)
    cols = ER.ppo_columns(x, ER.COLUMN_SEED)
    raw = Raw(x, cols, act_dtype=ACT_DTYPES[n % 3], g=0.625)
    assert raw.ws.numel() == 3 * ((n + 255) // 256)
    hold_to_model(x, cols, raw, (n, A), g=0.625)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("A", [1, 3, 5, 16, 32])
def test_the_sampling_heads_own_actions_get_its_own_bits_back(sfa, A, mode):
    import test_gpu_policy_head as G

    n = 4097
    x = PR.general_rows(n, A, 1.0, 11)
    for dt in ACT_DTYPES:
        head = G.Raw(sfa, x, act_dtype=dt)
        assert head.call(mode=mode) == 0
        a, logp, ent, _, bad = head.host()
        assert bad == 0
        adv = np.random.default_rng(A).standard_normal(n).astype(np.float32)
        z = np.zeros(n, np.float32)
        raw = Raw(x, (a, logp, adv, z, z), act_dtype=dt)
        assert raw.evaluate() == 0
        got_logp, got_ent = raw.host(raw.logp, raw.ent)
        TR.assert_bits_equal(got_logp, logp, "logp")
        TR.assert_bits_equal(got_ent, ent, "entropy")
        # old_logp = the stored one: r == 1 exactly, so s == adv
        assert raw.loss() == 0
        TR.assert_bits_equal(raw.host(raw.terms)[:, 0], adv, "s at r == 1")
        # clip_lo = clip_hi = 1: the closed range still hands on the whole gradient
        assert raw.loss_backward(lo=1.0, hi=1.0) == 0
        clipped = raw.grads().copy()
        TR.refill(raw.grad)
        assert raw.loss_backward(lo=0.0, hi=float("inf")) == 0
        TR.assert_bits_equal(raw.grads(), clipped, "clip [1, 1] against no clip")
        assert A == 1 or (clipped != 0).any()
        X = ER.exact_ppo(x, z, a, logp, adv, z, 0.0, np.inf, VC, EC, 1.0)  # (in float64 r is not exactly 1: no clip there)
        xa, dlt = ER.ratio_inputs(x, a, logp)
        within(clipped, X["grad_logits"], ER.ppo_grad_bounds(X, A, adv, 1.0, VC, xa, dlt)[0], ("r == 1", A, mode))


@pytest.mark.gpu
@pytest.mark.parametrize("A", [1, 3, 5, 16, 32])
def test_one_finite_logit_is_exact(sfa, A):
    n = 130
    r = np.random.default_rng(A)
    x = np.full((n, A), -np.inf, np.float32)
    k = r.integers(0, A, n)
    x[np.arange(n), k] = (r.standard_normal(n) * 30).astype(np.float32)
    cols = (k, np.zeros(n, np.float32)) + tuple(r.standard_normal(n).astype(np.float32) for _ in range(3))
    raw = Raw(x, cols, act_dtype=torch.uint8)
    raw.gl.copy_(torch.from_numpy(r.standard_normal(n).astype(np.float32)))
    raw.gH.copy_(torch.from_numpy(r.standard_normal(n).astype(np.float32)))
    assert raw.evaluate() == 0 and raw.evaluate_backward() == 0
    logp, ent = raw.host(raw.logp, raw.ent)
    assert (logp == 0).all() and (ent == 0).all() and (raw.grads() == 0).all()
    TR.refill(raw.grad)
    assert raw.loss() == 0 and raw.loss_backward() == 0
    terms = raw.host(raw.terms)
    TR.assert_bits_equal(terms[:, 0], cols[2], "s at r == 1")
    assert (terms[:, 2] == 0).all() and (raw.grads() == 0).all() and int(raw.bad.item()) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("A", [1, 2, 4, 8, 16, 32])
def test_equal_logits_with_a_power_of_two_actions_are_exact(sfa, A):
    n = 257
    r = np.random.default_rng(A)
    x = np.full((n, A), 1.75, np.float32)
    a = r.integers(0, A, n)
    gl = r.standard_normal(n).astype(np.float32)
    z = np.zeros(n, np.float32)
    raw = Raw(x, (a, z, z, z, z), act_dtype=torch.int32)
    raw.gl.copy_(torch.from_numpy(gl))
    assert raw.evaluate() == 0 and raw.evaluate_backward(gH=0) == 0
    logp, ent = raw.host(raw.logp, raw.ent)
    assert np.unique(ent).size == 1 and np.array_equal(logp, -ent)
    want = np.float32(np.log(float(A)))
    assert ent[0] == 0 if A == 1 else abs(float(ent[0]) - float(want)) <= np.spacing(want)
    delta = (np.arange(A)[None, :] == a[:, None]).astype(np.float32)
    TR.assert_bits_equal(raw.grads() + np.float32(0), gl[:, None] * (delta - np.float32(1.0 / A)) + np.float32(0), "g (delta - 1/A)")


@pytest.mark.gpu
def test_zero_advantages_and_a_zero_upstream_gradient(sfa):
    n, A = 257, 5
    x = PR.general_rows(n, A, 1.0, 12)
    a, old, adv, v, ret = ER.ppo_columns(x, 3)
    # adv == 0: the policy term is gone; without an entropy bonus the logits' gradient is 0, the value's is what it was
    raw = Raw(x, (a, old, np.zeros(n, np.float32), v, ret))
    assert raw.loss_backward(ec=0.0) == 0
    assert (raw.grads() == 0).all()
    gv = raw.host(raw.gv).copy()
    full = Raw(x, (a, old, adv, v, ret))
    assert full.loss_backward() == 0
    TR.assert_bits_equal(full.host(full.gv), gv, "grad_values does not depend on adv")
    # ... and with the bonus it is the entropy's alone: sf_policy_evaluate_backward under g_entropy = -(g / M) * entropy_coef
    TR.refill(raw.grad)
    assert raw.loss_backward() == 0
    with_bonus = raw.grads().copy()
    raw.gH.fill_(float(-(np.float32(1.0) / np.float32(n)) * np.float32(EC)))
    TR.refill(raw.grad)
    assert raw.evaluate_backward(gl=0) == 0
    TR.assert_bits_equal(with_bonus + np.float32(0), raw.grads() + np.float32(0), "the entropy's share")
    assert (with_bonus != 0).any()
    # g == 0
    zero = Raw(x, (a, old, adv, v, ret), g=0.0)
    assert zero.loss_backward() == 0
    assert (zero.grads() == 0).all() and (zero.host(zero.gv) == 0).all()


def _bad_case(dt):
    n, A = 130, 5
    x = PR.general_rows(n, A, 1.0, 13)
    cols = list(ER.ppo_columns(x, 5))
    good = (x.copy(), [c.copy() for c in cols])
    nan_rows, inf_rows, empty_rows = [0, 63, 70], [64, 129], [5, 65, 100]
    for i in nan_rows:
        x[i, i % A] = np.nan
    for i in inf_rows:
        x[i, (i + 1) % A] = np.inf
    for i in empty_rows:
        x[i] = -np.inf
    outside = {torch.uint8: [A, 200, 255], torch.int32: [A, -1, -2 ** 31, 2 ** 31 - 1],
               torch.int64: [A, -1, 2 ** 32, 2 ** 32 + 1, -2 ** 63, 2 ** 63 - 1]}[dt]
    act_rows = [1, 62, 66, 127, 128, 90][:len(outside)]
    a = cols[0].astype(NP_ACT[dt])
    a[act_rows] = np.array(outside, NP_ACT[dt])
    cols[0] = a
    bad = np.zeros(n, bool)
    bad[nan_rows + inf_rows + empty_rows + act_rows] = True
    return x, cols, good, bad


@pytest.mark.gpu
@pytest.mark.parametrize("dt", ACT_DTYPES)
def test_bad_rows_read_nan_everywhere_and_are_counted(sfa, dt):
    x, cols, (gx, gcols), bad = _bad_case(dt)
    n, A = x.shape
    raw, ref = Raw(x, cols, act_dtype=dt, stride=A + 2), Raw(gx, gcols, act_dtype=dt)
    for r in (raw, ref):
        r.gl.fill_(0.5)
        r.gH.fill_(-0.25)
    assert raw.evaluate() == 0 and ref.evaluate() == 0
    (logp, ent), (logp0, ent0) = raw.host(raw.logp, raw.ent), ref.host(ref.logp, ref.ent)
    assert int(raw.bad.item()) == bad.sum() and int(ref.bad.item()) == 0
    assert np.isnan(logp[bad]).all() and np.isnan(ent[bad]).all()
    TR.assert_bits_equal(logp[~bad], logp0[~bad])
    TR.assert_bits_equal(ent[~bad], ent0[~bad])
    assert raw.evaluate(bad=0) == 0  # the counter is optional
    assert raw.evaluate_backward() == 0 and ref.evaluate_backward() == 0
    g, g0 = raw.grads(), ref.grads()
    assert np.isnan(g[bad]).all()
    TR.assert_bits_equal(g[~bad], g0[~bad])
    for r in (raw, ref):
        TR.refill(r.grad)
        assert r.loss() == 0 and r.loss_backward() == 0
    (terms, sums, gv), (terms0, sums0, gv0) = raw.host(raw.terms, raw.sums, raw.gv), ref.host(ref.terms, ref.sums, ref.gv)
    assert int(raw.bad.item()) == 2 * bad.sum() and int(ref.bad.item()) == 0  # (the backward calls do not count)
    assert np.isnan(terms[bad]).all() and np.isnan(sums).all() and np.isfinite(sums0).all()
    TR.assert_bits_equal(terms[~bad], terms0[~bad])
    g, g0 = raw.grads(), ref.grads()
    assert np.isnan(g[bad]).all() and np.isnan(gv[bad]).all()
    TR.assert_bits_equal(g[~bad], g0[~bad])
    TR.assert_bits_equal(gv[~bad], gv0[~bad])
    m_logp, m_ent, m_bad = ER.evaluate(x, cols[0])
    assert np.array_equal(m_bad, bad)


@pytest.mark.gpu
def test_refusals_launch_nothing(sfa):
    from spacefortress_amd import _lib
    n, A = 130, 5
    x = PR.general_rows(n, A, 1.0, 6)
    raw = Raw(x, ER.ppo_columns(x, 6), stride=A + 3, gstride=A + 1)
    TR.refill(raw.bad)
    shape = [dict(logits=0), dict(act=0), dict(n=0), dict(n=-5), dict(A=0), dict(A=33, stride=40, gstride=40), dict(stride=A - 1),
             dict(at=2), dict(at=0), dict(logits=raw.logits.data_ptr() + 2)]
    grads = [dict(grad=0), dict(gstride=A - 1), dict(grad=raw.grad.data_ptr() + 1)]
    cols = [dict(v=0), dict(old=0), dict(adv=0), dict(ret=0), dict(adv=raw.adv.data_ptr() + 2)]
    calls = [(raw.evaluate, "sf_policy_evaluate", shape + [dict(logp=raw.logp.data_ptr() + 2)]),
             (raw.evaluate_backward, "sf_policy_evaluate_backward", shape + grads + [dict(gl=raw.gl.data_ptr() + 2)]),
             (raw.loss, "sf_ppo_loss", shape + cols + [dict(sums=0), dict(ws=0), dict(ws=raw.ws.data_ptr() + 4)]),
             (raw.loss_backward, "sf_ppo_loss_backward", shape + cols + grads + [dict(gloss=0), dict(gv=raw.gv.data_ptr() + 2)])]
    for call, name, cases in calls:
        for over in cases:
            assert call(**over) == _lib.SF_ERR_ARG, (name, over)
            assert _lib.last_error().startswith(name + ":"), (name, over, _lib.last_error())
    torch.cuda.synchronize()
    assert TR.untouched(*raw.outputs, raw.bad)
    TR.margins_intact(*raw.all)
    with pytest.raises(ValueError, match="sf_ppo_loss"):
        _lib.check(raw.loss(ws=0))
    # the functions refuse what they can see before the call
    with pytest.raises(ValueError):
        sfa.evaluate_actions(torch.zeros(4, 33, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda"))
    with pytest.raises(ValueError):
        sfa.evaluate_actions(torch.zeros(4, 3, device="cuda"), torch.zeros(4, device="cuda"))  # float actions
    with pytest.raises(ValueError):
        sfa.evaluate_actions(torch.zeros(4, 3, device="cuda"), torch.zeros(5, dtype=torch.int64, device="cuda"))


@pytest.mark.gpu
def test_a_side_stream_and_a_captured_graph_replayed_on_changed_logits(sfa):
    n, A = 4097, 5
    x0, x1 = PR.general_rows(n, A, 1.0, 14), PR.general_rows(n, A, 1.0, 15)
    cols = ER.ppo_columns(x0, 7)
    want = []
    for x in (x0, x1):  # the default stream's results
        ref = Raw(x, cols)
        assert ref.evaluate() == 0 and ref.loss() == 0 and ref.loss_backward() == 0
        want.append([t.copy() for t in ref.host(ref.logp, ref.ent, ref.terms, ref.sums, ref.grad, ref.gv)])
    raw = Raw(x0, cols)
    views = (raw.logp, raw.ent, raw.terms, raw.sums, raw.grad, raw.gv)
    side = torch.cuda.Stream(device=raw.dev)
    side.wait_stream(torch.cuda.current_stream(raw.dev))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        assert raw.evaluate() == 0 and raw.loss() == 0 and raw.loss_backward() == 0  # a side stream, and the warm-up
        side.synchronize()
        for got, w in zip(raw.host(*views), want[0]):
            TR.assert_bits_equal(got, w, "side stream")
        TR.refill(*views)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            assert raw.evaluate() == 0 and raw.loss() == 0 and raw.loss_backward() == 0
    torch.cuda.current_stream(raw.dev).wait_stream(side)
    torch.cuda.synchronize()
    assert TR.untouched(*views)  # (capturing launches nothing)
    for rep, w in ((0, want[0]), (1, want[1]), (2, want[1])):
        if rep == 1:
            raw.logits[:, :A].copy_(torch.from_numpy(x1))
        g.replay()
        for got, ww in zip(raw.host(*views), w):
            TR.assert_bits_equal(got, ww, "replay %d" % rep)
    assert int(raw.bad.item()) == 0


# ---------------------------------------------------------------------------------------------------------------
# the autograd functions, against torch's own float32 path on the device through a small linear layer
def _layer(n, A, seed, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    h = torch.randn(n, 8, generator=g).to("cuda", dtype)
    W = (torch.randn(A, 8, generator=g) * 0.5).to("cuda", dtype).requires_grad_(True)
    b = (torch.randn(A, generator=g) * 0.5).to("cuda", dtype).requires_grad_(True)
    wv = (torch.randn(1, 8, generator=g) * 0.5).to("cuda", dtype).requires_grad_(True)
    return h, W, b, wv


def _carried(bound_rows, grad_rows, h):
    """What a bound on the rows of d loss / d logits [n, A] becomes in d loss / d W = rows^T h: the bound carried through, and
    the float32 product's own accumulation over n terms on both sides, (n + 1) * 2^-24 of the sum of magnitudes each."""
    h = np.abs(h.astype(np.float64))
    return bound_rows.T @ h + 2 * (h.shape[0] + 1) * ER.U * (np.abs(grad_rows).T @ h) * ER.SLACK


@pytest.mark.gpu
@pytest.mark.parametrize("n,A,column", [(257, 5, True), (65, 3, False), (4097, 16, True)])
def test_evaluate_actions_gradients_against_torchs_own_path(sfa, n, A, column):
    h, W, b, _ = _layer(n, A, n + A)
    g = torch.Generator().manual_seed(1)
    a = torch.randint(0, A, (n, 1) if column else (n,), generator=g).cuda()
    c1, c2 = torch.randn(n, generator=g).cuda(), torch.randn(n, generator=g).cuda()
    logits = h @ W.t() + b
    logp, ent = sfa.evaluate_actions(logits, a)
    assert logp.shape == (n, 1) and ent.shape == (n,) and logp.requires_grad and ent.requires_grad
    got = torch.autograd.grad((logp[:, 0] * c1 + ent * c2).sum(), [logits, W, b], retain_graph=True)
    probs, log_probs = torch.softmax(logits, dim=1), torch.log_softmax(logits, dim=1)
    t_logp, t_ent = log_probs.gather(1, a.view(n, 1)), -(log_probs * probs).sum(-1)
    want = torch.autograd.grad((t_logp[:, 0] * c1 + t_ent * c2).sum(), [logits, W, b])
    x, an = logits.detach().cpu().numpy(), a.view(-1).cpu().numpy()
    E = ER.exact_row(x, an)
    xa, _ = ER.ratio_inputs(x, an, np.zeros(n, np.float32))
    within(logp.detach().cpu().numpy()[:, 0], t_logp.detach().cpu().numpy()[:, 0], 2 * PR.logp_bound(A, xa), "logp")
    within(ent.detach().cpu().numpy(), t_ent.detach().cpu().numpy(), 2 * PR.entropy_bound(A), "entropy")
    rows = 2 * ER.grad_bound(E, A, c1.cpu().numpy(), c2.cpu().numpy())  # the sum of both paths' bounds
    exact = ER.exact_grad(E, c1.cpu().numpy(), c2.cpu().numpy())
    within(got[0].cpu().numpy(), want[0].cpu().numpy(), rows, "d / d logits")
    within(got[1].cpu().numpy(), want[1].cpu().numpy(), _carried(rows, exact, h.cpu().numpy()), "d / d W")
    within(got[2].cpu().numpy(), want[2].cpu().numpy(), _carried(rows, exact, np.ones((n, 1)))[:, 0], "d / d b")
    # only one output used: the other's gradient is absent, not a tensor of zeros
    only = torch.autograd.grad(sfa.evaluate_actions(logits, a)[1].sum(), logits)[0].cpu().numpy()
    within(only, ER.exact_grad(E, np.zeros(n), np.ones(n)), ER.grad_bound(E, A, np.zeros(n), np.ones(n)), "entropy alone")
    assert sfa.evaluate_actions.check() == 0


def _torch_ppo(logits, values, a, old, adv, ret, clip, vc, ec):
    """rl/networks.py:82-85 and rl/train.py:123-129, literally"""
    probs, log_probs = torch.softmax(logits, dim=1), torch.log_softmax(logits, dim=1)
    action_log_probs = log_probs.gather(1, a)
    dist_entropy = -(log_probs * probs).sum(-1).mean()
    ratio = torch.exp(action_log_probs - old)
    surr1 = ratio * adv
    surr2 = torch.clamp(ratio, 1.0 - clip, 1.0 + clip) * adv
    action_loss = -torch.min(surr1, surr2).mean()
    value_loss = (values - ret).pow(2).mean()
    return action_loss + vc * value_loss - ec * dist_entropy, action_loss, value_loss, dist_entropy


@pytest.mark.gpu
@pytest.mark.parametrize("n,A,column", [(257, 5, True), (65, 3, False), (4097, 16, True)])
def test_ppo_loss_and_its_gradients_against_torchs_own_path(sfa, n, A, column):
    h, W, b, wv = _layer(n, A, 3 * n + A)
    logits, values = h @ W.t() + b, h @ wv.t()
    x = logits.detach().cpu().numpy()
    an, old, adv, _, ret = ER.ppo_columns(x, 8)
    assert ER.ratios_off_the_clip(x, (an, old)) == 0
    shape = (n, 1) if column else (n,)
    dev = lambda t: torch.from_numpy(np.asarray(t)).cuda().view(shape)
    a_t, old_t, adv_t, ret_t = dev(an), dev(old), dev(adv), dev(ret)
    v_in = values if column else values.view(n)
    got = sfa.ppo_loss(logits, v_in, a_t, old_t, adv_t, ret_t, ER.CLIP, VC, EC)
    assert all(t.shape == () and t.dtype == torch.float32 for t in got)
    assert got[0].requires_grad and not any(t.requires_grad for t in got[1:])
    col = lambda t: t.view(n, 1)
    want = _torch_ppo(logits, values, col(a_t), col(old_t), col(adv_t), col(ret_t), ER.CLIP, VC, EC)
    g_got = torch.autograd.grad(got[0], [logits, values, W, b, wv], retain_graph=True)
    g_want = torch.autograd.grad(want[0], [logits, values, W, b, wv])
    vn = values.detach().cpu().numpy()[:, 0]
    X = ER.exact_ppo(x, vn, an, old, adv, ret, LO, HI, VC, EC, 1.0)
    xa, dlt = ER.ratio_inputs(x, an, old)
    er = ER.ratio_rel_bound(A, xa, dlt)
    # the three means: both paths' per-row bounds, averaged, and torch's float32 sum of n terms
    rows = [ER.s_bound(X["r"], adv, LO, er), 3 * ER.U * X["q"] * ER.SLACK, np.full(n, PR.entropy_bound(A))]
    mags = [np.abs(X["s"]), X["q"], np.abs(X["H"])]
    tol = [2 * r.mean() + (n + 2) * ER.U * m.mean() * ER.SLACK for r, m in zip(rows, mags)]
    tol.append(tol[0] + VC * tol[1] + EC * tol[2] + 4 * ER.U * (abs(X["sums"][0]) + VC * X["sums"][1] + EC * X["sums"][2]))
    for j, k in enumerate((1, 2, 3, 0)):  # X["sums"]: action, value, entropy, loss; the functions return the loss first
        assert abs(float(got[k]) - float(want[k])) <= tol[j], (j, float(got[k]), float(want[k]), tol[j])
        assert abs(float(got[k]) - X["sums"][j]) <= tol[j], (j, float(got[k]), X["sums"][j], tol[j])
    bL, bV = ER.ppo_grad_bounds(X, A, adv, 1.0, VC, xa, dlt)
    within(g_got[0].cpu().numpy(), g_want[0].cpu().numpy(), 2 * bL, "d / d logits")
    within(g_got[1].cpu().numpy()[:, 0], g_want[1].cpu().numpy()[:, 0], 2 * bV, "d / d values")
    hn = h.cpu().numpy()
    within(g_got[2].cpu().numpy(), g_want[2].cpu().numpy(), _carried(2 * bL, X["grad_logits"], hn), "d / d W")
    within(g_got[3].cpu().numpy(), g_want[3].cpu().numpy(), _carried(2 * bL, X["grad_logits"], np.ones((n, 1)))[:, 0], "d / d b")
    within(g_got[4].cpu().numpy(), g_want[4].cpu().numpy(), _carried(2 * bV[:, None], X["grad_values"][:, None], hn), "d / d wv")
    assert sfa.ppo_loss.check() == 0


@pytest.mark.gpu
def test_the_functions_convert_what_is_not_dense_float32_and_count_bad_rows(sfa):
    n, A = 130, 5
    x = PR.general_rows(n, A, 1.0, 16)
    an, old, adv, v, ret = ER.ppo_columns(x, 9)
    dev = lambda t: torch.from_numpy(np.asarray(t)).cuda()
    xs = dev(x)
    args = (dev(v), dev(an), dev(old), dev(adv), dev(ret), ER.CLIP, VC, EC)
    want_eval = sfa.evaluate_actions(xs, dev(an))
    want_loss = sfa.ppo_loss(xs, *args)
    lg = xs.clone().requires_grad_(True)
    vg = dev(v).requires_grad_(True)
    sfa.ppo_loss(lg, vg, *args[1:])[0].backward()
    # float64 logits: converted on the way in, the gradient back in float64
    leaf = xs.double().requires_grad_(True)
    assert all(torch.equal(p, q) for p, q in zip(sfa.evaluate_actions(leaf, dev(an).int()), want_eval))
    loss = sfa.ppo_loss(leaf, *args)
    assert all(torch.equal(p, q) for p, q in zip(loss, want_loss))
    loss[0].backward()
    assert leaf.grad.dtype == torch.float64 and torch.equal(leaf.grad, lg.grad.double())
    # columns that are not contiguous in memory
    turned = xs.t().contiguous().t()
    assert not turned.is_contiguous()
    assert all(torch.equal(p, q) for p, q in zip(sfa.evaluate_actions(turned, dev(an)), want_eval))
    assert all(torch.equal(p, q) for p, q in zip(sfa.ppo_loss(turned, *args), want_loss))
    wide = torch.zeros(n, A + 3, device="cuda")
    wide[:, :A] = xs
    # a strided view as the graph's own tensor: the gradient lands in the wide leaf's columns
    wl = wide.clone().requires_grad_(True)
    sfa.ppo_loss(wl[:, :A], *args)[0].backward()
    assert torch.equal(wl.grad[:, :A], lg.grad) and bool((wl.grad[:, A:] == 0).all())
    # uint8 actions, [M] and [M, 1] columns
    col = [t.view(n, 1) if torch.is_tensor(t) else t for t in args]
    col[1] = col[1].to(torch.uint8)
    assert all(torch.equal(p, q) for p, q in zip(sfa.ppo_loss(xs, *col), want_loss))
    # bad rows: counted by both functions, read by check() once
    assert sfa.ppo_loss.check() == 0
    broken = xs.clone()
    broken[3, 1] = float("nan")
    broken[77] = float("-inf")
    acts = dev(an).clone()
    acts[100] = A
    logp, ent = sfa.evaluate_actions(broken, acts)
    assert bool(torch.isnan(logp[[3, 77, 100]]).all()) and int(torch.isnan(ent).sum()) == 3
    loss = sfa.ppo_loss(broken, args[0], acts, *args[2:])
    assert all(bool(torch.isnan(t)) for t in loss)
    assert sfa.evaluate_actions.check() == 6 and sfa.ppo_loss.check() == 0


@pytest.mark.gpu
def test_the_example_trains_with_the_loss_head_on_the_device(sfa):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = subprocess.run([sys.executable, os.path.join(root, "examples", "ppo_loop.py"), "--device-policy-head", "--envs", "256",
                          "--steps", "8", "--iters", "2"], cwd=root, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if "last minibatch:" in l]
    assert lines, out.stdout[-2000:]
    nums = [float(v) for v in re.findall(r"(?:loss|entropy) (-?[0-9.]+(?:e-?\d+)?|nan|inf)", lines[-1])]
    assert len(nums) == 4 and all(np.isfinite(nums)) and lines[-1].rstrip().endswith("bad rows 0"), lines[-1]
