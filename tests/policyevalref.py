"""The numpy model of the policy head's update side: include/sfmi_ppo.h restated, operation by operation.  No GPU, no torch.

It builds on policyref.py: the row (m, d, e, S, lse, the entropy) is policyref.policy_head's own, so that the log-probability
and the entropy of this model ARE the sampling head's.  float32 where the header says float32, float64 where it says float64;
expf and logf are numpy's float64 ones rounded to float32 (policyref.py says what that means for the bounds).

Below the model: the float64 closed forms on the same float32 inputs (`exact_*`), and the bounds of profiles/policy_eval.md as
formulas of the inputs -- never measured maxima.  A bound says how far ANY evaluation of the header's operations whose expf and
logf are within 1 ulp may lie from the closed form; the device and this model are both held to it.
"""
import numpy as np

import policyref as PR

f32, f64 = np.float32, np.float64
U = 2.0 ** -24            # float32's unit roundoff: one rounding moves a value by at most U times its magnitude
SLACK = 1.0 + 2.0 ** -10  # the second-order terms of every first-order bound below
FLOOR = 2.0 ** -120       # entries whose e[k] is subnormal or underflows: their relative bounds fail, their size is below this


def _col(t):
    return np.ascontiguousarray(t, f32).reshape(-1)


def row(logits, actions):
    """The row of the header for given actions -> dict: policyref.policy_head's (mode 1) plus a (0 where outside), outside, bad
    (the head's or an action outside [0, A)), d [n, A], p = e / Sf float32 [n, A], H float32 [n] (not NaN-ed), logp [n]."""
    x = np.ascontiguousarray(logits, f32)
    n, A = x.shape
    a = np.asarray(actions).reshape(-1).astype(np.int64)
    out = dict(PR.policy_head(x, mode=1))
    outside = (a < 0) | (a >= A)
    a = np.where(outside, 0, a)
    bad = out["bad"] | outside
    with np.errstate(all="ignore"):
        d = (out["x"] - out["m"][:, None]).astype(f32)
        Sf = out["S"].astype(f32)
        # policy_head NaNs a bad row's entropy; recompute nothing: a bad row's numbers are never looked at
        logp, _ = PR.logp_of(out, a)
        p = (out["e"] / Sf[:, None]).astype(f32)
    out.update(a=a, outside=outside, bad=bad, d=d, Sf=Sf, p=p, H=out["entropy"], logp_a=logp, n=n, A=A, masked=out["x"] == -np.inf)
    return out


def evaluate(logits, actions):
    """sf_policy_evaluate -> (logp float32 [n], entropy float32 [n], bad bool [n])"""
    R = row(logits, actions)
    nan = f32(np.nan)
    return np.where(R["bad"], nan, R["logp_a"]).astype(f32), np.where(R["bad"], nan, R["H"]).astype(f32), R["bad"]


def _row_grad(R, gl, gH):
    """the header's gradient entries from a row and the two per-row factors (float32 [n])"""
    n, A = R["n"], R["A"]
    gl, gH = _col(gl)[:, None], _col(gH)[:, None]
    with np.errstate(all="ignore"):
        delta = (np.arange(A)[None, :] == R["a"][:, None]).astype(f32)
        t1 = (gl * (delta - R["p"]).astype(f32)).astype(f32)
        w = ((R["d"] - R["lse"][:, None]).astype(f32) + R["H"][:, None]).astype(f32)
        t2 = np.where(R["e"] != 0, ((gH * R["p"]).astype(f32) * w).astype(f32), f32(0))
        g = (t1 - t2).astype(f32)
    g = np.where(R["masked"], f32(0), g)
    return np.where(R["bad"][:, None], f32(np.nan), g).astype(f32)


def evaluate_backward(logits, actions, grad_logp=None, grad_entropy=None):
    """sf_policy_evaluate_backward -> grad_logits float32 [n, A]"""
    R = row(logits, actions)
    z = np.zeros(R["n"], f32)
    return _row_grad(R, z if grad_logp is None else grad_logp, z if grad_entropy is None else grad_entropy)


def clip_bounds(clip):
    """(float32(1 - clip), float32(1 + clip)), rounded from the double"""
    return f32(1.0 - clip), f32(1.0 + clip)


def _surrogate(logp, old_logp, adv, clip_lo, clip_hi):
    with np.errstate(all="ignore"):
        r = np.exp((logp - old_logp).astype(f32).astype(f64)).astype(f32)
        c = np.where(r < clip_lo, f32(clip_lo), np.where(r > clip_hi, f32(clip_hi), r)).astype(f32)
        s1, s2 = (r * adv).astype(f32), (c * adv).astype(f32)
        s = np.where((s1 < s2) | np.isnan(s1), s1, s2)
    return r, s1, s2, s.astype(f32)


def wave_tree_sum(v, n):
    """The header's fixed order on float64 terms [n]: lane l of a wave takes lane l ^ 32, then ^ 16, ... ^ 1 (what lane 0 ends
    with); the four waves of a block of 256 in index order; the blocks in index order."""
    blocks = (n + 255) // 256
    t = np.zeros(blocks * 256, f64)
    t[:n] = v
    t = t.reshape(blocks, 4, 64)
    with np.errstate(all="ignore"):
        for off in (32, 16, 8, 4, 2, 1):
            t = t[..., :off] + t[..., off:2 * off]
        t = t[..., 0]
        per_block = ((t[:, 0] + t[:, 1]) + t[:, 2]) + t[:, 3]
        acc = f64(0)
        for b in per_block:
            acc = acc + b
    return acc


def combine(action_loss, value_loss, entropy, value_coef, entropy_coef):
    """the weighted sum, float32 on the three rounded means"""
    with np.errstate(all="ignore"):
        return f32(f32(f32(action_loss) + f32(f32(value_coef) * f32(value_loss))) - f32(f32(entropy_coef) * f32(entropy)))


def ppo_loss(logits, values, actions, old_logp, adv, returns, clip_lo, clip_hi, value_coef, entropy_coef):
    """sf_ppo_loss -> (row_terms float32 [n, 3] = (s, q, H), sums float32 [4], bad bool [n], r float32 [n])"""
    R = row(logits, actions)
    n = R["n"]
    v, old, adv, ret = _col(values), _col(old_logp), _col(adv), _col(returns)
    r, s1, s2, s = _surrogate(R["logp_a"], old, adv, f32(clip_lo), f32(clip_hi))
    with np.errstate(all="ignore"):
        dv = (v - ret).astype(f32)
        q = (dv * dv).astype(f32)
    terms = np.stack([s, q, R["H"]], 1).astype(f32)
    terms[R["bad"]] = np.nan
    with np.errstate(all="ignore"):
        tot = [wave_tree_sum(terms[:, j].astype(f64), n) for j in range(3)]
        al, vl, en = f32(-(tot[0] / f64(n))), f32(tot[1] / f64(n)), f32(tot[2] / f64(n))
    return terms, np.array([al, vl, en, combine(al, vl, en, value_coef, entropy_coef)], f32), R["bad"], r


def ppo_loss_backward(logits, values, actions, old_logp, adv, returns, clip_lo, clip_hi, value_coef, entropy_coef, g):
    """sf_ppo_loss_backward -> (grad_logits float32 [n, A], grad_values float32 [n])"""
    R = row(logits, actions)
    n = R["n"]
    v, old, adv, ret = _col(values), _col(old_logp), _col(adv), _col(returns)
    clip_lo, clip_hi = f32(clip_lo), f32(clip_hi)
    r, s1, s2, _ = _surrogate(R["logp_a"], old, adv, clip_lo, clip_hi)
    with np.errstate(all="ignore"):
        gm = f32(f32(g) / f32(n))
        passes = (s1 < s2) | ((clip_lo <= r) & (r <= clip_hi)) | np.isnan(s1) | np.isnan(s2)
        cl = np.where(passes, -(((gm * adv).astype(f32) * r).astype(f32)), f32(0)).astype(f32)
        cH = np.full(n, -f32(gm * f32(entropy_coef)), f32)
        cv = (f32(gm * f32(value_coef)) * (f32(2) * (v - ret).astype(f32)).astype(f32)).astype(f32)
    return _row_grad(R, cl, cH), np.where(R["bad"], f32(np.nan), cv).astype(f32)


# ---------------------------------------------------------------------------------------------------------------
# the float64 closed forms on the same float32 inputs
def exact_row(logits, actions):
    """-> dict(p, logp_k [n, A], logp [n], H [n]) in float64; a masked entry has p = 0 and adds nothing to H"""
    x = np.ascontiguousarray(logits, f32).astype(f64)
    a = np.asarray(actions).reshape(-1).astype(np.int64)
    with np.errstate(all="ignore"):
        m = x.max(1, keepdims=True)
        d = x - m
        lse = np.log(np.exp(d).sum(1, keepdims=True))
        logp_k = d - lse
        p = np.exp(logp_k)
        H = -np.where(p > 0, p * logp_k, 0.0).sum(1)
    return dict(p=p, logp_k=logp_k, logp=np.take_along_axis(logp_k, a[:, None], 1)[:, 0], H=H, a=a, masked=x == -np.inf)


def exact_grad(E, gl, gH):
    """grad[k] = g_l (delta(k, a) - p[k]) - g_H p[k] (logp_k + H), 0 at a masked entry"""
    gl, gH = np.asarray(gl, f64).reshape(-1, 1), np.asarray(gH, f64).reshape(-1, 1)
    delta = (np.arange(E["p"].shape[1])[None, :] == E["a"][:, None]).astype(f64)
    with np.errstate(all="ignore"):
        w = np.where(E["p"] > 0, E["logp_k"] + E["H"][:, None], 0.0)
        g = gl * (delta - E["p"]) - gH * E["p"] * w
    return np.where(E["masked"], 0.0, g)


def exact_row_sum(E, gl):
    """What a gradient row sums to: 0 (sum_k delta - p = 0 and sum_k p (logp_k + H) = 0), except where the action sits on a
    masked logit, whose own entry is held at 0 instead of g_l: there -g_l."""
    on_masked = np.take_along_axis(E["masked"], E["a"][:, None], 1)[:, 0]
    return np.where(on_masked, -np.asarray(gl, f64).reshape(-1), 0.0)


def exact_ppo(logits, values, actions, old_logp, adv, returns, clip_lo, clip_hi, value_coef, entropy_coef, g=1.0):
    """-> dict(r, s, q, H, sums [4], grad_logits, grad_values, cl, cH) in float64; the coefficients as the float32 the call gets"""
    E = exact_row(logits, actions)
    v, old, adv, ret = (_col(t).astype(f64) for t in (values, old_logp, adv, returns))
    lo, hi, vc, ec = (f64(f32(t)) for t in (clip_lo, clip_hi, value_coef, entropy_coef))
    n = v.size
    with np.errstate(all="ignore"):
        r = np.exp(E["logp"] - old)
        s1, s2 = r * adv, np.clip(r, lo, hi) * adv
        s, q = np.minimum(s1, s2), (v - ret) ** 2
        passes = (s1 < s2) | ((lo <= r) & (r <= hi))
        gm = f64(f32(g)) / n
        cl, cH = np.where(passes, -gm * adv * r, 0.0), np.full(n, -gm * ec)
        al, vl, en = -s.mean(), q.mean(), E["H"].mean()
    return dict(r=r, s=s, q=q, H=E["H"], sums=np.array([al, vl, en, al + vc * vl - ec * en]), cl=cl, cH=cH,
                grad_logits=exact_grad(E, cl, cH), grad_values=2.0 * gm * vc * (v - ret), row=E)


# ---------------------------------------------------------------------------------------------------------------
# the bounds of profiles/policy_eval.md
def p_rel_bound(A, d_abs):
    """|p'[k] - p[k]| <= p[k] * this: policyref.logp_bound(A, |d[k]|) (section 2 there; the direct count gives 3 * 2^-23)"""
    return PR.logp_bound(A, d_abs)


def grad_bound(E, A, gl, gH, dgl=0.0, dgH=0.0):
    """How far a computed gradient row may lie from exact_grad(E, gl, gH), entry by entry [n, A] (section 3): gl, gH the exact
    per-row factors, dgl, dgH how far the computed factors may lie from them (0 for sf_policy_evaluate_backward, which gets
    them as data)."""
    gl, gH = np.abs(np.asarray(gl, f64)).reshape(-1, 1), np.abs(np.asarray(gH, f64)).reshape(-1, 1)
    dgl, dgH = np.broadcast_to(np.asarray(dgl, f64).reshape(-1, 1), gl.shape), np.broadcast_to(np.asarray(dgH, f64).reshape(-1, 1), gH.shape)
    p = E["p"]
    with np.errstate(all="ignore"):
        d_abs = np.where(E["masked"], 0.0, np.abs(E["logp_k"] - E["logp_k"].max(1, keepdims=True)))
        w = np.where(p > 0, np.abs(E["logp_k"] + E["H"][:, None]), 0.0)
        ep = p_rel_bound(A, d_abs)
        el, eH = PR.logp_bound(A, d_abs), PR.entropy_bound(A)
        delta = (np.arange(p.shape[1])[None, :] == E["a"][:, None]).astype(f64)
        dp = np.abs(delta - p)
        t1, t2 = gl * dp, gH * p * w
        b = (gl * (p * ep + 2 * U * dp) + gH * p * (w * (ep + 3 * U) + el + eH) + U * (t1 + t2)
             + dgl * dp + dgH * p * w)
        b = b * SLACK + FLOOR * (gl + gH + dgl + dgH)
    return np.where(E["masked"], 0.0, b)


def ratio_rel_bound(A, xa_minus_m, logp_minus_old):
    """|r' - r| <= r * this (section 4): the log-probability's bound, the subtraction's rounding, expf's ulp and one more"""
    return (PR.logp_bound(A, xa_minus_m) + U * np.abs(logp_minus_old) + 3 * U) * SLACK


def s_bound(r, adv, clip_lo, er):
    """|s' - s| (section 4): min and clamp are 1-Lipschitz in r, each product rounds once"""
    adv = np.abs(np.asarray(adv, f64))
    return adv * (r * er + U * np.maximum(r, f64(clip_lo))) * SLACK + FLOOR


def clip_margin(r, er):
    """A row whose ratio lies further than this from clip_lo and clip_hi clips the same way in every evaluation"""
    return 2.0 * r * er


def sums_bound(terms64, n):
    """|mean' - mean| of float64 sums of the same float32 terms in any order: n * 2^-52 relative to the sum of magnitudes, and
    the one rounding to float32"""
    mean_abs = np.abs(terms64).sum() / n
    return n * 2.0 ** -52 * mean_abs + U * np.abs(terms64.sum() / n) * SLACK + 2.0 ** -149


def ppo_grad_bounds(X, A, adv, g, value_coef, xa_minus_m, logp_minus_old):
    """(bound of grad_logits [n, A], bound of grad_values [n]) against exact_ppo's X (section 5): c_l carries the ratio's bound
    and three roundings, c_H two, c_v four."""
    er = ratio_rel_bound(A, xa_minus_m, logp_minus_old)
    dcl = np.abs(X["cl"]) * (er + 3 * U) * SLACK
    dcH = np.abs(X["cH"]) * 2 * U * SLACK
    return grad_bound(X["row"], A, X["cl"], X["cH"], dcl, dcH), np.abs(X["grad_values"]) * 4 * U * SLACK + 2.0 ** -149


# ---------------------------------------------------------------------------------------------------------------
# the GPU tests' cases (here, so that the CPU suite can check what they need of the seeds)
MS, AS, SCALES = (1, 63, 64, 65, 255, 256, 257, 4097), (1, 3, 4, 5, 8, 9, 16, 17, 32), (0.1, 1.0, 10.0)
BIG_CASES = ((65537, 5), (262145, 5))
CLIP, VALUE_COEF, ENTROPY_COEF = 0.1, 0.5, 0.01
COLUMN_SEED = 1  # tests/test_policy_eval_model.py checks that no case then has a ratio within clip_margin of a clip bound


def ppo_columns(x, seed):
    """The other inputs of a loss case from its logits x [n, A]: actions of non-zero and of zero probability alike (a tenth of
    them land on a -inf logit where the row has one), old log-probabilities near the new ones (ratios on both sides of the clip
    range of CLIP = 0.1 and inside it), advantages of both signs, values and returns."""
    n, A = x.shape
    r = np.random.default_rng([seed, n, A, 77])
    finite = np.isfinite(x)
    k = r.integers(0, A, n)
    a = np.where(finite[np.arange(n), k], k, x.argmax(1)).astype(np.int64)
    on_masked = (r.random(n) < 0.1) & ~finite.all(1)
    a = np.where(on_masked, (~finite).argmax(1), a).astype(np.int64)
    logp = evaluate(x, a)[0].astype(f64)
    # log r = logp - old from three stretches, a third of the rows each: below ln 0.9, between the two clip bounds, above
    # ln 1.1 -- continuous, and clear of the two points where the gradient jumps (ratios_off_the_clip counts what is not)
    lo_hi = np.array([[-0.35, -0.115], [-0.095, 0.085], [0.105, 0.35]])[r.integers(0, 3, n)]
    log_r = lo_hi[:, 0] + (lo_hi[:, 1] - lo_hi[:, 0]) * r.random(n)
    old = np.where(np.isfinite(logp), logp - log_r, -3.0).astype(f32)
    adv = r.standard_normal(n).astype(f32)
    v, ret = r.standard_normal(n).astype(f32), (r.standard_normal(n) * 2).astype(f32)
    return a, old, adv, v, ret


def ratio_inputs(x, a, old):
    """(|x[a] - m|, logp - old_logp) as the ratio's bound takes them, 0 where the action's logit is -inf: there logp = -inf and
    r = 0 in every evaluation"""
    x64 = np.ascontiguousarray(x, f32).astype(f64)
    with np.errstate(all="ignore"):
        xa = np.abs(np.take_along_axis(x64, np.asarray(a, np.int64).reshape(-1, 1), 1)[:, 0] - x64.max(1))
        dlt = exact_row(x, a)["logp"] - _col(old).astype(f64)
    return np.where(np.isfinite(xa), xa, 0.0), np.where(np.isfinite(dlt), dlt, 0.0)


def ratios_off_the_clip(x, cols, clip=CLIP):
    """the number of rows whose ratio lies within clip_margin of clip_lo or clip_hi (the condition on a case: 0)"""
    a, old = cols[0], cols[1]
    lo, hi = clip_bounds(clip)
    xa, dlt = ratio_inputs(x, a, old)
    with np.errstate(all="ignore"):
        r = np.exp(exact_row(x, a)["logp"] - old.astype(f64))
        margin = clip_margin(r, ratio_rel_bound(x.shape[1], xa, dlt))
        near = (np.abs(r - f64(lo)) <= margin) | (np.abs(r - f64(hi)) <= margin)
    return int(near.sum())
