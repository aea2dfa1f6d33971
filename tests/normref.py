"""TEST INFRASTRUCTURE ONLY -- exact reference and derived error bounds for the device VecNormalize
(sf_normalize.hip, norm_partials_wave in sf_kernels.hip).

oracle/vecnorm_np.py stays the statement of the algorithm.  This file restates it with
  * the batch mean and population variance computed two-pass in numpy.longdouble (64-bit significand, pairwise
    sums along contiguous columns: relative error below 2^-58, i.e. below u / 32),
  * the parallel-variance merge done in longdouble,
  * `ret = ret * gamma + rew` and `count += n` kept in float64: one IEEE multiply and add per element and one add
    per call, no summation.  The kernels are built without FMA contraction, so these two are bit-exact and are
    compared exactly,
and carries, next to every statistic, a bound on |kernel value - exact value| obtained by running error analysis
of the kernels' own sequence of float64 operations (u = 2^-53):

  sum      |S^ - S| <= gamma_d     * sum|x|       gamma_d = d u / (1 - d u), d = the longest chain of dependent
  sumsq    |Q^ - Q| <= gamma_(d+1) * sum x^2      float64 additions of the launch (one more rounding for x * x)
  a (+) b  e = ea + eb + u (|a + b| + ea + eb)
  a (*) b  e = |a| eb + |b| ea + ea eb, then rounded as above
  a (/) b  e = (ea + |a / b| eb) / (|b| - eb), then rounded
  sqrt a   e = sqrt(a) - sqrt(max(a - ea, 0)), then rounded

in the order the kernels evaluate them: bmean = S / n; bvar = max(Q / n - bmean^2, 0); delta = bmean - mean;
mean' = mean + delta * n / tot; var' = (var * count + bvar * n + delta * delta * count * n / tot) / tot;
out = clip((x - mean') * (1 / sqrt(var' + eps))).  The clamp of bvar at 0 is a projection onto a set that holds the
exact value, so it never adds error, and it caps the error BELOW at the exact bvar itself: the variance therefore
carries a lower and an upper bound (a constant column may not push the running variance down).
Float32 outputs add half a float32 ulp of the reference value, float64 outputs one float64 ulp.  Tests allow
MARGIN = 2 times the bound, for the rounding of the bound's own arithmetic and of the longdouble reference; nothing
here is tuned to a kernel's result.

`one_pass=False` swaps the single line that bounds bvar for the two-pass one (numpy's np.var, or a kernel that
re-derives its sums about a shift): that line is `_bvar_err`.
"""
import ctypes as C
import math

import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps < 2.0 ** -60, "the exact reference needs an extended-precision long double"
U = 2.0 ** -53
MARGIN = 2.0


def gamma_d(d):
    return LD(d) * U / (1 - LD(d) * U)


# ---------------------------------------------------------------------------------------------------------------
# depth of the longest chain of dependent float64 additions, from the code
def ceil_div(a, b):
    return -(-a // b)


def depth_standalone(n, dim):
    """sf_norm_reduce_kernel + sf_norm_merge_kernel.
    rows per lane: a wave takes chunks of 64 rows, 1024 waves stride over them (ceil(chunks / 1024) per wave); in
                   a chunk a lane adds every groups-th row, groups = 64 // dim: ceil(64 / groups) rows;
    group fold:    `groups` additions into ts (starting from 0);
    four waves:    (w0 + w1) + (w2 + w3): 2;
    merge thread:  256 rows of partials over 256 threads: 1 addition into s = 0;
    butterfly:     6 xor-shuffle steps, then (p0 + p1) + (p2 + p3): 2.
    The returns: one row per lane and chunk, the butterfly (6) in place of the group fold."""
    chunks = ceil_div(n, 64)
    per_wave = ceil_div(chunks, 1024)
    groups = 64 // dim
    tail = 2 + 1 + 6 + 2
    return per_wave * ceil_div(64, groups) + groups + tail, per_wave + 6 + tail


def depth_fused(n, dim):
    """norm_partials_wave + sf_norm_merge_kernel: a wave sums its own 64 rows (ceil(64 / groups) per lane, group fold),
    one row of partials per wave of the padded batch (at most ceil(n / 256) * 4 rows), ceil(rows / 256) additions per
    merge thread, butterfly 6, four parts 2.  The returns: butterfly 6 in the wave."""
    groups = 64 // dim
    rows = ceil_div(n, 256) * 4
    tail = ceil_div(rows, 256) + 6 + 2
    return ceil_div(64, groups) + groups + tail, 6 + tail


# ---------------------------------------------------------------------------------------------------------------
# running error analysis on (value, bound) pairs; values are the exact ones (longdouble)
def _rnd(v, e, ulps=0.5):
    return e + 2 * ulps * U * (np.abs(v) + e)


def _add(a, b):
    v = a[0] + b[0]
    return v, _rnd(v, a[1] + b[1])


def _sub(a, b):
    v = a[0] - b[0]
    return v, _rnd(v, a[1] + b[1])


def _mul(a, b):
    v = a[0] * b[0]
    return v, _rnd(v, np.abs(a[0]) * b[1] + np.abs(b[0]) * a[1] + a[1] * b[1])


def _div(a, b, ulps=0.5):
    v = a[0] / b[0]
    den = np.abs(b[0]) - b[1]
    with np.errstate(divide="ignore", invalid="ignore"):  # a divisor that may be 0: no bound
        e = np.where(den > 0, (a[1] + np.abs(v) * b[1]) / np.where(den > 0, den, 1), np.inf)
    return v, _rnd(v, e, ulps)


def _sqrt(a, ulps=0.5):
    v = np.sqrt(a[0])
    return v, _rnd(v, v - np.sqrt(np.maximum(a[0] - a[1], 0)), ulps)


def _exact(v):
    v = np.asarray(v, LD)
    return v, np.zeros_like(v)


def _bvar_err(one_pass, d, n, absmean, sq, bm, ebm, bv, meanabsdev):
    """Bound on the batch variance.  One-pass: (Q^ / n) - bm^ * bm^, both of the size of mean(x^2).
    Two-pass: sum((x - bm^)^2) / n -- every term carries bm^'s error and one rounding, the sum gamma_(d+1)."""
    if one_pass:
        q = _div((sq, gamma_d(d + 1) * sq), _exact(n))
        b2 = _mul((bm, ebm), (bm, ebm))
        return _rnd(bv, q[1] + b2[1])
    e_c = ebm + U * (meanabsdev + ebm)  # per centred term, on average
    return _rnd(bv, 2 * meanabsdev * e_c + e_c * e_c + (gamma_d(d + 2) + 2 * U) * bv)


class ExactRMS:
    """RunningMeanStd with exact batch moments; em / ev_lo / ev_hi bound what a float64 evaluation may be off by."""

    def __init__(self, k, epsilon=1e-4):
        self.mean, self.var, self.count = np.zeros(k, LD), np.ones(k, LD), epsilon
        self.em, self.ev_lo, self.ev_hi = np.zeros(k, LD), np.zeros(k, LD), np.zeros(k, LD)

    def copy_state(self):
        return (self.mean.copy(), self.var.copy(), self.count, self.em.copy(), self.ev_lo.copy(), self.ev_hi.copy())

    def set_state(self, st):
        self.mean, self.var, self.count, self.em, self.ev_lo, self.ev_hi = [s.copy() if hasattr(s, "copy") else s for s in st]

    def load(self, mean, var, count):
        """sf_normalizer_set_state: the float64 values given ARE the state, so they carry no error."""
        k = self.mean.shape[0]
        self.mean, self.var, self.count = np.broadcast_to(np.asarray(mean, LD), (k,)).copy(), np.broadcast_to(np.asarray(var, LD), (k,)).copy(), float(count)
        self.em, self.ev_lo, self.ev_hi = np.zeros(k, LD), np.zeros(k, LD), np.zeros(k, LD)

    def update(self, x, d, one_pass=True):
        """x: float64 [n, k] (the exact inputs); d: depth of the summation."""
        n = x.shape[0]
        xt = np.ascontiguousarray(x.reshape(n, -1).T).astype(LD)  # [k, n]: the sums below run pairwise along n
        s = xt.sum(-1)
        bm = s / n
        c = xt - bm[:, None]
        mad = np.abs(c).sum(-1) / n
        bv = (c * c).sum(-1) / n
        del c
        a = np.abs(xt).sum(-1)
        sq = (xt * xt).sum(-1)
        del xt
        bmean = _div((s, gamma_d(d) * a), _exact(n))
        ebv = _bvar_err(one_pass, d, n, a / n, sq, bmean[0], bmean[1], bv, mad)
        ebv_lo = np.minimum(ebv, bv)  # the clamp at 0: never below zero, and the exact value is >= 0
        mean, cnt, nn = (self.mean, self.em), _exact(self.count), _exact(n)
        tot64 = self.count + float(n)  # float64, as the kernel and the oracle add it
        tot = _exact(tot64)
        delta = _sub(bmean, mean)
        nmean = _add(mean, _div(_mul(delta, nn), tot))
        d3 = _div(_mul(_mul(_mul(delta, delta), cnt), nn), tot)

        def chain(ev, eb):
            m2 = _add(_add(_mul((self.var, ev), cnt), _mul((bv, eb), nn)), d3)
            return _div(m2, tot)

        hi, lo = chain(self.ev_hi, ebv), chain(self.ev_lo, ebv_lo)
        self.mean, self.em = nmean
        self.var, self.ev_hi, self.ev_lo = hi[0], hi[1], lo[1]
        self.count = tot64
        self.last_kappa = sq / n / np.maximum(bv, np.finfo(np.float64).tiny)  # mean(x^2) / var of the batch

    # what the tests compare the device statistics with
    def stats_tol(self):
        return {"mean": (self.mean, self.em, self.em), "var": (self.var, self.ev_lo, self.ev_hi)}


def _ulp(ref, e, dtype):
    """The final cast: half a float32 ulp, or one float64 ulp, of the reference value (taken at |ref| + e: the value
    that is rounded may lie in the binade above)."""
    mag = np.abs(ref) + e
    if dtype == np.float32:
        return 0.5 * np.spacing(mag.astype(np.float32)).astype(np.float64)
    return np.spacing(mag.astype(np.float64))


def _apply(x, mean, em, var, ev, eps, clip, dtype, centre=True):
    """clip((x - mean) * (1 / sqrt(var + eps))) and its bound, per element.  x float64 [n, k]; statistics [k]."""
    inv = _div(_exact(np.ones_like(var)), _sqrt(_add((var, ev), _exact(eps)), 1.0), 1.0)  # sqrt, 1 / x: within 1 ulp
    wt = LD if dtype == np.float64 else np.float64  # (float32 outputs: float64 is 2^29 finer than their ulp)
    xv = x.astype(wt)
    if centre:
        t = xv - mean.astype(wt)
        et = _rnd(t, em.astype(wt))
    else:
        t, et = xv, wt(0)
    y = t * inv[0].astype(wt)
    with np.errstate(invalid="ignore"):
        ey = _rnd(y, np.abs(t) * inv[1].astype(wt) + np.abs(inv[0].astype(wt)) * et + et * inv[1].astype(wt))
    ref = np.clip(y, -clip, clip)  # a projection: the bound holds through it
    with np.errstate(invalid="ignore"):
        ey = np.asarray(ey, np.float64)
    ey = np.where(ey <= 2 * clip, ey, 2 * clip)  # (and two values in [-clip, clip] are never further apart; nan: 0 * inf)
    ref64 = np.asarray(ref, np.float64)
    # the reference stays unrounded (float64): two values rounded to float32 separately may differ by a whole ulp
    return ref64, ey + _ulp(ref64, ey, dtype)


class ExactVecNormalize:
    """oracle/vecnorm_np.VecNormalize, exact, with bounds.  Filter form: feed it what the wrapped vec-env returned."""

    def __init__(self, num_envs, dim, ob=True, ret=True, clipob=10., cliprew=10., gamma=0.99, epsilon=1e-8, one_pass=True):
        self.n, self.dim = num_envs, dim
        self.ob_rms = ExactRMS(dim) if ob else None
        self.ret_rms = ExactRMS(1) if ret else None
        self.clipob, self.cliprew, self.gamma, self.epsilon, self.one_pass = clipob, cliprew, gamma, epsilon, one_pass
        self.ret = np.zeros(num_envs)

    def load(self, stats, ret=None):
        """sf_normalizer_set_state with the C ABI's state vector (and the per-env returns)"""
        d = self.dim
        if self.ob_rms:
            self.ob_rms.load(stats[:d], stats[d:2 * d], stats[2 * d + 2])
        if self.ret_rms:
            self.ret_rms.load(stats[2 * d], stats[2 * d + 1], stats[2 * d + 3])
        if ret is not None:
            self.ret = np.array(ret, np.float64)

    def obfilt(self, obs, dtype, d=None, update=True):
        """-> (reference output, float64 and not rounded to `dtype`; allowed absolute error per element of a `dtype` result)"""
        if not self.ob_rms:
            return np.asarray(obs, np.float64), np.zeros(obs.shape)
        x = np.asarray(obs, np.float64)
        if update:
            self.ob_rms.update(x, d, self.one_pass)
        r = self.ob_rms
        return _apply(x, r.mean, r.em, r.var, np.maximum(r.ev_lo, r.ev_hi), self.epsilon, self.clipob, dtype)

    def rewfilt(self, rews, d=None, update=True):
        if not self.ret_rms:
            return None, None
        rw = np.asarray(rews, np.float64)
        if update:
            self.ret = self.ret * self.gamma + rw  # float64, two roundings: what the kernels do, bit for bit
            self.ret_rms.update(self.ret[:, None], d, self.one_pass)
        r = self.ret_rms
        return _apply(rw[:, None], r.mean, r.em, r.var, np.maximum(r.ev_lo, r.ev_hi), self.epsilon, self.cliprew, np.float32,
                      centre=False)

    def step(self, obs, rews, dtype, d_ob, d_ret, update=True):
        """One VecNormalize.step_wait.  -> obs_ref, obs_tol, rew_ref [n], rew_tol [n] (None, None without ret)"""
        o, eo = self.obfilt(obs, dtype, d_ob, update)
        r, er = self.rewfilt(rews, d_ret, update)
        if r is not None:
            r, er = r[:, 0], er[:, 0]
        return o, eo, r, er


# ---------------------------------------------------------------------------------------------------------------
# comparisons; every ratio |got - ref| / bound is kept for the record (profiles/norm_tests.md), never asserted beyond
# MARGIN
RECORD = {}


def _note(family, what, ratio, abserr):
    k = (family, what)
    old = RECORD.get(k, (0.0, 0.0))
    RECORD[k] = (max(old[0], float(ratio)), max(old[1], float(abserr)))


def check(family, what, got, ref, tol, tol_lo=None, where=""):
    """|got - ref| <= MARGIN * tol elementwise (tol_lo: a separate bound for got < ref).  Where the bound is 0 the
    values must be equal."""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, (family, what, got.shape, ref.shape)
    wt = LD if (got.dtype == np.float64 or ref.dtype == LD) else np.float64
    diff = got.astype(wt) - ref.astype(wt)
    assert np.all(np.isfinite(np.asarray(diff, np.float64))), (family, what, where, "not finite")
    tol = np.broadcast_to(np.asarray(tol, wt), diff.shape)
    lim = tol if tol_lo is None else np.where(diff < 0, np.broadcast_to(np.asarray(tol_lo, wt), diff.shape), tol)
    ad = np.abs(diff)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(ad == 0, 0, ad / lim)
    worst = float(np.max(ratio)) if ratio.size else 0.0
    _note(family, what, worst, float(np.max(ad)) if ad.size else 0.0)
    if not worst <= MARGIN:
        i = np.unravel_index(int(np.argmax(ratio)), ratio.shape) if ratio.ndim else ()
        raise AssertionError("%s %s %s: |got - ref| = %.3e at %s, %.2f x the derived bound %.3e (got %r, ref %r); %d of %d over"
                             % (family, what, where, float(ad[i]), i, worst, float(lim[i]), got[i], ref[i],
                                int(np.sum(ratio > MARGIN)), ratio.size))
    return worst


def check_stats(family, model, stats, ret=None, where=""):
    """stats: the C ABI's state vector [2 D + 4]; ret: the per-env returns.  Counts and returns exactly."""
    d = model.dim
    if model.ob_rms:
        r = model.ob_rms
        check(family, "ob_mean", stats[:d], r.mean, r.em, where=where)
        check(family, "ob_var", stats[d:2 * d], r.var, r.ev_hi, r.ev_lo, where=where)
        assert stats[2 * d + 2] == r.count, (family, where, "ob count", stats[2 * d + 2], r.count)
    if model.ret_rms:
        r = model.ret_rms
        check(family, "ret_mean", stats[2 * d:2 * d + 1], r.mean, r.em, where=where)
        check(family, "ret_var", stats[2 * d + 1:2 * d + 2], r.var, r.ev_hi, r.ev_lo, where=where)
        assert stats[2 * d + 3] == r.count, (family, where, "ret count", stats[2 * d + 3], r.count)
    if ret is not None:
        assert np.array_equal(ret, model.ret), (family, where, "ret differs in %d envs" % int(np.sum(ret != model.ret)))


def record_lines():
    return ["NORMREC %-28s %-9s ratio %.4f  abs %.3e" % (f, w, r, a) for (f, w), (r, a) in sorted(RECORD.items())]


# ---------------------------------------------------------------------------------------------------------------
# inputs, fixed seeds.  Every generator returns float64 arrays that hold values of `dtype` exactly.
OBS_KINDS = ("game", "unit", "constant", "clipping", "ill-1e-2", "ill-3e-4")
WELL_CONDITIONED = ("game", "unit", "constant", "clipping")
REW_KINDS = ("game", "zero", "equal", "big")
_CONST = (355.1, 0.0, 1.0, -3.5, 710.0, 1e-3, 0.1, -180.0)


def gen_obs(kind, n, dim, step, dtype=np.float32, seed=0):
    rng = np.random.default_rng([seed, OBS_KINDS.index(kind), n, dim, step])
    if kind == "game":  # positions, velocities, angles, small integers, column by column
        x = np.empty((n, dim))
        for f in range(dim):
            x[:, f] = (rng.uniform(0, 710, n), rng.uniform(-8, 8, n), rng.uniform(0, 360, n),
                       rng.integers(0, 11, n).astype(np.float64))[f % 4]
    elif kind == "unit":
        x = rng.standard_normal((n, dim))
    elif kind == "constant":
        x = np.tile(np.array([_CONST[f % len(_CONST)] for f in range(dim)]), (n, 1))
    elif kind == "clipping":
        x = rng.standard_normal((n, dim))
        k = max(1, min(5, n // 8))
        rows = rng.choice(n, k, replace=False)
        x[rows] = 50.0 * rng.choice([-1.0, 1.0], (k, dim))
    elif kind in ("ill-1e-2", "ill-3e-4"):
        x = 1000.0 + float(kind[4:]) * rng.standard_normal((n, dim))
    else:
        raise ValueError(kind)
    return x.astype(dtype).astype(np.float64)


def gen_rew(kind, n, step, seed=0):
    rng = np.random.default_rng([seed, 100 + REW_KINDS.index(kind), n, step])
    if kind == "game":
        r = rng.choice(np.array([-1, 0, 0, 0, 0, 1, 2, 100], np.int32), n)
    elif kind == "zero":
        r = np.zeros(n, np.int32)
    elif kind == "equal":
        r = np.full(n, 3, np.int32)
    elif kind == "big":
        r = rng.integers(-2, 3, n).astype(np.int32)
        k = max(1, min(6, n // 4))
        r[rng.choice(n, k, replace=False)] = rng.choice(np.array([-1000000, 1000000], np.int32), k)
    else:
        raise ValueError(kind)
    return r.astype(np.int32)


def ill_start(kind, dim):
    """The ill-conditioned inputs show only once the running variance has come down to the data's own (a fresh
    normaliser's first merge leaves mean^2 * 1e-4 / n in it for thousands of steps): they start from the state of a
    long-trained normaliser, loaded through set_state.  -> the C ABI's state vector [2 dim + 4]"""
    sd = float(kind[4:])
    return np.concatenate([np.full(dim, 1000.0), np.full(dim, sd * sd), [0.0, 1.0, 1e6, 1e-4]])


# ---------------------------------------------------------------------------------------------------------------
# a float64 one-pass evaluation in numpy, in the kernels' order of operations after the sums: for the soundness test
def numpy_pairwise_depth(n):
    """np.add.reduce along a contiguous axis: blocks of 128 with 8 accumulators (16 additions each, 3 to combine),
    halved recursively above that."""
    return 19 + max(0, math.ceil(math.log2(max(n, 1) / 128.0))) + 1


class OnePassF64:
    def __init__(self, n, dim, order, clipob=10., cliprew=10., gamma=0.99, epsilon=1e-8):
        self.st = [np.zeros(dim), np.ones(dim), 1e-4]
        self.rst = [np.zeros(1), np.ones(1), 1e-4]
        self.order, self.ret = order, np.zeros(n)
        self.clipob, self.cliprew, self.gamma, self.epsilon = clipob, cliprew, gamma, epsilon

    def depth(self, n):
        return numpy_pairwise_depth(n) if self.order == "pairwise" else n

    def _sum(self, xt):
        if self.order == "pairwise":
            return xt.sum(-1)
        if self.order == "forward":
            return np.cumsum(xt, -1)[:, -1]
        return np.cumsum(xt[:, ::-1], -1)[:, -1]

    def _update(self, st, x):
        n = x.shape[0]
        xt = np.ascontiguousarray(x.T)
        s, q = self._sum(xt), self._sum(xt * xt)
        bm = s / n
        bv = np.maximum(q / n - bm * bm, 0)
        mean, var, count = st
        delta, tot = bm - mean, count + n
        st[0] = mean + delta * n / tot
        st[1] = (var * count + bv * n + delta * delta * count * n / tot) / tot
        st[2] = tot

    def step(self, obs, rews, dtype):
        self.ret = self.ret * self.gamma + rews
        self._update(self.st, obs)
        o = np.clip((obs - self.st[0]) * (1.0 / np.sqrt(self.st[1] + self.epsilon)), -self.clipob, self.clipob).astype(dtype)
        self._update(self.rst, self.ret[:, None])
        r = np.clip(rews * (1.0 / np.sqrt(self.rst[1] + self.epsilon)), -self.cliprew, self.cliprew).astype(np.float32)
        return o, r


# ---------------------------------------------------------------------------------------------------------------
# the device side of the GPU tests: one sf_normalizer through ctypes, with guarded outputs
PATTERN = -777.25  # guard rows and untouched outputs
GUARD = 4


class Norm:
    """One sf_normalizer and guarded output tensors."""

    def __init__(self, lib, n, dim, f64=False, ob=True, ret=True):
        import torch
        from spacefortress_amd.vecnormalize import _Params
        self.lib, self.L, self.n, self.dim, self.f64 = lib, lib.lib(), n, dim, f64
        self.dev = torch.device("cuda", torch.cuda.current_device())
        self.tdt, self.ndt = (torch.float64, np.float64) if f64 else (torch.float32, np.float32)
        p = _Params(n, dim, self.dev.index, int(f64), int(ob), int(ret), 10., 10., 0.99, 1e-8)
        self.h = C.c_void_p()
        lib.check(self.L.sf_normalizer_create(C.byref(p), C.byref(self.h)))
        # guard rows in front of and behind every output (GUARD rows are a multiple of 16 bytes for every dim: the step
        # kernel's fast observation writer needs its output 16-byte aligned)
        self._obs_g = torch.full((n + 2 * GUARD, dim), PATTERN, dtype=self.tdt, device=self.dev)
        self._rew_g = torch.full((n + 128,), PATTERN, dtype=torch.float32, device=self.dev)
        self.obs_out, self.rew_out = self._obs_g[GUARD:-GUARD], self._rew_g[64:-64]

    def close(self):
        self.L.sf_normalizer_destroy(self.h)

    def stream(self):
        return self.lib.raw_stream(self.dev)

    def dev_obs(self, x):
        """float64 host values -> a guarded device tensor of the normaliser's dtype"""
        import torch
        g = torch.full((self.n + 2, self.dim), PATTERN, dtype=self.tdt, device=self.dev)
        g[1:-1].copy_(torch.from_numpy(x.astype(self.ndt)))
        return g

    def call(self, obs=None, obs_out=None, rew=None, rew_out=None, frozen=False, stream=None):
        p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None
        return self.L.sf_normalize(self.h, p(obs), p(obs_out), p(rew), p(rew_out), int(frozen), stream or self.stream())

    def state(self):
        st, ret = np.zeros(2 * self.dim + 4), np.zeros(self.n)
        self.lib.check(self.L.sf_normalizer_get_state(self.h, st.ctypes.data_as(C.c_void_p), ret.ctypes.data_as(C.c_void_p),
                                                      self.stream()))
        return st, ret

    def set_state(self, st, ret=None):
        st = np.ascontiguousarray(st, np.float64)
        ret = None if ret is None else np.ascontiguousarray(ret, np.float64)
        self.lib.check(self.L.sf_normalizer_set_state(self.h, st.ctypes.data_as(C.c_void_p),
                                                      ret.ctypes.data_as(C.c_void_p) if ret is not None else None, self.stream()))

    def guards_intact(self, *guarded):
        assert bool((self._obs_g[:GUARD] == PATTERN).all()) and bool((self._obs_g[-GUARD:] == PATTERN).all()), "guard rows overwritten"
        for g in guarded:
            assert bool((g[0] == PATTERN).all()) and bool((g[-1] == PATTERN).all()), "guard row overwritten"
        assert bool((self._rew_g[:64] == PATTERN).all()) and bool((self._rew_g[-64:] == PATTERN).all()), "reward guard overwritten"
