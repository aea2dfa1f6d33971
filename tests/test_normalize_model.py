"""The exact VecNormalize reference and its derived bounds (tests/normref.py), checked on the CPU so that the GPU
tests (test_gpu_normalize_kernels.py, test_gpu_vecnormalize.py) cannot fail because of the reference or the inputs.

 * the exact reference agrees with oracle/vecnorm_np.py (numpy, two-pass) within the two-pass bound;
 * the bound is sound: a float64 one-pass evaluation in numpy, in three summation orders, stays inside it (no margin);
 * the conditioning contract of sfmi.h: on well-conditioned inputs the bound on float32 outputs is below 1e-6 at every
   batch size the GPU tests use; on the ill-conditioned ones (mean 1000, deviation 1e-2 and 3e-4) it is not -- the
   one-pass batch variance loses mean(x^2) / var units of float64 precision.
"""
import numpy as np
import pytest

import normref as R
from oracle import vecnorm_np as V

DIM = 19
# every batch size of test_gpu_normalize_kernels.py and test_gpu_vecnormalize.py
GPU_SIZES = (1, 63, 64, 65, 333, 1000, 4096, 4100, 16384, 16448, 27648, 32768, 32832, 65536, 65537, 65600, 100000, 131072,
             262144, 262145)


@pytest.mark.parametrize("kind", R.OBS_KINDS)
@pytest.mark.parametrize("n,dtype", [(1, np.float32), (63, np.float64), (333, np.float32), (4096, np.float64)])
def test_exact_reference_agrees_with_numpy_model(kind, n, dtype):
    """oracle/vecnorm_np.py reduces along axis 0 of a C-ordered array, i.e. row after row: chains of n additions."""
    rk = R.REW_KINDS[R.OBS_KINDS.index(kind) % len(R.REW_KINDS)]
    ex = R.ExactVecNormalize(n, DIM, one_pass=False)
    mo = V.VecNormalize(n, (DIM,))
    o0 = R.gen_obs(kind, n, DIM, 99, dtype)
    ref, tol = ex.obfilt(o0, np.float64, n)
    R.check("model/" + kind, "reset", mo.reset(o0), ref, tol)
    for t in range(20):
        o, r = R.gen_obs(kind, n, DIM, t, dtype), R.gen_rew(rk, n, t)
        oref, otol, rref, rtol = ex.step(o, r, np.float64, n, n)
        mob, mrew = mo.step(o, r.astype(np.float64))
        R.check("model/" + kind, "obs", mob, oref, otol, where="step %d" % t)
        # (rewards: the reference rounds to float32 as the device does; the numpy model does not)
        R.check("model/" + kind, "rew", mrew.astype(np.float32), rref, rtol, where="step %d" % t)
        st = np.concatenate([mo.ob_rms.mean, mo.ob_rms.var, [mo.ret_rms.mean, mo.ret_rms.var, mo.ob_rms.count, mo.ret_rms.count]])
        R.check_stats("model/" + kind, ex, st, mo.ret, where="step %d" % t)


@pytest.mark.parametrize("order", ["pairwise", "forward", "backward"])
@pytest.mark.parametrize("kind", R.OBS_KINDS)
@pytest.mark.parametrize("n,dtype", [(1, np.float32), (65, np.float64), (4100, np.float32), (65537, np.float32)])
def test_bound_holds_for_one_pass_float64(kind, n, dtype, order):
    rk = R.REW_KINDS[(R.OBS_KINDS.index(kind) + 1) % len(R.REW_KINDS)]
    ex, k = R.ExactVecNormalize(n, DIM), R.OnePassF64(n, DIM, order)
    if kind.startswith("ill"):
        st0 = R.ill_start(kind, DIM)
        ex.load(st0)
        k.st = [st0[:DIM].copy(), st0[DIM:2 * DIM].copy(), st0[2 * DIM + 2]]
    d = k.depth(n)
    for t in range(6 if n > 10000 else 20):
        o, r = R.gen_obs(kind, n, DIM, t, dtype), R.gen_rew(rk, n, t)
        oref, otol, rref, rtol = ex.step(o, r, dtype, d, d)
        ko, kr = k.step(o, r.astype(np.float64), dtype)
        st = np.concatenate([k.st[0], k.st[1], k.rst[0], k.rst[1], [k.st[2], k.rst[2]]])
        w = [R.check("sound/" + kind, "obs", ko, oref, otol, where="step %d" % t),
             R.check("sound/" + kind, "rew", kr, rref, rtol, where="step %d" % t)]
        R.check_stats("sound/" + kind, ex, st, k.ret, where="step %d" % t)
        w += [R.RECORD[("sound/" + kind, q)][0] for q in ("ob_mean", "ob_var", "ret_mean", "ret_var")]
        assert max(w) <= 1.0, (kind, n, order, t, w)  # inside the bound itself, not only inside MARGIN times it


def _worst_f32_bound(kind, n, steps=3):
    ex = R.ExactVecNormalize(n, DIM)
    if kind.startswith("ill"):
        ex.load(R.ill_start(kind, DIM))
    d_ob = max(R.depth_standalone(n, DIM)[0], R.depth_fused(n, DIM)[0])
    d_ret = max(R.depth_standalone(n, DIM)[1], R.depth_fused(n, DIM)[1])
    worst = 0.0
    for t in range(steps):
        _, otol, _, rtol = ex.step(R.gen_obs(kind, n, DIM, t), R.gen_rew("game", n, t), np.float32, d_ob, d_ret)
        worst = max(worst, float(otol.max()), float(rtol.max()))
    return worst, float(ex.ob_rms.last_kappa.max())


@pytest.mark.parametrize("n", GPU_SIZES)
def test_well_conditioned_bounds_are_below_1e6(n):
    """The tolerance test_gpu_vecnormalize.py has always used (1e-6 on float32 outputs) is implied by the derived
    bound wherever mean(x^2) / var is moderate: half a float32 ulp at the clip value 10 is 2^-21 = 4.8e-7."""
    for kind in R.WELL_CONDITIONED:
        worst, _ = _worst_f32_bound(kind, n, 2 if n > 100000 else 3)
        assert worst < 1e-6, (kind, n, worst)


@pytest.mark.parametrize("kind,floor", [("ill-1e-2", 1e-6), ("ill-3e-4", 1e-3)])
def test_ill_conditioned_bounds_are_not(kind, floor):
    """mean 1000, deviation 1e-2: mean(x^2) / var = 1e10; deviation 3e-4: 1e13.  The one-pass variance leaves no useful
    bound on the output there (sfmi.h says so); a two-pass evaluation keeps it at rounding level."""
    n = 65537
    worst, kappa = _worst_f32_bound(kind, n)
    assert kappa > 1e9
    assert worst > floor, (kind, worst)
    ex2 = R.ExactVecNormalize(n, DIM, one_pass=False)
    ex2.load(R.ill_start(kind, DIM))
    d = R.depth_standalone(n, DIM)[0]
    _, otol, _, _ = ex2.step(R.gen_obs(kind, n, DIM, 0, np.float64), R.gen_rew("game", n, 0), np.float32, d, d)
    assert float(otol.max()) < 1e-6 if kind == "ill-1e-2" else float(otol.max()) < worst / 100
