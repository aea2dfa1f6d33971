"""SFVecNormalize (sf_normalize.hip) against the numpy restatement of gym_vecenv.VecNormalize
(oracle/vecnorm_np.py; the package itself is not in the reference tree: parity unpinned beyond that).
Tolerance: 1e-6 absolute on normalised float32 observations / rewards (float64 math inside, one-pass
batch variance vs numpy's two-pass), 1e-9 relative on the running statistics."""
import os

import numpy as np
import pytest

from lockstep import sfa

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.mark.parametrize("gametype,obs_type,f64,n", [("youturn", "features", False, 4096), ("autoturn", "features", True, 1000),
                                                    ("youturn", "monitors", False, 333)])
def test_vecnormalize_matches_numpy_model(sfa, gametype, obs_type, f64, n):
    from oracle import vecnorm_np as V
    rng = np.random.default_rng(4)
    mk = lambda: sfa.SFVecEnv(n, gametype=gametype, obs_type=obs_type, spawn_stride=1,
                              obs_dtype=torch.float64 if f64 else torch.float32)
    raw, env = mk(), sfa.SFVecNormalize(mk())
    model = V.VecNormalize(n, (raw.obs_dim,))
    o_raw = raw.reset().cpu().numpy().astype(np.float64)
    o = env.reset().cpu().numpy()
    assert np.abs(o - model.reset(o_raw)).max() < 1e-6
    for t in range(300):
        a = torch.from_numpy(rng.integers(0, raw.n_actions, n).astype(np.uint8)).to(raw.device)
        o_raw, r_raw, d_raw, i_raw = raw.step_tensors(a)
        o, r, d, i = env.step_tensors(a)
        mo, mr = model.step(o_raw.cpu().numpy().astype(np.float64), r_raw.cpu().numpy().astype(np.float64))
        assert torch.equal(d, d_raw) and torch.equal(i, i_raw)
        assert np.abs(o.cpu().numpy() - mo).max() < 1e-6, t
        assert np.abs(r.cpu().numpy() - mr).max() < 1e-6, t
    ob, rt = env.ob_rms, env.ret_rms
    assert np.allclose(ob.mean, model.ob_rms.mean, rtol=1e-9, atol=1e-12) and np.allclose(ob.var, model.ob_rms.var, rtol=1e-9, atol=1e-12)
    assert ob.count == model.ob_rms.count and rt.count == model.ret_rms.count
    assert np.isclose(rt.mean, model.ret_rms.mean, rtol=1e-9) and np.isclose(rt.var, model.ret_rms.var, rtol=1e-9)
    assert np.allclose(env.ret, model.ret, rtol=1e-12)
    # frozen statistics (evaluation) and a state round trip
    sd = env.state_dict()
    env.training = False
    a = torch.zeros(n, dtype=torch.uint8, device=raw.device)
    o_raw, r_raw, _, _ = raw.step_tensors(a)
    o, r, _, _ = env.step_tensors(a)
    want = np.clip((o_raw.cpu().numpy() - model.ob_rms.mean) / np.sqrt(model.ob_rms.var + 1e-8), -10, 10)
    assert np.abs(o.cpu().numpy() - want).max() < 1e-6
    assert np.array_equal(env.state_dict()["stats"], sd["stats"])
    env.load_state_dict(sd)
    assert np.array_equal(env.state_dict()["ret"], sd["ret"])
    # the numpy-in / numpy-out surface of the reference's wrapper
    env.training = True
    on, rn, dn, inn = env.step(np.zeros(n, np.int64))
    assert on.shape == (n, raw.obs_dim) and rn.dtype == np.float64 and dn.dtype == bool
    env.close()
    raw.close()


def test_vecnormalize_rejects_images(sfa):
    v = sfa.SFVecEnv(4, obs_type="image")
    with pytest.raises(ValueError):
        sfa.SFVecNormalize(v)
    v.close()


# ---------------------------------------------------------------------------------------------------------------------
# The fused path (sf_step_normalize: the batch sums ride on the step kernel) at every launch shape of sf_launch_step,
# through the C ABI with guarded outputs, against the exact reference and the derived bounds of tests/normref.py.
# A raw twin batch (same seed, spawn_stride=1) supplies the unnormalised observations and int rewards; the raw step
# itself is pinned by the parity suite.
#
#   size      lanes (padded to 256)   step launch for youturn `features` float32
#   4 096      4 096                  64 threads, split
#  16 384     16 384                  64 threads, split (the largest)
#   4 100      4 352                  64 threads, generic observation writer (n % 64 != 0), ragged last wave
#  16 448     16 640                  128 threads, split (the smallest)
#  32 768     32 768                  128 threads, split (the largest)
#  32 832     33 024                  256 threads, split, 516 rows of partial sums
#  65 536     65 536                  256 threads, split, 1 024 rows: the merge kernel's second pass begins beyond
#  65 600     65 792                  256 threads, fast writer, no split; 1 028 rows: the merge loops
# 131 072    131 072                  above 65 536: 2 048 rows
# 262 145    262 400                  every tail at once: generic writer, ragged wave, three padded waves, 4 100 rows
# float64 `features`, `normalized-features` and `monitors` always take the generic writer, never the split launch.
import ctypes as C

import normref as R

FUSED_SIZES = (4096, 16384, 4100, 16448, 32768, 32832, 65536, 65600, 131072, 262145)
OTHER_SIZES = (4100, 32832, 65536, 262145)
LATE = (4100, 65536)          # `time` set late in the episode: auto-reset rows flow through the sums
WITH_STANDALONE = (4100, 65536, 131072)


def _steps(n):
    """40 steps; fewer at the two largest sizes, where the longdouble reference on the host is what takes the time"""
    return 40 if n <= 65600 else (12 if n <= 131072 else 8)


class _Fused:
    """An SFVecEnv and an sf_normalizer driven through sf_step_normalize / sf_step + sf_normalize, outputs guarded."""

    def __init__(self, sfa, n, gametype, obs_type, f64, ob=True, ret=True):
        from spacefortress_amd import _lib
        self.v = sfa.SFVecEnv(n, gametype=gametype, obs_type=obs_type, spawn_stride=1, obs_dtype=torch.float64 if f64 else torch.float32)
        self.z = R.Norm(_lib, n, self.v.obs_dim, f64, ob, ret)
        self.lib, self.L, self.n = _lib, _lib.lib(), n
        dev = self.v.device
        self.rdi = torch.full((6 * n + 128,), 0x5A, dtype=torch.uint8, device=dev)
        self.rew, self.done, self.info = self.rdi[64:64 + 4 * n].view(torch.int32), self.rdi[64 + 4 * n:64 + 5 * n], self.rdi[64 + 5 * n:64 + 6 * n]

    def reset(self):
        o = self.v.reset()
        assert self.z.call(o, self.z.obs_out) == 0
        return o, self.z.obs_out

    def step(self, a, frozen=False, fused=True):
        """-> normalised obs (in place, guarded), raw int32 rewards, done, info, normalised rewards"""
        z, p = self.z, lambda t: C.c_void_p(t.data_ptr())
        z.rew_out.fill_(R.PATTERN)
        if fused:
            self.lib.check(self.L.sf_step_normalize(self.v._h, z.h, p(a), 1, p(z.obs_out), p(self.rew), p(self.done), p(self.info),
                                                    p(z.rew_out), int(frozen), z.stream()))
        else:
            self.lib.check(self.L.sf_step(self.v._h, p(a), 1, p(z.obs_out), p(self.rew), p(self.done), p(self.info), z.stream()))
            assert z.call(z.obs_out, z.obs_out, self.rew, z.rew_out, frozen) == 0
        self.v._stepped(a, self.rew, self.done, self.info)
        return z.obs_out, self.rew, self.done, self.info, z.rew_out

    def guards_intact(self):
        self.z.guards_intact()
        assert bool((self.rdi[:64] == 0x5A).all()) and bool((self.rdi[-64:] == 0x5A).all()), "reward / done / info guard overwritten"

    def close(self):
        self.z.close()
        self.v.close()


def _late(*envs):
    for e in envs:
        e.set_field("time", np.full(e.num_envs, 34 * 5288, np.int32))


def _fused_case(sfa, fam, gametype, obs_type, f64, n, with_standalone=False, late=False):
    rng = np.random.default_rng(n)
    ndt = np.float64 if f64 else np.float32
    raw = sfa.SFVecEnv(n, gametype=gametype, obs_type=obs_type, spawn_stride=1, obs_dtype=torch.float64 if f64 else torch.float32)
    fu = _Fused(sfa, n, gametype, obs_type, f64)
    sa = _Fused(sfa, n, gametype, obs_type, f64) if with_standalone else None
    dim = raw.obs_dim
    ex = R.ExactVecNormalize(n, dim)
    exs = R.ExactVecNormalize(n, dim) if sa else None  # (the stand-alone kernels have their own summation depth)
    d_f, d_s = R.depth_fused(n, dim), R.depth_standalone(n, dim)
    o_raw = raw.reset().cpu().numpy().astype(np.float64)
    for e, m in ((fu, ex), (sa, exs)):
        if e is not None:
            _, o = e.reset()
            want, tol = m.obfilt(o_raw, ndt, d_s[0])
            R.check(fam, "obs", o.cpu().numpy(), want, tol, where="reset")
    if late:
        _late(raw, fu.v, *([sa.v] if sa else []))
    any_done = False
    for t in range(_steps(n)):
        a = torch.from_numpy(rng.integers(0, raw.n_actions, n).astype(np.uint8)).to(raw.device)
        o_raw, r_raw, d_raw, i_raw = raw.step_tensors(a)
        x, r = o_raw.cpu().numpy().astype(np.float64), r_raw.cpu().numpy()
        o, rr, d, i, rn = fu.step(a)
        assert torch.equal(d, d_raw) and torch.equal(i, i_raw) and torch.equal(rr, r_raw), t
        any_done |= bool(d_raw.any())
        want, tol, wr, tr = ex.step(x, r, ndt, *d_f)
        og, rg = o.cpu().numpy(), rn.cpu().numpy()
        R.check(fam, "obs", og, want, tol, where="step %d" % t)
        R.check(fam, "rew", rg, wr, tr, where="step %d" % t)
        R.check_stats(fam, ex, *fu.z.state(), where="step %d" % t)
        fu.guards_intact()
        if sa:  # sf_step + sf_normalize on a third copy: a cross-check of the two paths, both held to the reference too
            o2, rr2, d2, i2, rn2 = sa.step(a, fused=False)
            assert torch.equal(d2, d_raw) and torch.equal(i2, i_raw) and torch.equal(rr2, r_raw), t
            want2, tol2, wr2, tr2 = exs.step(x, r, ndt, *d_s)
            R.check(fam + "/standalone", "obs", o2.cpu().numpy(), want2, tol2, where="step %d" % t)
            R.check(fam + "/standalone", "rew", rn2.cpu().numpy(), wr2, tr2, where="step %d" % t)
            R.check_stats(fam + "/standalone", exs, *sa.z.state(), where="step %d" % t)
            # (each path within its bound of the same exact value: within the sum of the two of each other)
            R.check(fam + "/fused-vs-standalone", "obs", og, o2.cpu().numpy().astype(np.float64), tol + tol2, where="step %d" % t)
            R.check(fam + "/fused-vs-standalone", "rew", rg, rn2.cpu().numpy().astype(np.float64), tr + tr2, where="step %d" % t)
            s1, s2 = fu.z.state()[0], sa.z.state()[0]
            R.check(fam + "/fused-vs-standalone", "ob_mean", s1[:dim], s2[:dim], ex.ob_rms.em + exs.ob_rms.em)
            R.check(fam + "/fused-vs-standalone", "ob_var", s1[dim:2 * dim], s2[dim:2 * dim], ex.ob_rms.ev_hi + exs.ob_rms.ev_hi)
            sa.guards_intact()
    if late:
        assert any_done, "no episode ended: the auto-reset rows were not exercised"
    for e in (fu, sa):
        if e is not None:
            e.close()
    raw.close()


@pytest.fixture(scope="module")
def norm_record():
    yield
    print()
    for line in R.record_lines():
        print(line)


@pytest.mark.parametrize("n", FUSED_SIZES)
def test_fused_step_youturn_features_f32(sfa, norm_record, n):
    _fused_case(sfa, "fused/youturn-f32", "youturn", "features", False, n, with_standalone=n in WITH_STANDALONE, late=n in LATE)


@pytest.mark.parametrize("gametype,obs_type,f64", [("autoturn", "features", True), ("youturn", "normalized-features", False),
                                                   ("autoturn", "monitors", False)])
@pytest.mark.parametrize("n", OTHER_SIZES)
def test_fused_step_other_observations(sfa, norm_record, gametype, obs_type, f64, n):
    _fused_case(sfa, "fused/%s-%s" % (obs_type, "f64" if f64 else "f32"), gametype, obs_type, f64, n, late=n in LATE)


@pytest.mark.parametrize("n", [4100, 65536])
def test_fused_step_with_ob_off_and_with_ret_off(sfa, norm_record, n):
    """sf_step_normalize with VecNormalize(ob=False) and with VecNormalize(ret=False): Python never takes the fused path
    for these, the C ABI does."""
    rng = np.random.default_rng(n + 1)
    raw = sfa.SFVecEnv(n, gametype="youturn", spawn_stride=1)
    no_ob, no_ret = _Fused(sfa, n, "youturn", "features", False, ob=False), _Fused(sfa, n, "youturn", "features", False, ret=False)
    dim = raw.obs_dim
    ex_ob, ex_ret = R.ExactVecNormalize(n, dim, ob=False), R.ExactVecNormalize(n, dim, ret=False)
    d_f = R.depth_fused(n, dim)
    o_raw = raw.reset()
    for e in (no_ob, no_ret):
        e.v.reset()
    init = no_ob.z.state()[0]
    for t in range(20):
        a = torch.from_numpy(rng.integers(0, raw.n_actions, n).astype(np.uint8)).to(raw.device)
        o_raw, r_raw, d_raw, i_raw = raw.step_tensors(a)
        x, r = o_raw.cpu().numpy().astype(np.float64), r_raw.cpu().numpy()
        # ob = 0: observations come back as the step wrote them, rewards are normalised
        o, rr, d, i, rn = no_ob.step(a)
        assert torch.equal(o, o_raw) and torch.equal(rr, r_raw) and torch.equal(d, d_raw) and torch.equal(i, i_raw), t
        _, _, wr, tr = ex_ob.step(x, r, np.float32, *d_f)
        R.check("fused/ob-off", "rew", rn.cpu().numpy(), wr, tr, where="step %d" % t)
        st, rt = no_ob.z.state()
        R.check_stats("fused/ob-off", ex_ob, st, rt, where="step %d" % t)
        assert np.array_equal(st[:2 * dim], init[:2 * dim]) and st[2 * dim + 2] == init[2 * dim + 2]
        no_ob.guards_intact()
        # ret = 0: reward_out is not touched, the returns stay zero
        o, rr, d, i, rn = no_ret.step(a)
        assert torch.equal(rr, r_raw) and torch.equal(d, d_raw) and torch.equal(i, i_raw), t
        assert bool((rn == R.PATTERN).all()), "reward_out written with ret = 0"
        want, tol, _, _ = ex_ret.step(x, r, np.float32, *d_f)
        R.check("fused/ret-off", "obs", o.cpu().numpy(), want, tol, where="step %d" % t)
        st, rt = no_ret.z.state()
        R.check_stats("fused/ret-off", ex_ret, st, where="step %d" % t)
        assert not rt.any() and np.array_equal(st[2 * dim:2 * dim + 2], init[2 * dim:2 * dim + 2]) and st[2 * dim + 3] == init[2 * dim + 3]
        no_ret.guards_intact()
    for e in (no_ob, no_ret):
        e.close()
    raw.close()


def test_frozen_fused_step_at_65536(sfa, norm_record):
    n = 65536
    rng = np.random.default_rng(7)
    raw, fu = sfa.SFVecEnv(n, gametype="youturn", spawn_stride=1), _Fused(sfa, n, "youturn", "features", False)
    dim = raw.obs_dim
    ex = R.ExactVecNormalize(n, dim)
    d_f = R.depth_fused(n, dim)
    ex.obfilt(raw.reset().cpu().numpy().astype(np.float64), np.float32, R.depth_standalone(n, dim)[0])
    fu.reset()
    for t in range(6):
        frozen = t >= 3
        a = torch.from_numpy(rng.integers(0, raw.n_actions, n).astype(np.uint8)).to(raw.device)
        o_raw, r_raw, d_raw, i_raw = raw.step_tensors(a)
        before = fu.z.state()
        o, rr, d, i, rn = fu.step(a, frozen=frozen)
        want, tol, wr, tr = ex.step(o_raw.cpu().numpy().astype(np.float64), r_raw.cpu().numpy(), np.float32, *d_f, update=not frozen)
        assert torch.equal(rr, r_raw) and torch.equal(d, d_raw) and torch.equal(i, i_raw), t
        R.check("fused/frozen", "obs", o.cpu().numpy(), want, tol, where="step %d" % t)
        R.check("fused/frozen", "rew", rn.cpu().numpy(), wr, tr, where="step %d" % t)
        after = fu.z.state()
        if frozen:
            assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes(), "a frozen step changed the state"
        R.check_stats("fused/frozen", ex, *after, where="step %d" % t)
        fu.guards_intact()
    fu.close()
    raw.close()


def test_fused_training_step_is_refused_inside_a_capture(sfa, norm_record):
    """sfmi.h: sf_step_normalize updates the statistics unless frozen, and such a call flips their double buffer on the
    host: refused with SF_ERR_ARG before the step is launched.  A frozen fused step is captured and replays."""
    from spacefortress_amd import _lib
    n = 4096
    fu, tw = _Fused(sfa, n, "youturn", "features", False), _Fused(sfa, n, "youturn", "features", False)
    a = torch.ones(n, dtype=torch.uint8, device=fu.v.device)
    for e in (fu, tw):
        e.reset()
        e.step(a)
        e.step(a, frozen=True)  # (everything a step allocates exists before the capture)
    p = lambda t: C.c_void_p(t.data_ptr())
    z = fu.z
    before = z.state()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = fu.L.sf_step_normalize(fu.v._h, z.h, p(a), 1, p(z.obs_out), p(fu.rew), p(fu.done), p(fu.info), p(z.rew_out), 0, z.stream())
        rc_frozen = fu.L.sf_step_normalize(fu.v._h, z.h, p(a), 1, p(z.obs_out), p(fu.rew), p(fu.done), p(fu.info), p(z.rew_out), 1, z.stream())
    assert rc == _lib.SF_ERR_ARG and rc_frozen == 0, (rc, rc_frozen)
    for it in range(3):  # the graph holds one frozen step: each replay is one eager frozen step of the twin
        g.replay()
        o2, r2, d2, i2, rn2 = tw.step(a, frozen=True)
        torch.cuda.synchronize()
        assert torch.equal(z.obs_out, o2) and torch.equal(z.rew_out, rn2) and torch.equal(fu.rew, r2) and torch.equal(fu.done, d2), it
    after = z.state()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    fu.close()
    tw.close()
