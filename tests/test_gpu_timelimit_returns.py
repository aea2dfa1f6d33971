"""sf_compute_returns_tl (the returns recursion with the time limit's bootstrap) and DeviceRollout(time_limit_bootstrap=True).

The kernel against three evaluations, bit for bit (trainerref.assert_bits_equal): the numpy model (tests/timelimit_np.py), the
library's own sf_compute_returns on torch.where(masks[1:] == 0, rewards + gamma32 * fv, rewards), and the reference's
expressions on torch CPU tensors.  Then the rollout end to end on the constructed batch of tests/finalobsref.py."""
import ctypes as C

import numpy as np
import pytest

import finalobsref as F
import normref as NR
import timelimit_np as TL
import trainerref as TR
from sfcompare import obs_close

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda"
TS, NS = (1, 2, 7), (1, 63, 64, 65, 257, 4097)


@pytest.fixture(scope="module")
def L():
    import spacefortress_amd  # noqa: F401
    from spacefortress_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _lib.lib()


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _dev(x):
    x = np.ascontiguousarray(x)
    return TR.guarded(x.shape, torch.float32, DEV, x)


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _run_tl(L, kind, n, T, gae, gamma, tau):
    rewards, vp, masks, nv = TR.gen_returns_case(kind, T, n)
    fv = TL.gen_final_value(kind, n)
    tag = "%s n=%d T=%d %s (%r, %r)" % (kind, n, T, "gae" if gae else "plain", gamma, tau)
    want, want_vp = TL.compute_returns_tl(rewards, vp.copy(), masks, nv, fv, gae, gamma, tau)
    want_t, _ = TL.torch_compute_returns_tl(rewards, vp.copy(), masks, nv, fv, gae, gamma, tau)
    d_rew, d_vp, d_masks, d_nv, d_fv, d_ret = _dev(rewards), _dev(vp), _dev(masks), _dev(nv), _dev(fv), TR.guarded((T + 1, n), torch.float32, DEV)
    assert L.sf_compute_returns_tl(T, n, _p(d_rew), _p(d_vp), _p(d_masks), _p(d_nv), _p(d_fv), _p(d_ret), int(gae), gamma, tau, None) == 0, tag
    # the library's plain recursion on the rewards a trainer would patch by hand
    g32 = torch.tensor(gamma, dtype=torch.float32, device=DEV)
    d_rew2 = torch.where(d_masks[1:] == 0, d_rew + g32 * d_fv, d_rew).contiguous()
    d_vp2, d_ret2 = _dev(vp), TR.guarded((T + 1, n), torch.float32, DEV)
    assert L.sf_compute_returns(T, n, _p(d_rew2), _p(d_vp2), _p(d_masks), _p(d_nv), _p(d_ret2), int(gae), gamma, tau, None) == 0, tag
    torch.cuda.synchronize()
    rows = slice(0, T) if gae else slice(0, T + 1)
    TR.assert_bits_equal(d_ret[rows], want[rows], tag + " vs the numpy model")
    TR.assert_bits_equal(d_ret[rows], want_t[rows], tag + " vs torch")
    TR.assert_bits_equal(d_ret[rows], d_ret2[rows], tag + " vs sf_compute_returns on patched rewards")
    if gae:
        assert TR.untouched(d_ret[T]), tag
        TR.assert_bits_equal(d_vp, want_vp, tag + " value_preds")
    else:
        assert _bytes(d_vp) == vp.tobytes(), tag
    assert _bytes(d_rew) == rewards.tobytes() and _bytes(d_masks) == masks.tobytes() and _bytes(d_nv) == nv.tobytes() \
        and _bytes(d_fv) == fv.tobytes(), tag + ": an input changed"
    TR.margins_intact(d_rew, d_vp, d_masks, d_nv, d_fv, d_ret)
    # NaN in the final_value of the envs that never finish leaves no trace
    never = ~TL.finished(masks)
    if never.any():
        fv2 = fv.copy()
        fv2[never] = np.nan
        d_fv2, d_vp3, d_ret3 = _dev(fv2), _dev(vp), TR.guarded((T + 1, n), torch.float32, DEV)
        assert L.sf_compute_returns_tl(T, n, _p(d_rew), _p(d_vp3), _p(d_masks), _p(d_nv), _p(d_fv2), _p(d_ret3), int(gae), gamma, tau, None) == 0
        torch.cuda.synchronize()
        assert _bytes(d_ret3) == _bytes(d_ret), tag + ": a never-finished env's final_value shows"
    return never


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("n", NS)
def test_returns_tl_at_every_shape(L, n, T):
    kind, (gamma, tau) = TR.RETURNS_FULL
    for gae in (True, False):
        _run_tl(L, kind, n, T, gae, gamma, tau)


@pytest.mark.parametrize("kind", TR.KINDS)
def test_returns_tl_of_every_kind_and_pair(L, kind):
    """every value kind (subnormals, +-0, inf, NaN among them) with every (gamma, tau) pair of the table, at a partial last
    block (257 x 7) and at more than one block with the shortest scan (4097 x 1)"""
    seen_never = False
    for gamma, tau in TR.GAMMA_TAU:
        for n, T in ((257, 7), (4097, 1)):
            for gae in (True, False):
                seen_never |= bool(_run_tl(L, kind, n, T, gae, gamma, tau).any())
    assert seen_never


def test_returns_tl_refusals(L):
    n, T = 257, 3
    rewards, vp, masks, nv = TR.gen_returns_case("normal", T, n)
    fv = TL.gen_final_value("normal", n)
    d_rew, d_vp, d_masks, d_nv, d_fv, d_ret = _dev(rewards), _dev(vp), _dev(masks), _dev(nv), _dev(fv), TR.guarded((T + 1, n), torch.float32, DEV)
    a = [T, n, _p(d_rew), _p(d_vp), _p(d_masks), _p(d_nv), _p(d_fv), _p(d_ret), 1, 0.99, 0.95, None]
    for i, v in ((6, None), (0, 0), (0, -1), (1, 0), (1, -5), (2, None), (3, None), (4, None), (5, None), (7, None)):
        b = list(a)
        b[i] = v
        assert L.sf_compute_returns_tl(*b) == -2, (i, v)  # SF_ERR_ARG
    torch.cuda.synchronize()
    assert TR.untouched(d_ret) and _bytes(d_vp) == vp.tobytes()
    TR.margins_intact(d_rew, d_vp, d_masks, d_nv, d_fv, d_ret)


# ---------------------------------------------------------------------------------------------------------------
# DeviceRollout(time_limit_bootstrap=True), end to end
@pytest.mark.parametrize("normalised", [False, True], ids=["raw", "vecnormalize"])
def test_rollout_with_time_limit_bootstrap(normalised):
    import spacefortress_amd as sfa

    n, T = 130, F.T_RUN
    run = F.oracle_run("youturn", n)
    env = sfa.SFVecEnv(n, gametype="youturn")
    dev = env.device
    raw = torch.full((n, env.obs_dim), float("nan"), dtype=torch.float32, device=dev)  # never-written rows: NaN for the critic
    env.enable_final_obs(out=raw)
    z = sfa.SFVecNormalize(env) if normalised else None
    ro = sfa.DeviceRollout(z if normalised else env, T, time_limit_bootstrap=True)
    assert env.final_obs is raw  # (adopted, not replaced)
    # (no ro.reset(): new games would move the lanes' spawn cursors off the oracle's; observations[0] is not looked at)
    F.load_env(env, run["base"], run["pv"])
    g = torch.Generator().manual_seed(3)
    values = torch.randn(T, n, 1, generator=g).to(dev)
    a = torch.from_numpy(run["acts"].copy()).to(dev)
    for t in range(T):
        ro.step(t, a[t], value_pred=values[t])
    w = torch.randn(env.obs_dim, generator=g).to(dev) * 0.1
    critic = lambda x: x @ w  # a fixed critic: NaN for a row that was never written
    with pytest.raises(ValueError):
        ro.compute_returns(values[0], True, 0.99, 0.95)  # no silent fall-back
    stats0 = z.state_dict()["stats"] if normalised else None
    seen = ro.final_obs()
    torch.cuda.synchronize()
    want, finished = F.final_rows(run)
    assert finished.sum() == n - -(-n // 7)
    rawn = raw.cpu().numpy()
    assert np.isnan(rawn[~finished]).all()
    ok = obs_close(rawn[finished], want[finished], False)
    assert ok.all(), np.argwhere(~ok)[:5]
    if normalised:
        # the frozen normalisation of the rows the env holds (shown above to be the oracle's, to float32), with the statistics
        # as they stand at the call: normref's exact evaluation and its derived bound for a float32 result
        assert seen.data_ptr() != raw.data_ptr()
        model = NR.ExactVecNormalize(n, env.obs_dim)
        model.load(stats0)
        ref, tol = model.obfilt(rawn[finished].astype(np.float64), np.float32, update=False)
        NR.check("final_obs", "normalised rows", seen.cpu().numpy()[finished], ref, tol)
        again = ro.final_obs()
        assert _bytes(again) == _bytes(seen) and np.array_equal(z.state_dict()["stats"], stats0)  # nothing was updated
    else:
        assert seen is raw
    fv, nv = critic(seen), torch.randn(n, generator=g).to(dev)
    assert bool(torch.isnan(fv[torch.from_numpy(~finished).to(dev)]).all())
    for gae in (True, False):
        ro.compute_returns(nv, gae, 0.99, 0.95, final_value=fv)
        torch.cuda.synchronize()
        rew, vp, masks = (x[:, :, 0].cpu().numpy() for x in (ro.rewards, ro.value_preds, ro.masks))
        assert np.array_equal(masks[1:] == 0, run["done"])
        model_ret, _ = TL.compute_returns_tl(rew, vp.copy(), masks, nv.cpu().numpy(), fv.cpu().numpy(), gae, 0.99, 0.95)
        rows = slice(0, T) if gae else slice(0, T + 1)
        got = ro.returns[:, :, 0].cpu().numpy()
        TR.assert_bits_equal(got[rows], model_ret[rows], "returns, gae=%s" % gae)
        assert np.isfinite(got[rows]).all()
        plain, _ = TR.compute_returns(rew, vp.copy(), masks, nv.cpu().numpy(), gae, 0.99, 0.95)
        assert (got[:T][run["done"]] != plain[:T][run["done"]]).any()  # the bootstrap is there
    (z or env).close()


def test_rollout_refusals():
    import spacefortress_amd as sfa

    env = sfa.SFVecEnv(65)
    with pytest.raises(ValueError):
        sfa.DeviceRollout(env, env.max_ticks + 2, time_limit_bootstrap=True)
    with pytest.raises(ValueError):
        sfa.DeviceRollout(env, 4, num_stack=4, time_limit_bootstrap=True)
    with pytest.raises(ValueError):
        sfa.FrameRollout(env, 4, time_limit_bootstrap=True)
    assert env.final_obs is None
    ro = sfa.DeviceRollout(env, 4)  # without the flag: no final rows, the reference's recursion
    with pytest.raises(ValueError):
        ro.final_obs()
    assert env.final_obs is None
    env.close()
    env = sfa.SFVecEnv(65, auto_reset=False)
    with pytest.raises(ValueError):
        sfa.DeviceRollout(env, 4, time_limit_bootstrap=True)
    env.close()
