"""The finished game's last observation (sfmi.h: sf_set_final_obs_output; SFVecEnv.enable_final_obs).

1. parity with the oracle driven one env at a time (tests/finalobsref.py), every step: finished lanes' rows, untouched rows,
   guard margins, and the step's own outputs and final state;
2. every stepping entry point against plain sf_step on the recorded actions: bit-identical rows;
3. an independent device path at the three workgroup sizes: a twin batch WITHOUT auto-reset holds a finished lane's last
   observation in its ordinary observation row;
4. off means off; 5. refusals; 6. a captured graph.

Tolerance of 1: sfcompare.obs_close, the existing parity tests' rule for the dtype.  Everything else is compared bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import finalobsref as F
import trainerref as TR
from sfcompare import compare_state, obs_close
from lockstep import sfa

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _guarded_rows(env):
    return TR.guarded((env.num_envs, env.obs_dim), env.obs_dtype, env.device)


def _outs(env, T):
    n, dev = env.num_envs, env.device
    return (torch.empty((T, n, env.obs_dim), dtype=env.obs_dtype, device=dev), torch.empty((T, n), dtype=torch.int32, device=dev),
            torch.empty((T, n), dtype=torch.uint8, device=dev), torch.empty((T, n), dtype=torch.uint8, device=dev))


def _bytes(t):
    return t.cpu().numpy().tobytes()


# ---------------------------------------------------------------------------------------------------------------
# 1. oracle parity
@pytest.mark.parametrize("faithful", [True, False], ids=["faithful", "realshells"])
@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("obs_type", ["features", "normalized-features", "monitors"])
@pytest.mark.parametrize("gametype", ["youturn", "autoturn", "test-youturn"])
@pytest.mark.parametrize("n", [1, 63, 65, 130])
def test_final_rows_equal_the_oracles(sfa, n, gametype, obs_type, f64, faithful):
    T = F.T_RUN
    run = F.oracle_run(gametype, n, obs_type, faithful)
    env = F.make_env(sfa, run, gametype, n, obs_type, f64, faithful)
    fin = _guarded_rows(env)
    assert env.enable_final_obs(out=fin) is fin and env.final_obs is fin
    a = torch.from_numpy(run["acts"].copy()).to(env.device)
    obs, rew, done, info = _outs(env, T)
    hist = torch.empty((T,) + tuple(fin.shape), dtype=fin.dtype, device=env.device)
    for t in range(T):
        env.step_tensors(a[t], out=(obs[t], rew[t], done[t], info[t]))
        hist[t].copy_(fin)
    torch.cuda.synchronize()
    TR.margins_intact(fin)
    obs, rew, done, info, hist = obs.cpu().numpy(), rew.cpu().numpy(), done.cpu().numpy().astype(bool), info.cpu().numpy().astype(bool), hist.cpu().numpy()
    # the step itself
    assert np.array_equal(rew, run["rew"]) and np.array_equal(done, run["done"]) and np.array_equal(info, run["info"])
    ok = obs_close(obs, run["obs"], f64)
    assert ok.all(), np.argwhere(~ok)[:5]
    assert not compare_state(env.state_dict(), run["snaps"])
    # the rows, after every step
    assert int(done.sum()) == int(run["done"].sum()) >= n - -(-n // 7)
    for t in range(T):
        want, finished = F.final_rows(run, t)
        assert F.is_sentinel(hist[t][~finished]).all(), (t, "a row of a lane that has not finished was written")
        if finished.any():
            ok = obs_close(hist[t][finished], want[finished], f64)
            assert ok.all(), (t, np.flatnonzero(finished)[np.argwhere(~ok)[:5, 0]], np.argwhere(~ok)[:5])
    env.close()
    assert env.final_obs is None


# ---------------------------------------------------------------------------------------------------------------
# 2. every entry point
def _plain_rows(sfa, run, n, acts_u8):
    """the reference of this section: the same batch driven by plain sf_step on `acts_u8` [T, n] -> (rows, state)"""
    env = F.make_env(sfa, run, "youturn", n)
    fin = _guarded_rows(env)
    env.enable_final_obs(out=fin)
    a = torch.from_numpy(np.ascontiguousarray(acts_u8)).to(env.device)
    for t in range(a.shape[0]):
        env.step_tensors(a[t])
    torch.cuda.synchronize()
    TR.margins_intact(fin)
    out = _bytes(fin), env.state_dict()
    env.close()
    return out


ENTRY_POINTS = ("sf_step", "sf_step_record", "sf_step_normalize", "sf_step_sampled", "sf_rollout", "sf_rollout_sampled")


@pytest.mark.parametrize("entry", ENTRY_POINTS)
@pytest.mark.parametrize("n", [130, 128])  # (128: full waves, the default observation's own instantiations)
def test_every_entry_point_writes_the_same_rows(sfa, n, entry):
    from spacefortress_amd import _lib

    T = F.T_RUN
    run = F.oracle_run("youturn", n)
    env = F.make_env(sfa, run, "youturn", n)
    L, dev = _lib.lib(), env.device
    fin = _guarded_rows(env)
    env.enable_final_obs(out=fin)
    given = torch.from_numpy(run["acts"].copy()).to(dev)
    played = given
    if entry == "sf_step":
        wide = given.to(torch.int32)
        for t in range(T):
            env.step_tensors(wide[t])
    elif entry == "sf_step_record":
        obs, rew, done, info = _outs(env, 1)
        rf = torch.empty(n, dtype=torch.float32, device=dev)
        p = lambda x: C.c_void_p(x.data_ptr())
        for t in range(T):
            assert L.sf_step_record(env._h, p(given[t]), 1, p(obs), p(rew), p(done), p(info), p(rf), None, None, None, None,
                                    env._stream()) == 0
    elif entry == "sf_step_normalize":
        z = sfa.SFVecNormalize(env)
        for t in range(T):
            z.step_tensors(given[t])
    elif entry == "sf_step_sampled":
        env.seed_actions(99)
        played = torch.empty((T, n), dtype=torch.uint8, device=dev)
        for t in range(T):
            env.step_sampled(actions_out=played[t])
    elif entry == "sf_rollout":
        env.rollout(given)
    else:
        env.seed_actions(99)
        played = env.rollout_sampled(T)[4]
    torch.cuda.synchronize()
    TR.margins_intact(fin)
    got, sd = _bytes(fin), env.state_dict()
    if entry == "sf_step_normalize":
        z.close()  # (closes the env too)
    else:
        env.close()
    want, want_sd = _plain_rows(sfa, run, n, played.cpu().numpy())
    assert got == want, entry
    assert all(np.array_equal(sd[k], want_sd[k]) for k in sd), entry
    rows = np.frombuffer(got, np.float32).reshape(n, -1)
    assert (~F.is_sentinel(rows)).sum() >= n - -(-n // 7)


# ---------------------------------------------------------------------------------------------------------------
# 3. the twin without auto-reset, at the three workgroup sizes
@pytest.mark.parametrize("n", [257, 16384 + 64, 32768 + 64])
def test_rows_equal_a_no_auto_reset_twins_observation(sfa, n):
    T = 8
    rng = np.random.default_rng(n)
    env = sfa.SFVecEnv(n, gametype="youturn", spawn_stride=1)
    env.reset()
    warm = torch.from_numpy(rng.integers(0, 5, (40, n)).astype(np.uint8)).to(env.device)
    env.rollout(warm, want_obs=False)  # ships under way, missiles and shells in the air
    clock = (180000 - 34 * rng.integers(1, T + 1, n)).astype(np.int32)  # game over after 1 .. T more ticks
    clock[::7] = 34 * 100
    env.set_field("time", clock)
    sd = env.state_dict()
    twin = sfa.SFVecEnv(n, gametype="youturn", spawn_stride=1, auto_reset=False)
    twin.load_state_dict(sd)
    fin = _guarded_rows(env)
    env.enable_final_obs(out=fin)
    a = torch.from_numpy(rng.integers(0, 5, (T, n)).astype(np.uint8)).to(env.device)
    eo, tw = _outs(env, T), _outs(twin, T)
    for t in range(T):
        env.step_tensors(a[t], out=tuple(x[t] for x in eo))
        twin.step_tensors(a[t], out=tuple(x[t] for x in tw))
    torch.cuda.synchronize()
    TR.margins_intact(fin)
    done, tdone = eo[2].cpu().numpy().astype(bool), tw[2].cpu().numpy().astype(bool)
    assert done.sum(0).max() == 1 and done.sum() == n - -(-n // 7)
    first = np.where(tdone.any(0), tdone.argmax(0), -1)  # the twin stays done once it is
    assert np.array_equal(first, np.where(done.any(0), done.argmax(0), -1))
    rows, tobs = fin.cpu().numpy(), tw[0].cpu().numpy()
    lanes = np.flatnonzero(first >= 0)
    assert rows[lanes].tobytes() == tobs[first[lanes], lanes].tobytes()
    assert F.is_sentinel(rows[first < 0]).all()
    env.close()
    twin.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. off means off
@pytest.mark.parametrize("n", [130, 128])
def test_off_means_off(sfa, n):
    T = F.T_RUN
    run = F.oracle_run("youturn", n)
    res = {}
    for mode in ("on", "never", "withdrawn"):
        env = F.make_env(sfa, run, "youturn", n)
        fin = _guarded_rows(env)
        if mode != "never":
            env.enable_final_obs(out=fin)
        if mode == "withdrawn":
            assert env.enable_final_obs(False) is None and env.final_obs is None
        a = torch.from_numpy(run["acts"].copy()).to(env.device)
        outs = _outs(env, T)
        for t in range(T):
            env.step_tensors(a[t], out=tuple(x[t] for x in outs))
        torch.cuda.synchronize()
        TR.margins_intact(fin)
        assert TR.untouched(fin) == (mode != "on"), mode
        res[mode] = ([_bytes(x) for x in outs], env.state_dict())
        env.close()
    for mode in ("never", "withdrawn"):
        assert res[mode][0] == res["on"][0], mode
        assert all(np.array_equal(res[mode][1][k], res["on"][1][k]) for k in res["on"][1]), mode


# ---------------------------------------------------------------------------------------------------------------
# 5. refusals
def test_refusals_leave_the_batch_stepping(sfa):
    from spacefortress_amd import _lib

    L = _lib.lib()
    n = 65
    for kw in (dict(obs_type="image"), dict(auto_reset=False)):
        env = sfa.SFVecEnv(n, **kw)
        buf = torch.zeros(n * 32, dtype=torch.float32, device=env.device)
        with pytest.raises(ValueError):
            env.enable_final_obs()
        assert env.final_obs is None
        assert L.sf_set_final_obs_output(env._h, C.c_void_p(buf.data_ptr())) == _lib.SF_ERR_ARG
        text = _lib.last_error()
        assert ("sf_reset_lanes" in text and "SF_FLAG_NO_AUTO_RESET" in text) if "obs_type" in kw else "SF_FLAG_NO_AUTO_RESET" in text
        assert L.sf_set_final_obs_output(env._h, None) == 0  # (off is always possible)
        env.reset()
        env.step_tensors(torch.zeros(n, dtype=torch.uint8, device=env.device))
        torch.cuda.synchronize()
        env.close()
    env = sfa.SFVecEnv(n)
    big = TR.guarded((n * env.obs_dim + 4,), torch.float32, env.device)
    for off in (1, 2, 3):
        assert L.sf_set_final_obs_output(env._h, C.c_void_p(big.data_ptr() + 4 * off)) == _lib.SF_ERR_ARG, off
    with pytest.raises(ValueError):
        env.enable_final_obs(out=big[1:1 + n * env.obs_dim].view(n, env.obs_dim))
    with pytest.raises(ValueError):
        env.enable_final_obs(out=torch.zeros((n, env.obs_dim), dtype=torch.float64, device=env.device))
    assert env.final_obs is None
    env.set_field("time", np.full(n, 180000 - 34, np.int32))  # every lane finishes on the next tick: nothing may be written
    env.step_tensors(torch.zeros(n, dtype=torch.uint8, device=env.device))
    torch.cuda.synchronize()
    assert TR.untouched(big)
    TR.margins_intact(big)
    env.close()


# ---------------------------------------------------------------------------------------------------------------
# 6. a captured graph
def test_captured_steps_write_the_eager_runs_rows(sfa):
    n, K = 130, 8
    run = F.oracle_run("youturn", n)
    base = run["base"].copy()
    rng = np.random.default_rng(5)
    base["time"] = 180000 - 34 * rng.integers(2, 2 * K, n)  # finishes spread over both replays, none in the eager step in front
    base["time"][::7] = 34 * 100
    base["tick"] = base["time"] // 34
    acts = torch.from_numpy(run["acts"][:K].copy())
    res = []
    for captured in (False, True):
        env = sfa.SFVecEnv(n, gametype="youturn")
        F.load_env(env, base, run["pv"])
        dev = env.device
        fin = _guarded_rows(env)
        env.enable_final_obs(out=fin)
        a = acts.to(dev)
        outs = _outs(env, K)
        # one eager step first: the missile slots that load_env edited are folded back into the tiles' pools by the first launch
        # behind the edit, and that launch belongs in front of the graph, not into it
        env.step_tensors(a[0])
        torch.cuda.synchronize()
        assert TR.untouched(fin)
        if captured:
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                with torch.cuda.graph(g, stream=side):  # one stream, no parallel branches
                    for k in range(K):
                        env.step_tensors(a[k], out=tuple(x[k] for x in outs))
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize()
            assert TR.untouched(fin)  # (a capture runs nothing)
            mid = []
            for rep in range(2):
                g.replay()
                torch.cuda.synchronize()
                mid.append(_bytes(fin))
            del g
        else:
            mid = []
            for rep in range(2):
                for k in range(K):
                    env.step_tensors(a[k], out=tuple(x[k] for x in outs))
                torch.cuda.synchronize()
                mid.append(_bytes(fin))
        TR.margins_intact(fin)
        res.append((mid, [_bytes(x) for x in outs], env.state_dict()))
        env.close()
    (em, eo, es), (gm, go, gs) = res
    assert em[0] != em[1], "no lane finished in the second replay"
    assert gm == em and go == eo and all(np.array_equal(es[k], gs[k]) for k in es)
    rows = np.frombuffer(em[1], np.float32).reshape(n, -1)
    assert (~F.is_sentinel(rows)).sum() == n - -(-n // 7)
