"""Action repeat on the device (include/sfmi_repeat.h: sf_step_repeat; SFVecEnv.step_repeat / frame_skip).

1. parity with the oracle driven one env at a time through the contract's loop (tests/frameskipref.py), every window;
2. the final-observation rows, and DeviceRollout(time_limit_bootstrap=True) on window rewards;  3. K = 1 is sf_step, byte for
byte;  4. windows in which nobody finishes against a twin stepped tick by tick, also at 65 600 envs;  5. a whole tile finishing
mid-window;  6. action types, a bad action;  7. image batches, FrameStack;  8. SFVecNormalize, DeviceRollout, the episode log;
9. a captured graph;  10. refusals.

Tolerance of the observations: sfcompare.obs_close, the existing parity tests' rule.  Everything else is compared bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import finalobsref as F
import frameskipref as R
import trainerref as TR
from sfcompare import compare_state, obs_close
from lockstep import sfa

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _guarded_outs(env, W):
    n, dev = env.num_envs, env.device
    return (TR.guarded((W, n, env.obs_dim), env.obs_dtype, dev), TR.guarded((W, n), torch.int32, dev),
            TR.guarded((W, n), torch.uint8, dev), TR.guarded((W, n), torch.uint8, dev), TR.guarded((W, n), torch.uint8, dev))


def _play(env, acts, K, outs, after=None):
    """W windows of K through env.step_repeat into row w of `outs` (obs, rew, done, info, ticks)"""
    a = torch.from_numpy(np.array(acts)).to(env.device)
    for w in range(a.shape[0]):
        env.step_repeat(a[w], K, out=tuple(x[w] for x in outs[:4]), ticks_out=outs[4][w])
        if after is not None:
            after(w)
    torch.cuda.synchronize()
    TR.margins_intact(*outs)
    return [x.cpu().numpy() for x in outs]


def _check_against(run, env, got, f64):
    obs, rew, done, info, ticks = got
    assert np.array_equal(rew, run["rew"]), np.argwhere(rew != run["rew"])[:5]
    assert np.array_equal(done.astype(bool), run["done"]) and np.array_equal(info.astype(bool), run["info"])
    assert np.array_equal(ticks, run["ticks"]), np.argwhere(ticks != run["ticks"])[:5]
    ok = obs_close(obs, run["obs"], f64)
    assert ok.all(), np.argwhere(~ok)[:5]
    bad = compare_state(env.state_dict(), run["snaps"])
    assert not bad, bad
    st, want = env.episode_stats(), R.expected_stats(run)
    assert st[0] == want["episodes"] and st[1] == want["ret"] and st[2] == want["ret2"] and st[3] == want["kills"]
    if want["episodes"]:
        assert st[6] == want["lo"] and st[7] == want["hi"]


# ---------------------------------------------------------------------------------------------------------------
# 1. oracle parity, every window
def _parity(sfa, gametype, n, K, obs_type="features", f64=False, finish=None):
    run = R.oracle_windows(gametype, n, K, obs_type, True, finish)
    env = F.make_env(sfa, run, gametype, n, obs_type, f64)
    got = _play(env, run["acts"], K, _guarded_outs(env, run["acts"].shape[0]))
    _check_against(run, env, got, f64)
    env.close()


@pytest.mark.parametrize("gametype", ["youturn", "autoturn", "test-youturn"])
@pytest.mark.parametrize("K", [2, 3, 4, 16])
@pytest.mark.parametrize("n", [63, 64, 65, 130, 257])
def test_windows_equal_the_oracles(sfa, n, K, gametype):
    _parity(sfa, gametype, n, K)


@pytest.mark.parametrize("gametype", ["youturn", "autoturn", "test-youturn"])
@pytest.mark.parametrize("K", [2, 3, 4, 16])
def test_one_env_finishing_at_the_first_a_middle_and_the_last_tick(sfa, K, gametype):
    for finish in (K + 1, K + 1 + K // 2, 2 * K):
        _parity(sfa, gametype, 1, K, finish=finish)


@pytest.mark.parametrize("gametype", ["youturn", "autoturn", "test-youturn"])
@pytest.mark.parametrize("K", [2, 3, 4, 16])
@pytest.mark.parametrize("obs_type,f64", [("features", True), ("normalized-features", False), ("monitors", False)])
def test_windows_of_the_other_observations(sfa, obs_type, f64, K, gametype):
    _parity(sfa, gametype, 130, K, obs_type, f64)


# ---------------------------------------------------------------------------------------------------------------
# 2. the final observation
@pytest.mark.parametrize("K", [3, 4])
@pytest.mark.parametrize("n", [64, 130])
def test_final_rows_are_the_finishing_ticks(sfa, n, K):
    run = R.oracle_windows("youturn", n, K)
    env = F.make_env(sfa, run, "youturn", n)
    fin = TR.guarded((n, env.obs_dim), env.obs_dtype, env.device)
    env.enable_final_obs(out=fin)
    W = run["acts"].shape[0]
    hist = torch.empty((W,) + tuple(fin.shape), dtype=fin.dtype, device=env.device)
    got = _play(env, run["acts"], K, _guarded_outs(env, W), after=lambda w: hist[w].copy_(fin))
    TR.margins_intact(fin)
    _check_against(run, env, got, False)
    hist = hist.cpu().numpy()
    for w in range(W):
        want, finished = R.final_rows(run, w)
        assert F.is_sentinel(hist[w][~finished]).all(), (w, "a row of a lane that has not finished was written")
        if finished.any():
            ok = obs_close(hist[w][finished], want[finished], False)
            assert ok.all(), (w, np.argwhere(~ok)[:5])
    env.close()


def test_rollout_with_time_limit_bootstrap_on_window_rewards(sfa):
    import timelimit_np as TL

    n, K = 130, 4
    run = R.oracle_windows("youturn", n, K)
    T = run["acts"].shape[0]
    env = sfa.SFVecEnv(n, gametype="youturn", frame_skip=K)
    dev = env.device
    raw = torch.full((n, env.obs_dim), float("nan"), dtype=torch.float32, device=dev)
    env.enable_final_obs(out=raw)
    ro = sfa.DeviceRollout(env, T, time_limit_bootstrap=True)
    F.load_env(env, run["base"], run["pv"])
    g = torch.Generator().manual_seed(3)
    values = torch.randn(T, n, 1, generator=g).to(dev)
    a = torch.from_numpy(run["acts"].copy()).to(dev)
    for t in range(T):
        ro.step(t, a[t], value_pred=values[t])
    torch.cuda.synchronize()
    assert np.array_equal(env.last_ticks.cpu().numpy(), run["ticks"][-1])
    want, finished = R.final_rows(run)
    rawn = raw.cpu().numpy()
    assert np.isnan(rawn[~finished]).all() and obs_close(rawn[finished], want[finished], False).all()
    assert obs_close(ro.observations[1:].cpu().numpy(), run["obs"], False).all()
    w = torch.randn(env.obs_dim, generator=g).to(dev) * 0.1
    fv, nv = ro.final_obs() @ w, torch.randn(n, generator=g).to(dev)
    for gae in (True, False):
        ro.compute_returns(nv, gae, 0.99, 0.95, final_value=fv)
        torch.cuda.synchronize()
        rew, vp, masks = (x[:, :, 0].cpu().numpy() for x in (ro.rewards, ro.value_preds, ro.masks))
        assert np.array_equal(rew, run["rew"].astype(np.float32)) and np.array_equal(masks[1:] == 0, run["done"])
        model_ret, _ = TL.compute_returns_tl(rew, vp.copy(), masks, nv.cpu().numpy(), fv.cpu().numpy(), gae, 0.99, 0.95)
        rows = slice(0, T) if gae else slice(0, T + 1)
        TR.assert_bits_equal(ro.returns[:, :, 0].cpu().numpy()[rows], model_ret[rows], "returns, gae=%s" % gae)
    env.close()


# ---------------------------------------------------------------------------------------------------------------
# 3. K = 1 is sf_step
@pytest.mark.parametrize("n", [130, 128])
def test_repeat_one_is_the_single_step(sfa, n):
    run = F.oracle_run("youturn", n)
    T = F.T_RUN
    res = []
    for repeat in (False, True):
        env = F.make_env(sfa, run, "youturn", n)
        fin = TR.guarded((n, env.obs_dim), env.obs_dtype, env.device)
        env.enable_final_obs(out=fin)
        a = torch.from_numpy(run["acts"].copy()).to(env.device)
        outs = _guarded_outs(env, T)
        for t in range(T):
            if repeat:
                env.step_repeat(a[t], 1, out=tuple(x[t] for x in outs[:4]), ticks_out=outs[4][t])
            else:
                env.step_tensors(a[t], out=tuple(x[t] for x in outs[:4]))
        torch.cuda.synchronize()
        TR.margins_intact(fin, *outs)
        if repeat:
            assert (outs[4].cpu().numpy() == 1).all()
        res.append(([_bytes(x) for x in outs[:4]], _bytes(fin), _bytes(env.save_lanes().rows)))
        env.close()
    assert res[0] == res[1]
    assert np.frombuffer(res[0][0][2], np.uint8).sum() >= n - -(-n // 7)


# ---------------------------------------------------------------------------------------------------------------
# 4. windows in which nobody finishes
def _fresh_pair(sfa, n, gametype="youturn", **kw):
    envs = [sfa.SFVecEnv(n, gametype=gametype, spawn_stride=1, **kw) for _ in range(2)]
    for e in envs:
        e.reset()
        e.enable_events()
    return envs


@pytest.mark.parametrize("gametype", ["youturn", "autoturn"])
@pytest.mark.parametrize("n", [130, 128])
def test_quiet_windows_equal_four_single_steps(sfa, n, gametype):
    K, W = 4, 12
    env, twin = _fresh_pair(sfa, n, gametype)
    rng = np.random.default_rng(n)
    acts = torch.from_numpy(rng.integers(0, env.n_actions, (W, n)).astype(np.uint8)).to(env.device)
    for w in range(W):
        o, r, d, i = env.step_repeat(acts[w], K)
        rs, ii, ev = torch.zeros_like(r), torch.zeros_like(i), torch.zeros_like(env.events)
        for j in range(K):
            to, tr, td, ti = twin.step_tensors(acts[w])
            rs += tr
            ii |= ti
            ev |= twin.events
            assert not bool(td.any())
        assert _bytes(o) == _bytes(to) and torch.equal(r, rs) and torch.equal(i, ii) and not bool(d.any()), w
        assert torch.equal(env.events, ev) and bool((env.last_ticks == K).all()), w
        assert _bytes(env.save_lanes().rows) == _bytes(twin.save_lanes().rows), w
    assert bool(ev.any())
    env.close()
    twin.close()


def test_every_env_of_a_large_batch_plays_the_game_it_would_play_alone(sfa):
    K, W, n = 4, 12, 130
    big = sfa.SFVecEnv(65600, gametype="youturn", spawn_stride=1)
    small = sfa.SFVecEnv(n, gametype="youturn", spawn_stride=1)
    big.reset()
    small.reset()
    rng = np.random.default_rng(1)
    acts = rng.integers(0, 5, (W, 65600)).astype(np.uint8)
    ab = torch.from_numpy(acts).to(big.device)
    asm = torch.from_numpy(np.ascontiguousarray(acts[:, :n])).to(big.device)
    lanes = torch.arange(n, device=big.device)
    for w in range(W):
        ob, rb, db, ib = big.step_repeat(ab[w], K)
        os_, rs, ds, is_ = small.step_repeat(asm[w], K)
        assert _bytes(ob[:n]) == _bytes(os_) and torch.equal(rb[:n], rs) and torch.equal(ib[:n], is_) and not bool(db.any()), w
    # (a row's 16-byte header names the batch's spawn table, whose length grows with the batch: the states behind it)
    assert _bytes(big.save_lanes(lanes).rows[:, 16:]) == _bytes(small.save_lanes().rows[:, 16:])
    assert np.array_equal(big.lane_state_header()[:3], small.lane_state_header()[:3])
    big.check_state()
    big.close()
    small.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. a whole tile finishing mid-window
@pytest.mark.parametrize("n", [64, 128])
def test_a_whole_tile_finishes_at_tick_two_of_four(sfa, n):
    K = 4
    base, pv, rng = R.start_state("youturn", n)
    base["time"][:] = 180000 - 34 * 2
    base["tick"] = base["time"] // 34
    acts = rng.integers(0, 5, (3, n)).astype(np.uint8)
    run = R.run_windows("youturn", n, K, base, pv, acts)
    assert run["done"][0].all() and (run["ticks"][0] == 2).all() and not run["done"][1:].any()
    env = sfa.SFVecEnv(n, gametype="youturn")
    F.load_env(env, base, pv)
    outs = _guarded_outs(env, 3)
    a = torch.from_numpy(np.array(acts)).to(env.device)
    env.step_repeat(a[0], K, out=tuple(x[0] for x in outs[:4]), ticks_out=outs[4][0])
    torch.cuda.synchronize()
    assert not env.get_field("missile_mask").any() and not env.get_field("shell_mask").any()
    assert (env.get_field("time") == 0).all()  # no tick of the new game has been played
    for w in (1, 2):
        env.step_repeat(a[w], K, out=tuple(x[w] for x in outs[:4]), ticks_out=outs[4][w])
    torch.cuda.synchronize()
    TR.margins_intact(*outs)
    _check_against(run, env, [x.cpu().numpy() for x in outs], False)
    env.close()


# ---------------------------------------------------------------------------------------------------------------
# 6. action types; an action outside the action set
def test_action_types_agree_and_a_bad_action_plays_noop(sfa):
    n, K = 130, 3
    run = R.oracle_windows("youturn", n, K)
    res = []
    for dt in (torch.uint8, torch.int32, torch.int64):
        env = F.make_env(sfa, run, "youturn", n)
        a = torch.from_numpy(run["acts"].astype(np.int64)).to(env.device).to(dt)
        outs = _guarded_outs(env, a.shape[0])
        for w in range(a.shape[0]):
            env.step_repeat(a[w], K, out=tuple(x[w] for x in outs[:4]), ticks_out=outs[4][w])
        torch.cuda.synchronize()
        env.check_actions()
        res.append(([_bytes(x) for x in outs], _bytes(env.save_lanes().rows)))
        env.close()
    assert res[0] == res[1] == res[2]
    # an id outside the action set: NOOP for the whole window, reported
    noop = run["acts"].astype(np.int32).copy()
    noop[:, 5::9] = 0
    bad = noop.copy()
    bad[:, 5::9] = 77
    bad[0, 5] = -3
    got = []
    for acts, raises in ((noop, False), (bad, True)):
        env = F.make_env(sfa, run, "youturn", n)
        a = torch.from_numpy(acts).to(env.device)
        outs = _guarded_outs(env, a.shape[0])
        for w in range(a.shape[0]):
            env.step_repeat(a[w], K, out=tuple(x[w] for x in outs[:4]), ticks_out=outs[4][w])
        torch.cuda.synchronize()
        if raises:
            with pytest.raises(IndexError):
                env.check_actions()
        env.check_actions()
        got.append(([_bytes(x) for x in outs], _bytes(env.save_lanes().rows)))
        env.close()
    assert got[0] == got[1]


# ---------------------------------------------------------------------------------------------------------------
# 7. image batches
def _live_record_bytes(rec):
    """The bytes of draw records [N, 432] (sf_drawrec.h) that mean something: the header, the ship's position, the positions
    and headings of the LIVE missile slots (as in test_gpu_image.py)."""
    n = rec.shape[0]
    assert rec.shape[1] == 432
    live = np.zeros((n, 432), bool)
    live[:, :48] = True
    objmask = rec[:, 12:16].copy().view(np.uint32)[:, 0]
    for s in range(20):
        on = ((objmask >> (2 + s)) & 1).astype(bool)[:, None]
        live[:, 64 + 16 * s:80 + 16 * s] = on
        live[:, 384 + 2 * s:386 + 2 * s] = on
    return np.where(live, rec, 0)


def _image_env(sfa, n, rng, **kw):
    """an image batch under way whose lanes finish 1 .. 40 ticks from now (every 7th nowhere near it)"""
    env = sfa.SFVecEnv(n, gametype="youturn", obs_type="image", spawn_stride=1, **kw)
    env.reset()
    warm = torch.from_numpy(rng.integers(0, 5, (40, n)).astype(np.uint8)).to(env.device)
    env.rollout(warm, want_obs=False)
    clock = (180000 - 34 * (1 + np.arange(n) % 41)).astype(np.int32)
    clock[::7] = 34 * 100
    env.set_field("time", clock)
    return env


def test_image_windows_return_the_frames_of_the_state(sfa):
    import framestack_np as FS

    n, K, W, S = 130, 4, 12, 4
    rng = np.random.default_rng(9)
    env = _image_env(sfa, n, rng)
    stk_env = _image_env(sfa, n, np.random.default_rng(9), frame_skip=K)
    stk = sfa.FrameStack(stk_env, S)
    model = stk.ring.cpu().numpy().copy()
    head = stk.head
    acts = torch.from_numpy(rng.integers(0, 5, (W, n)).astype(np.uint8)).to(env.device)
    n_done = 0
    for w in range(W):
        frames, r, d, i = env.step_repeat(acts[w], K)
        torch.cuda.synchronize()
        assert _bytes(frames) == _bytes(env.render("image")), w
        assert _live_record_bytes(env.draw_records(False)).tobytes() == _live_record_bytes(env.draw_records(True)).tobytes(), w
        r2, d2, i2 = stk.step(acts[w])
        assert torch.equal(r2, r) and torch.equal(d2.view(torch.uint8), d) and torch.equal(i2.view(torch.uint8), i), w
        head = (head + 1) % S
        model = FS.render_stack(model, frames.cpu().numpy()[:, 0], head, d.cpu().numpy())
        assert stk.head == head and stk.ring.cpu().numpy().tobytes() == model.tobytes(), w
        n_done += int(d.sum())
    assert n_done == n - -(-n // 7)
    env.close()
    stk_env.close()


# ---------------------------------------------------------------------------------------------------------------
# 8. the wrappers and the episode log
def test_vecnormalize_follows_the_windows(sfa):
    import normref as NR

    n, K, W = 130, 3, 16
    run = R.oracle_windows("youturn", n, K)
    raw = F.make_env(sfa, run, "youturn", n)
    env = F.make_env(sfa, run, "youturn", n, frame_skip=K)
    z = sfa.SFVecNormalize(env)
    ex = NR.ExactVecNormalize(n, env.obs_dim)
    d_s = NR.depth_standalone(n, env.obs_dim)
    a = torch.from_numpy(run["acts"].copy()).to(env.device)
    for w in range(W):
        o_raw, r_raw, d_raw, i_raw = raw.step_repeat(a[w], K)
        o, rn, d, i = z.step_tensors(a[w])
        assert torch.equal(d, d_raw) and torch.equal(i, i_raw), w
        want, tol, wr, tr = ex.step(o_raw.cpu().numpy().astype(np.float64), r_raw.cpu().numpy(), np.float32, *d_s)
        NR.check("frame_skip", "obs", o.cpu().numpy(), want, tol, where="window %d" % w)
        NR.check("frame_skip", "rew", rn.cpu().numpy(), wr, tr, where="window %d" % w)
    assert np.array_equal(env.last_ticks.cpu().numpy(), run["ticks"][W - 1])
    z.close()
    raw.close()


def test_device_rollout_and_the_episode_log_count_agent_steps(sfa):
    from eplog_np import NpEpisodeLog

    n, K = 130, 3
    run = R.oracle_windows("youturn", n, K)
    T = run["acts"].shape[0]
    env = F.make_env(sfa, run, "youturn", n, frame_skip=K)
    log = env.enable_episode_log(capacity=512, hist=(-60, 100))
    ro = sfa.DeviceRollout(env, T)
    a = torch.from_numpy(run["acts"].copy()).to(env.device)
    ep, fin = np.zeros(n, np.float32), np.zeros(n, np.float32)
    for t in range(T):
        ro.step(t, a[t])
        torch.cuda.synchronize()
        r, m, ep, fin, act = TR.record_step(run["rew"][t], run["done"][t].astype(np.uint8), ep, fin, run["acts"][t])
        TR.assert_bits_equal(ro.rewards[t, :, 0], r, "rewards %d" % t)
        TR.assert_bits_equal(ro.masks[t + 1, :, 0], m, "masks %d" % t)
        TR.assert_bits_equal(ro.episode_rewards[:, 0], ep, "episode_rewards %d" % t)
        TR.assert_bits_equal(ro.final_rewards[:, 0], fin, "final_rewards %d" % t)
        assert np.array_equal(ro.actions[t, :, 0].cpu().numpy(), act)
    assert obs_close(ro.observations[1:].cpu().numpy(), run["obs"], False).all()
    model = NpEpisodeLog(n, log.capacity, log.hist_lo, log.bins)
    recs, seq = model.update(run["rew"], run["done"], run["info"], run["acts"])
    got = log.drain()
    for k in ("env", "episode_return", "length", "kills", "fire_actions", "end_row"):
        assert np.array_equal(got[k], recs[k]), k
    assert len(recs) == n - -(-n // 7) and log.rows_seen == T  # lengths in agent steps: one row per window
    env.close()


# ---------------------------------------------------------------------------------------------------------------
# 9. a captured graph
def test_captured_windows_equal_the_eager_ones(sfa):
    n, K = 130, 4
    run = R.oracle_windows("youturn", n, K)
    base = run["base"].copy()
    base["time"] = 180000 - 34 * (6 + np.arange(n) % 17)  # finishes spread over both replays, none in the eager call in front
    base["time"][::7] = 3400
    base["tick"] = base["time"] // 34
    res = []
    for captured in (False, True):
        env = sfa.SFVecEnv(n, gametype="youturn")
        F.load_env(env, base, run["pv"])
        dev = env.device
        a = torch.from_numpy(run["acts"][:3].copy()).to(dev)
        outs = _guarded_outs(env, 3)
        # one eager call first: the missile slots load_env edited are folded back into the pools by the first launch behind it
        env.step_repeat(a[0], K)
        torch.cuda.synchronize()
        mid = []
        if captured:
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                with torch.cuda.graph(g, stream=side):  # one stream, no parallel branches
                    for k in range(3):
                        env.step_repeat(a[k], K, out=tuple(x[k] for x in outs[:4]), ticks_out=outs[4][k])
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize()
            assert TR.untouched(*outs)  # (a capture runs nothing)
            for rep in range(2):
                g.replay()
                torch.cuda.synchronize()
                mid.append([_bytes(x) for x in outs])
            del g
        else:
            for rep in range(2):
                for k in range(3):
                    env.step_repeat(a[k], K, out=tuple(x[k] for x in outs[:4]), ticks_out=outs[4][k])
                torch.cuda.synchronize()
                mid.append([_bytes(x) for x in outs])
        TR.margins_intact(*outs)
        res.append((mid, _bytes(env.save_lanes().rows)))
        env.close()
    assert res[0] == res[1]
    for rep in range(2):
        assert np.frombuffer(res[0][0][rep][2], np.uint8).any(), "no lane finished in replay %d" % rep


# ---------------------------------------------------------------------------------------------------------------
# 10. refusals
def test_refusals_leave_the_batch_as_it_was(sfa):
    from spacefortress_amd import _lib

    L = _lib.lib()
    n = 65
    env = sfa.SFVecEnv(n)
    env.reset()
    a = torch.ones(n, dtype=torch.uint8, device=env.device)
    env.step_tensors(a)
    before = _bytes(env.save_lanes().rows)
    outs = _guarded_outs(env, 1)
    p = lambda t: C.c_void_p(t.data_ptr())
    args = lambda: [env._h, p(a), 1, 4, p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), p(outs[4]), env._stream()]
    for i, v in ((3, 0), (3, 256), (3, -1), (1, None), (2, 2), (2, 0), (0, None)):
        b = args()
        b[i] = v
        assert L.sf_step_repeat(*b) == _lib.SF_ERR_ARG, (i, v)
        assert "sf_step_repeat" in _lib.last_error()
    for rep in (0, 256):
        with pytest.raises(ValueError):
            env.step_repeat(a, rep)
    env.enable_durations()
    with pytest.raises(RuntimeError):
        env.step_repeat(a, 4)
    env._durations = None
    torch.cuda.synchronize()
    assert TR.untouched(*outs) and _bytes(env.save_lanes().rows) == before
    env.close()
    # a batch without auto-reset
    with pytest.raises(ValueError):
        sfa.SFVecEnv(n, auto_reset=False, frame_skip=2)
    with pytest.raises(ValueError):
        sfa.SFVecEnv(n, frame_skip=0)
    env = sfa.SFVecEnv(n, auto_reset=False)
    env.reset()
    before = _bytes(env.save_lanes().rows)
    b = [env._h, p(a), 1, 4, p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), p(outs[4]), env._stream()]
    assert L.sf_step_repeat(*b) == _lib.SF_ERR_ARG and "SF_FLAG_NO_AUTO_RESET" in _lib.last_error()
    with pytest.raises(ValueError):
        env.step_repeat(a, 4)
    torch.cuda.synchronize()
    assert TR.untouched(*outs) and _bytes(env.save_lanes().rows) == before
    env.close()
    # a recording
    env = sfa.SFVecEnv(n, frame_skip=2)
    with pytest.raises(RuntimeError):
        env.start_recording()
    env.close()
    env = sfa.SFVecEnv(n)
    env.start_recording()
    with pytest.raises(RuntimeError):
        env.step_repeat(a, 2)
    env.step_repeat(a, 1)  # (sf_step: a replay file can hold it)
    env.close()
