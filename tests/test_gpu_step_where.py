"""The masked step on the device (include/sfmi_hold.h: sf_step_where; SFVecEnv.step_where): chosen envs tick, the others hold.

1. lock-step against the model of tests/holdref.py (one oracle env per lane, only the active lanes stepped), every call;
2. schedule independence: a lane's c-th active step equals step c of a twin batch stepped plainly, games that end included;
3. held means untouched: lane rows, the final-observation and event buffers, episode_stats, a batch without auto-reset;
4. edges of the mask: all ones is sf_step, all zeros changes nothing, any non-zero byte, every output NULL in turn;
5. action repeat next to held envs;  6. image batches against a twin;  7. beyond one wave per SIMD (66 000 envs);
8. a captured graph;  9. every refusal, C and Python.

Observations against the oracle here: sfcompare.obs_close, the existing parity tests' rule for rows of games under way (the
oracle's own bearings are glibc's, not the 70-digit reference).  The bounds of DESIGN 9 on the held lanes' rows -- bearings
within 1.88e-13 / 2.18e-13 degrees, ndist and every other column exact, float32 and float64, features, normalized-features and
monitors, SF_FLAG_REF_RESET_OBS -- are tests/test_gpu_step_where_bearings.py's.  Against a twin batch: byte for byte.
Everything else: bit for bit.
"""
import ctypes as C

import numpy as np
import pytest

import holdref as H
import trainerref as TR
from finalobsref import is_sentinel
from lockstep import fuzz_crowded, load_state, sfa  # noqa: F401  (sfa: the fixture)
from sfcompare import compare_state, obs_close

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _bytes(t):
    return t.cpu().numpy().tobytes()


def _outs(env):
    n, dev = env.num_envs, env.device
    return (TR.guarded((n,) + tuple(env.obs_shape), env.obs_dtype, dev), TR.guarded(n, torch.int32, dev), TR.guarded(n, torch.uint8, dev),
            TR.guarded(n, torch.uint8, dev), TR.guarded(n, torch.uint8, dev))


def _busy_actions(rng, n_act, shape):
    """actions that fire and thrust often (ids 1 and 2 of action set 1): pools and shell slots are populated when lanes are held"""
    a = rng.integers(0, n_act, shape)
    return np.where(rng.random(shape) < 0.5, rng.integers(1, 3, shape), a).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------
# 1. lock-step against the model
@pytest.mark.parametrize("auto_reset", [True, False])
@pytest.mark.parametrize("gametype", ["youturn", "autoturn"])
def test_every_call_equals_the_models(sfa, gametype, auto_reset):
    from oracle import oracle as O

    n, T = 200, 240  # three whole tiles and a partial one of 8
    rng = np.random.default_rng([41, len(gametype), int(auto_reset)])
    base, pv = fuzz_crowded(O, gametype, n, rng)
    base["time"] = 180000 - 34 * rng.integers(1, T // 2, n)  # games end inside the run, next to held tile-mates
    base["time"][::7] = 3400
    base["tick"] = base["time"] // 34
    model = H.HoldModel(gametype, base, pv, auto_reset=auto_reset)
    env = sfa.SFVecEnv(n, gametype=gametype, auto_reset=auto_reset)
    load_state(env, base, pv)
    env.enable_events()
    fin = None
    if auto_reset:
        fin = TR.guarded((n, env.obs_dim), env.obs_dtype, env.device)
        env.enable_final_obs(out=fin)
    fin_model = np.full((n, env.obs_dim), np.nan)
    acts = _busy_actions(rng, model.n_actions, (T, n))
    masks = H.draw_masks(rng, n, T)
    a_dev, m_dev = torch.from_numpy(acts).to(env.device), torch.from_numpy(masks).to(env.device)
    outs = _outs(env)
    bearing = np.zeros(env.obs_dim, bool)
    bearing[list(H.BEARING_COLUMNS)] = True
    held_with_missiles = 0
    for t in range(T):
        if t % 16 == 0:
            held_with_missiles += int((env.get_field("missile_mask")[~masks[t]] != 0).sum())
        env.step_where(a_dev[t], m_dev[t], out=outs[:4], ticks_out=outs[4])
        want = model.step_where(acts[t], masks[t])
        obs, rew, done, info, ticks = (x.cpu().numpy() for x in outs)
        assert np.array_equal(rew, want["rew"]), (t, np.flatnonzero(rew != want["rew"])[:5])
        assert np.array_equal(done.astype(bool), want["done"]) and np.array_equal(info.astype(bool), want["info"]), t
        assert np.array_equal(ticks, want["ticks"]) and np.array_equal(ticks, masks[t].astype(np.uint8)), t
        ok = obs_close(obs, want["obs"], False) | (bearing[None, :] & ~model.seen[:, None])
        assert ok.all(), (t, np.argwhere(~ok)[:5], masks[t][np.argwhere(~ok)[:5, 0]])
        assert not env.events.cpu().numpy()[~masks[t]].any(), t
        bad = compare_state(env.state_dict(), model.snapshots())
        assert not bad, (t, bad)
        finished = ~np.isnan(want["final"][:, 0])
        fin_model[finished] = want["final"][finished]
    TR.margins_intact(*outs)
    assert held_with_missiles > 50
    st, ws = env.episode_stats(), model.expected_stats()
    assert (st[0], st[1], st[2], st[3]) == (ws["episodes"], ws["ret"], ws["ret2"], ws["kills"])
    if auto_reset:
        assert ws["episodes"] >= n // 2
        TR.margins_intact(fin)
        f = fin.cpu().numpy()
        got = ~np.isnan(fin_model[:, 0])
        assert is_sentinel(f[~got]).all() and obs_close(f[got], fin_model[got], False).all()
    env.check_actions()
    env.close()


# ---------------------------------------------------------------------------------------------------------------
# 2. / 7. schedule independence
def _schedule_pair(sfa, n, T, seed, gametype="youturn", near_end=True, p=0.5):
    """Two batches of one seed: A plain-stepped T times (every output kept), B masked for 2 T calls in which lane i plays the
    action of ITS c-th step.  All on the device; -> the number of B's (lane, call) pairs that were active."""
    A, B = (sfa.SFVecEnv(n, gametype=gametype, spawn_stride=1, seed=seed) for _ in range(2))
    dev = A.device
    rng = np.random.default_rng([seed, n])
    for e in (A, B):
        e.reset()
        e.enable_events()
    warm = torch.from_numpy(_busy_actions(rng, A.n_actions, (30, n))).to(dev)
    clock = (180000 - 34 * (1 + np.arange(n) % (T - 2))).astype(np.int32)  # the auto-reset and the spawn stream are crossed
    clock[::7] = 34 * 100
    for e in (A, B):
        e.rollout(warm, want_obs=False)
        if near_end:
            e.set_field("time", clock)
    acts = torch.from_numpy(_busy_actions(rng, A.n_actions, (T, n))).to(dev)
    hist = []
    for t in range(T):
        o, r, d, i = A.step_tensors(acts[t])
        hist.append((o.clone(), r.clone(), d.clone(), i.clone(), A.events.clone()))
    ho, hr, hd, hi, he = (torch.stack(x) for x in zip(*hist))
    c = torch.zeros(n, dtype=torch.int64, device=dev)
    lanes = torch.arange(n, device=dev)
    g = torch.Generator(device="cpu").manual_seed(seed)
    bad = torch.zeros((), dtype=torch.int64, device=dev)
    played = 0
    prev = None
    for t in range(2 * T):
        m = (torch.rand(n, generator=g) < p).to(dev) & (c < T)
        a = acts[c.clamp(max=T - 1), lanes]
        o, r, d, i = B.step_where(a, m)
        cc = c.clamp(max=T - 1)
        same = ((o == ho[cc, lanes]).all(1) & (r == hr[cc, lanes]) & (d == hd[cc, lanes]) & (i == hi[cc, lanes])
                & (B.events == he[cc, lanes]) & (B.last_ticks == 1))
        quiet = (r == 0) & (d == 0) & (i == 0) & (B.events == 0) & (B.last_ticks == 0)
        if prev is not None:  # a held lane shows the observation of its unchanged state: the integer columns of its last row
            quiet &= (o[:, [0, 5, 9, 10, 11, 12, 13, 14]] == prev[:, [0, 5, 9, 10, 11, 12, 13, 14]]).all(1) | (c == 0)
        bad += (~torch.where(m, same, quiet)).sum()
        played += int(m.sum())
        c += m.long()
        prev = o.clone()
    done_total = int(hd.sum())
    n_bad = int(bad)
    # lanes that played all T steps hold the state A's do
    full = (c == T).nonzero()[:, 0]
    rows_a, rows_b = A.save_lanes(full).rows, B.save_lanes(full).rows
    same_rows = _bytes(rows_a) == _bytes(rows_b)
    B.check_state()
    A.close()
    B.close()
    return n_bad, played, done_total, int(full.numel()), same_rows


def test_a_lanes_cth_active_step_is_step_c_of_a_plain_twin(sfa):
    n, T = 200, 60
    n_bad, played, done_total, full, same_rows = _schedule_pair(sfa, n, T, 3)
    assert n_bad == 0
    assert done_total >= n // 2 and full >= n // 4 and same_rows


def test_beyond_one_wave_per_simd(sfa):
    """66 000 envs: the regime in which a wide store without its wait state loses lanes 12-15 of every 16 (build.py's scan)"""
    n, T = 66000, 20
    n_bad, played, done_total, full, same_rows = _schedule_pair(sfa, n, T, 5, near_end=False)
    assert n_bad == 0 and played > n * T // 2 and full > n // 10 and same_rows


# ---------------------------------------------------------------------------------------------------------------
# 3. held means untouched
def test_held_lanes_are_untouched(sfa):
    from oracle import oracle as O

    n = 200
    rng = np.random.default_rng(8)
    base, pv = fuzz_crowded(O, "youturn", n, rng)
    base["time"] = 180000 - 34 * rng.integers(2, 20, n)  # every lane would finish within 20 ticks, none in the plain step below
    base["tick"] = base["time"] // 34
    env = sfa.SFVecEnv(n, gametype="youturn")
    load_state(env, base, pv)
    dev = env.device
    fin = TR.guarded((n, env.obs_dim), env.obs_dtype, dev)
    env.enable_final_obs(out=fin)
    ev = TR.guarded(n, torch.int32, dev)
    from spacefortress_amd import _lib
    _lib.check(env._L.sf_set_event_output(env._h, C.c_void_p(ev.data_ptr())))
    env.step_tensors(torch.zeros(n, dtype=torch.uint8, device=dev))  # (the first launch folds the edited missile slots into the pools)
    TR.refill(fin, ev)
    mask = torch.from_numpy(rng.random(n) < 0.5).to(dev)
    mask[:64] = True
    mask[64:128] = False
    held = (~mask).nonzero()[:, 0]
    before = _bytes(env.save_lanes(held).rows)
    assert int((env.get_field("missile_mask")[(~mask).cpu().numpy()] != 0).sum()) > 20
    env.episode_stats(clear=True)
    outs = _outs(env)
    n_done = torch.zeros(n, dtype=torch.int64, device=dev)
    for t in range(30):
        a = torch.from_numpy(_busy_actions(rng, env.n_actions, n)).to(dev)
        o, r, d, i = env.step_where(a, mask, out=outs[:4], ticks_out=outs[4])
        n_done += d
    torch.cuda.synchronize()
    TR.margins_intact(fin, ev, *outs)
    assert _bytes(env.save_lanes(held).rows) == before
    hm = (~mask).cpu().numpy()
    assert is_sentinel(fin.cpu().numpy()[hm]).all() and not is_sentinel(fin.cpu().numpy()[~hm]).any()
    # the event word of a held env is part of its output row: 0 (sfmi_hold.h), never the tick's
    assert not ev.cpu().numpy()[hm].any()
    assert not n_done[held].any() and bool((n_done[mask] == 1).all())
    assert env.episode_stats()[0] == int(mask.sum())
    env.close()


def test_finished_lanes_of_a_batch_without_auto_reset_keep_their_game_over(sfa):
    n, k = 130, 400
    env = sfa.SFVecEnv(n, gametype="youturn", auto_reset=False, spawn_stride=1)
    env.reset()
    dev = env.device
    rng = np.random.default_rng(2)
    env.rollout(torch.from_numpy(_busy_actions(rng, 5, (40, n))).to(dev), want_obs=False)
    clock = (180000 - 34 * (1 + np.arange(n) % 50)).astype(np.int32)
    env.set_field("time", clock)
    active = torch.ones(n, dtype=torch.bool, device=dev)
    a = torch.from_numpy(_busy_actions(rng, 5, (k, n))).to(dev)
    frozen = None
    for t in range(k):
        o, r, d, i = env.step_where(a[t], active)
        active &= d == 0  # a finished lane is held from its next call on
        if t == 60:
            assert not bool(active.any())
            frozen = _bytes(env.save_lanes().rows)
    assert _bytes(env.save_lanes().rows) == frozen
    time = env.get_field("time")
    assert (time >= 180000).all() and (time < 180000 + 34).all()
    env.check_state()
    assert env.episode_stats()[0] == 0  # (a batch without auto-reset accumulates no episode: as sf_step)
    env.close()


# ---------------------------------------------------------------------------------------------------------------
# 4. edges of the mask
def _twin_envs(sfa, n, seed=4, warm=40, **kw):
    envs = [sfa.SFVecEnv(n, spawn_stride=1, **kw) for _ in range(2)]
    rng = np.random.default_rng(seed)
    w = torch.from_numpy(_busy_actions(rng, envs[0].n_actions, (warm, n))).to(envs[0].device)
    for e in envs:
        e.reset()
        if not e.is_image:
            e.enable_events()
        e.rollout(w, want_obs=False)
    return envs, rng


@pytest.mark.parametrize("n", [200, 256])
def test_an_all_ones_mask_is_the_plain_step_and_an_all_zero_mask_nothing(sfa, n):
    (env, twin), rng = _twin_envs(sfa, n)
    dev = env.device
    ones = torch.from_numpy(rng.integers(1, 256, n).astype(np.uint8)).to(dev)  # bytes other than 1 count as set
    zeros = torch.zeros(n, dtype=torch.uint8, device=dev)
    outs, touts = _outs(env), _outs(twin)
    for t in range(20):
        a = torch.from_numpy(_busy_actions(rng, env.n_actions, n)).to(dev)
        env.step_where(a, ones, out=outs[:4], ticks_out=outs[4])
        twin.step_tensors(a, out=touts[:4])
        assert [_bytes(x) for x in outs[:4]] == [_bytes(x) for x in touts[:4]], t
        assert bool((outs[4] == 1).all()) and torch.equal(env.events, twin.events)
    assert _bytes(env.save_lanes().rows) == _bytes(twin.save_lanes().rows)
    sa, sb = env.state_dict(), twin.state_dict()
    assert all(np.asarray(sa[k]).tobytes() == np.asarray(sb[k]).tobytes() for k in sa)
    last = outs[0].clone()
    env.step_where(a, zeros, out=outs[:4], ticks_out=outs[4])
    torch.cuda.synchronize()
    TR.margins_intact(*outs)
    assert _bytes(env.save_lanes().rows) == _bytes(twin.save_lanes().rows)
    assert not any(bool(x.any()) for x in outs[1:]) and not bool(env.events.any())
    assert obs_close(outs[0].cpu().numpy(), last.cpu().numpy().astype(np.float64), False).all()
    assert np.array_equal(env.episode_stats(), twin.episode_stats())
    env.close()
    twin.close()


def test_every_output_may_be_null(sfa):
    from spacefortress_amd import _lib

    n = 200
    (env, twin), rng = _twin_envs(sfa, n)
    L, dev = _lib.lib(), env.device
    p = lambda t: C.c_void_p(t.data_ptr())
    mask = torch.from_numpy((rng.random(n) < 0.5).astype(np.uint8) * 3).to(dev)
    for null in range(5):
        a = torch.from_numpy(_busy_actions(rng, env.n_actions, n)).to(dev)
        outs, touts = _outs(env), _outs(twin)
        ptrs = [p(x) for x in outs]
        ptrs[null] = None
        _lib.check(L.sf_step_where(env._h, p(mask), p(a), 1, 1, *ptrs, env._stream()))
        twin.step_where(a, mask, out=touts[:4], ticks_out=touts[4])
        torch.cuda.synchronize()
        TR.margins_intact(*outs)
        for k in range(5):
            assert TR.untouched(outs[k]) if k == null else _bytes(outs[k]) == _bytes(touts[k]), (null, k)
        assert _bytes(env.save_lanes().rows) == _bytes(twin.save_lanes().rows)
    env.close()
    twin.close()


# ---------------------------------------------------------------------------------------------------------------
# 5. action repeat
@pytest.mark.parametrize("gametype", ["youturn", "autoturn"])
def test_windows_next_to_held_envs_equal_the_models(sfa, gametype):
    from oracle import oracle as O

    n, K, W = 200, 4, 40
    rng = np.random.default_rng([43, len(gametype)])
    base, pv = fuzz_crowded(O, gametype, n, rng)
    base["time"] = 180000 - 34 * rng.integers(1, 2 * W, n)  # finishes at every tick of a window, beside held tile-mates
    base["time"][::7] = 3400
    base["tick"] = base["time"] // 34
    model = H.HoldModel(gametype, base, pv)
    env = sfa.SFVecEnv(n, gametype=gametype, frame_skip=K)
    load_state(env, base, pv)
    acts = _busy_actions(rng, model.n_actions, (W, n))
    masks = H.draw_masks(rng, n, W, stretch=6)
    a_dev, m_dev = torch.from_numpy(acts).to(env.device), torch.from_numpy(masks).to(env.device)
    outs = _outs(env)
    bearing = np.zeros(env.obs_dim, bool)
    bearing[list(H.BEARING_COLUMNS)] = True
    seen_ticks = set()
    for w in range(W):
        env.step_where(a_dev[w], m_dev[w], out=outs[:4], ticks_out=outs[4])
        want = model.step_where(acts[w], masks[w], K)
        obs, rew, done, info, ticks = (x.cpu().numpy() for x in outs)
        assert np.array_equal(rew, want["rew"]) and np.array_equal(done.astype(bool), want["done"]), w
        assert np.array_equal(info.astype(bool), want["info"]) and np.array_equal(ticks, want["ticks"]), w
        assert not ticks[~masks[w]].any() and torch.equal(env.last_ticks, outs[4])
        ok = obs_close(obs, want["obs"], False) | (bearing[None, :] & ~model.seen[:, None])
        assert ok.all(), (w, np.argwhere(~ok)[:5])
        bad = compare_state(env.state_dict(), model.snapshots())
        assert not bad, (w, bad)
        seen_ticks |= set(ticks[want["done"]].tolist())
    TR.margins_intact(*outs)
    assert seen_ticks == set(range(1, K + 1))  # parked at every tick of the window
    st, ws = env.episode_stats(), model.expected_stats()
    assert (st[0], st[1], st[2], st[3]) == (ws["episodes"], ws["ret"], ws["ret2"], ws["kills"]) and ws["episodes"] >= n // 3
    env.close()


# ---------------------------------------------------------------------------------------------------------------
# 6. image batches
@pytest.mark.parametrize("obs_type", ["image", "image-raw"])
def test_frames_of_active_lanes_are_the_twins_and_held_frames_stay(sfa, obs_type):
    from oracle import oracle as O

    n, T = 128, 10
    rng = np.random.default_rng(6)
    base, pv = fuzz_crowded(O, "youturn", n, rng)
    # four even lanes fly into the small hexagon (radius 40 around (355, 315)) inside the window, with no shell to die of first;
    # four odd lanes are 300 ms into their explosion
    crash, burning = [4, 36, 68, 100], [5, 37, 69, 101]
    base["ship_alive"][crash] = 1
    base["ship_x"][crash], base["ship_y"][crash] = 425.0, 315.0
    base["ship_vx"][crash], base["ship_vy"][crash] = -8.0, 0.0
    base["shell_alive"][crash] = 0
    base["ship_alive"][burning] = 0
    base["ship_death_timer"][burning] = 300
    envs = [sfa.SFVecEnv(n, gametype="youturn", obs_type=obs_type) for _ in range(2)]
    env, twin = envs
    for e in envs:
        load_state(e, base, pv)
    dev = env.device
    acts = torch.from_numpy(_busy_actions(rng, 5, (T, n))).to(dev)
    even = (torch.arange(n, device=dev) % 2 == 0)
    window = range(2, 7)  # the odd lanes are held in these calls; the even lanes stay in lock-step with the twin
    c = torch.zeros(n, dtype=torch.int64, device=dev)
    lanes = torch.arange(n, device=dev)
    # the twin first: frames, liveness and death timers of every step
    tf, alive, death = [], [], []
    for t in range(T):
        tf.append(twin.step_tensors(acts[t])[0].clone())
        alive.append((twin.get_field("flags") & 1).astype(bool))
        death.append(twin.get_field("ship_death_timer").copy())
    tf = torch.stack(tf)
    odd = ~even.cpu().numpy()
    # the conditions of the test, on the twin: an odd lane is held in mid-explosion; an even lane dies beside held tile-mates
    assert (~alive[1][odd] & (death[1][odd] < 1000 - 34 * len(window))).any()
    assert any((alive[t - 1][~odd] & ~alive[t][~odd]).any() for t in window)
    prev = None
    for t in range(T + len(window)):
        m = (even | torch.tensor(t not in window, device=dev)) & (c < T)
        a = acts[c.clamp(max=T - 1), lanes]
        frames, r, d, i = env.step_where(a, m)
        want = tf[c.clamp(max=T - 1), lanes]
        if prev is not None:
            want = torch.where(m.view(-1, *([1] * (frames.dim() - 1))), want, prev)
        assert torch.equal(frames, want), (t, (frames != want).flatten(1).any(1).nonzero()[:5, 0].tolist())
        assert torch.equal(frames, env.render(obs_type)), t  # ... and they are the frames of the state
        c += m.long()
        prev = frames.clone()
    assert bool((c == T).all())
    assert _bytes(env.save_lanes().rows) == _bytes(twin.save_lanes().rows)
    for e in envs:
        e.close()


# ---------------------------------------------------------------------------------------------------------------
# 8. a captured graph
def test_captured_masked_steps_equal_the_eager_ones(sfa):
    n, K = 200, 3
    res = []
    for captured in (False, True):
        (env, other), rng = _twin_envs(sfa, n, seed=12)
        other.close()
        dev = env.device
        env.set_field("time", (180000 - 34 * (3 + np.arange(n) % 9)).astype(np.int32))  # finishes spread over the replays
        a = torch.from_numpy(_busy_actions(rng, env.n_actions, (K, n))).to(dev)
        m = torch.from_numpy(rng.random((K, n)) < 0.5).to(dev)
        outs = [_outs(env) for _ in range(K)]
        env.step_where(a[0], m[0])  # eager first: the stash is made here, and the edited field is folded in
        torch.cuda.synchronize()
        mid = []
        if captured:
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                with torch.cuda.graph(g, stream=side):  # one stream, no parallel branches
                    for k in range(K):
                        env.step_where(a[k], m[k], out=outs[k][:4], ticks_out=outs[k][4])
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize()
            assert all(TR.untouched(*o) for o in outs)  # (a capture runs nothing)
            for rep in range(2):
                g.replay()
                torch.cuda.synchronize()
                mid.append([[_bytes(x) for x in o] for o in outs])
            del g
        else:
            for rep in range(2):
                for k in range(K):
                    env.step_where(a[k], m[k], out=outs[k][:4], ticks_out=outs[k][4])
                torch.cuda.synchronize()
                mid.append([[_bytes(x) for x in o] for o in outs])
        for o in outs:
            TR.margins_intact(*o)
        res.append((mid, _bytes(env.save_lanes().rows), env.episode_stats().tolist()))
        env.close()
    assert res[0] == res[1]
    assert res[0][2][0] > 0  # games ended inside the replays


# ---------------------------------------------------------------------------------------------------------------
# 9. refusals
def test_refusals_leave_the_batch_as_it_was(sfa):
    from spacefortress_amd import _lib

    L = _lib.lib()
    n = 65
    env = sfa.SFVecEnv(n)
    env.reset()
    dev = env.device
    a = torch.ones(n, dtype=torch.uint8, device=dev)
    m = torch.ones(n, dtype=torch.uint8, device=dev)
    env.step_tensors(a)
    before = _bytes(env.save_lanes().rows)
    outs = _outs(env)
    p = lambda t: C.c_void_p(t.data_ptr())
    args = lambda e: [e._h, p(m), p(a), 1, 1, p(outs[0]), p(outs[1]), p(outs[2]), p(outs[3]), p(outs[4]), e._stream()]
    for i, v in ((0, None), (1, None), (2, None), (3, 0), (3, 2), (3, 3), (4, 0), (4, 256), (4, -1)):
        b = args(env)
        b[i] = v
        assert L.sf_step_where(*b) == _lib.SF_ERR_ARG, (i, v)
        assert "sf_step_where" in _lib.last_error()
    for bad in (m[:-1], m.to(torch.int32), m.cpu(), torch.ones(2 * n, dtype=torch.uint8, device=dev)[::2], m.view(1, n), None):
        with pytest.raises(ValueError, match=r"active must be a contiguous uint8 or bool tensor \[%d\] on " % n):
            env.step_where(a, bad)
    for rep in (0, 256):  # (the C text reaches Python as it is)
        env.frame_skip = rep
        with pytest.raises(ValueError, match=r"sf_step_where: repeat must be in \[1, 255\]"):
            env.step_where(a, m)
    env.frame_skip = 1
    torch.cuda.synchronize()
    assert TR.untouched(*outs) and _bytes(env.save_lanes().rows) == before
    env.close()
    # the logs that count rows, each on a batch of its own
    for enable, text in ((lambda e: e.enable_durations(), "duration log is enabled.*counts rows, not the ticks"),
                         (lambda e: e.enable_episode_log(capacity=64), "episode log is enabled.*counts rows, not the ticks")):
        env = sfa.SFVecEnv(n)
        env.reset()
        before = _bytes(env.save_lanes().rows)
        enable(env)
        with pytest.raises(ValueError, match=text):
            env.step_where(a, m, out=outs[:4], ticks_out=outs[4])
        torch.cuda.synchronize()
        assert TR.untouched(*outs) and _bytes(env.save_lanes().rows) == before
        env.close()
    # a recording
    env = sfa.SFVecEnv(n)
    env.start_recording()
    with pytest.raises(ValueError, match="during a recording: a replay file holds one action per env and step"):
        env.step_where(a, m)
    assert env._rec is not None  # (the recording goes on)
    env.close()
    # a batch without auto-reset: repeat 1 only
    env = sfa.SFVecEnv(n, auto_reset=False)
    env.reset()
    before = _bytes(env.save_lanes().rows)
    b = args(env)
    b[4] = 2
    assert L.sf_step_where(*b) == _lib.SF_ERR_ARG and "SF_FLAG_NO_AUTO_RESET" in _lib.last_error()
    torch.cuda.synchronize()
    assert TR.untouched(*outs) and _bytes(env.save_lanes().rows) == before
    b[4] = 1
    assert L.sf_step_where(*b) == 0
    torch.cuda.synchronize()
    assert bool((outs[4] == 1).all())
    env.close()
