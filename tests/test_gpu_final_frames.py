"""Final frames of image batches (include/sfmi_final.h: sf_set_final_frame_output, sf_final_stack_shift;
SFVecEnv.enable_final_frames; DeviceRollout / FrameRollout(time_limit_bootstrap=True) on image envs).

Three batches with the same seed, the same preparation and the same actions:
  A  auto-reset, final frames on, the buffer pre-filled with a sentinel inside guard margins;
  B  auto_reset=False: after a tick on which an env finishes, the frame sf_render draws of it IS that game's last frame -- drawn
     by the frame kernel of the batch's geometry, not by the painter the final frames come from; then reset_lanes(mask=done);
  C  auto-reset, output off: what every other byte of A must equal.
C runs first (its sampled actions are what the others play), then B (the expected buffer after every tick), then A.

1. sf_step at 1, 65 and 130 envs, and 1 024 envs that all finish on one tick;  2. image-raw and another geometry;  3. the other
entry points and a captured graph;  4. sf_final_stack_shift against the model;  5. both rollouts;  6. refusals, and off is off.
Everything is compared byte for byte.
"""
import ctypes as C

import numpy as np
import pytest

import finalframes_np as FF
import timelimit_np as TL
import trainerref as TR
from lockstep import sfa

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GAME_MS, TICK_MS = 180000, 34
NEVER = 0  # ticks to the finish: an env that plays on
GEOMETRY = (0.23, (130, 80, 450, 460), 3)  # a 103 x 105 surface: an odd number of bytes, raw frames at odd addresses
SEED = 20261021


def _schedule(n, T):
    """ticks to the finish per env (NEVER: it plays on): staggered over T ticks, every fifth env plays on; every env of the tile
    64 .. 127 on tick 9; the partial last tile's envs finish (130: on different ticks).  n = 1: tick 5."""
    k = 1 + (7 * np.arange(n)) % (T - 2)
    k[4::5] = NEVER
    if n >= 128:
        k[64:128] = 9
    if n % 64:
        k[n - 1] = 3
    if n % 64 > 1:
        k[n - 2] = 20
    if n == 1:
        k[:] = 5
    return k


def _prepare(env, warm, k):
    """reset, `warm` ticks of fire / thrust / turn, then the states the finishes should show -- a few destroyed fortresses, ships
    mid-explosion and scores, through set_field -- and the clocks."""
    n, dev = env.num_envs, env.device
    env.reset()
    rng = np.random.default_rng(SEED)
    wa = torch.from_numpy(rng.integers(0, env.n_actions, (warm, n)).astype(np.uint8)).to(dev)
    for t in range(warm):
        env.step_tensors(wa[t])
    flags, sdt, fdt, pts, time = (env.get_field(f) for f in ("flags", "ship_death_timer", "fort_death_timer", "points", "time"))
    soon = np.flatnonzero((k > 0) & (k < 25))  # (both explosions last 1 000 ms: 29 ticks)
    for j, e in enumerate(soon[:12]):
        if j % 3 == 0:
            flags[e] &= ~np.uint8(2)  # the fortress is destroyed
            fdt[e] = 0
        elif j % 3 == 1:
            flags[e] &= ~np.uint8(1)  # the ship explodes
            sdt[e] = 0
        else:
            pts[e] = (-1) ** j * (37 * j + 5)
    time = np.where(k > 0, GAME_MS - TICK_MS * k, time).astype(np.int32)
    for f, v in (("flags", flags), ("ship_death_timer", sdt), ("fort_death_timer", fdt), ("points", pts), ("time", time)):
        env.set_field(f, v)
    env.seed_actions(SEED)


def _make(sfa, n, obs_type, geometry, **kw):
    return sfa.SFVecEnv(n, gametype="youturn", obs_type=obs_type, seed=7, image_geometry=geometry, **kw)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _np(t):
    return t.cpu().numpy()


PER_TICK = ("sf_step", "sf_step_sampled", "sf_step_record", "graph")


def _drive(env, entry, acts, T, on_tick=None):
    """T ticks of `env` through `entry`.  Returns dict(obs [T, n, ...], rew, done, info, events [T, n], acts (what was played),
    extra (the float outputs of sf_step_record), rows (the save_lanes rows after every tick, or after the call)).
    on_tick(t): called behind every tick of a per-tick entry, synchronised."""
    from spacefortress_amd import _lib

    L, n, dev = _lib.lib(), env.num_envs, env.device
    env.enable_events()
    out = dict(extra=None)
    # (a tensor per tick: row t of one [T, n, 92, 90] tensor would not start 16-byte aligned, which raw frames must)
    obs = [torch.empty((n,) + tuple(env.obs_shape), dtype=torch.uint8, device=dev) for _ in range(T)]
    rew = torch.empty((T, n), dtype=torch.int32, device=dev)
    done, info = (torch.empty((T, n), dtype=torch.uint8, device=dev) for _ in range(2))
    ev = torch.zeros((T, n), dtype=torch.int32, device=dev)
    played = torch.zeros((T, n), dtype=torch.uint8, device=dev)
    rows = []
    if entry in PER_TICK:
        if entry == "sf_step_record":
            rf, mk, ep, fin = (torch.zeros(n, dtype=torch.float32, device=dev) for _ in range(4))
            ao = torch.zeros(n, dtype=torch.int64, device=dev)
            hist = torch.zeros((T, 4, n), dtype=torch.float32, device=dev)
        graph = None
        if entry == "graph":
            a_cur = torch.zeros(n, dtype=torch.uint8, device=dev)
            o1 = (torch.empty_like(obs[0]), torch.empty_like(rew[0]), torch.empty_like(done[0]), torch.empty_like(info[0]))
            a_cur.copy_(acts[0])
            env.step_tensors(a_cur, out=o1)  # eager: the launch that folds the edited state back belongs in front of the graph
            first = [x.clone() for x in o1] + [env.events.clone()]
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                with torch.cuda.graph(graph, stream=side):  # one stream, no parallel branches
                    env.step_tensors(a_cur, out=o1)
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize()
        for t in range(T):
            if entry == "sf_step":
                env.step_tensors(acts[t], out=(obs[t], rew[t], done[t], info[t]))
                played[t].copy_(acts[t])
            elif entry == "sf_step_sampled":
                env.step_sampled(out=(obs[t], rew[t], done[t], info[t]), actions_out=played[t])
            elif entry == "sf_step_record":
                assert L.sf_step_record(env._h, _p(acts[t]), 1, _p(obs[t]), _p(rew[t]), _p(done[t]), _p(info[t]), _p(rf), _p(mk), _p(ep),
                                        _p(fin), _p(ao), env._stream()) == 0, _lib.last_error()
                hist[t].copy_(torch.stack((rf, mk, ep, fin)))
                played[t].copy_(ao.to(torch.uint8))
            else:
                if t == 0:
                    res = first
                else:
                    a_cur.copy_(acts[t])
                    graph.replay()
                    res = list(o1) + [env.events]
                for dst, src in zip((obs[t], rew[t], done[t], info[t]), res):
                    dst.copy_(src)
                ev[t].copy_(res[4])
                played[t].copy_(acts[t])
            if entry != "graph":
                ev[t].copy_(env.events)
            torch.cuda.synchronize()
            rows.append(_np(env.save_lanes().rows))
            if on_tick is not None:
                on_tick(t)
        if entry == "sf_step_record":
            out["extra"] = _np(hist)
        del graph
        obs = torch.stack(obs)
    else:
        want_obs = not entry.endswith("_noobs")
        if entry.startswith("sf_rollout_sampled"):
            o, r, d, i, a = env.rollout_sampled(T, want_obs=want_obs)
        else:
            o, r, d, i = env.rollout(acts, want_obs=want_obs)
            a = acts
        torch.cuda.synchronize()
        obs = o if want_obs else None
        rew, done, info, played, ev = r, d, i, a, env.rollout_events
        rows.append(_np(env.save_lanes().rows))
    out.update(obs=_np(obs) if obs is not None else None, rew=_np(rew), done=_np(done), info=_np(info), events=_np(ev), acts=_np(played),
               rows=rows)
    return out


def _expected_buffers(envB, acts, T, mode, sentinel):
    """B, tick by tick on `acts` [T, n]: the final buffer A should hold after every tick, [T, n, ...]; the done flags; and what the
    finishing states showed."""
    n, dev = envB.num_envs, envB.device
    a = torch.from_numpy(np.ascontiguousarray(acts)).to(dev)
    buf = np.full((n,) + tuple(envB.obs_shape), sentinel, np.uint8)
    exp, dones = [], []
    seen = dict(missile=0, shell=0, ship_exploding=0, fort_destroyed=0, points=0, finishes=0)
    for t in range(T):
        _, _, done, _ = envB.step_tensors(a[t])
        frames = _np(envB.render(mode))
        d = _np(done) != 0
        if d.any():
            buf[d] = frames[d]
            fl, mm, sm, pt = (envB.get_field(f) for f in ("flags", "missile_mask", "shell_mask", "points"))
            seen["missile"] += int((mm[d] != 0).sum())
            seen["shell"] += int((sm[d] != 0).sum())
            seen["ship_exploding"] += int(((fl[d] & 1) == 0).sum())
            seen["fort_destroyed"] += int(((fl[d] & 2) == 0).sum())
            seen["points"] += int((pt[d] != 0).sum())
            seen["finishes"] += int(d.sum())
            envB.reset_lanes(mask=done)
        exp.append(buf.copy())
        dones.append(d)
    return np.stack(exp), np.stack(dones), seen


def _case(sfa, n, T, warm, entry="sf_step", obs_type="image", geometry=None, k=None, coverage=False):
    k = _schedule(n, T) if k is None else k
    sampled = "sampled" in entry
    rng = np.random.default_rng(SEED + 1)
    given = rng.integers(0, 5, (T, n)).astype(np.uint8)
    # C: the same calls with the output off
    envC = _make(sfa, n, obs_type, geometry)
    dev = envC.device
    _prepare(envC, warm, k)
    acts_dev = torch.from_numpy(given).to(dev)
    c = _drive(envC, entry, acts_dev, T)
    statsC = envC.episode_stats()
    envC.close()
    acts = c["acts"] if sampled else given
    # B: the finished games' frames from the frame kernel of the geometry
    envB = _make(sfa, n, obs_type, geometry, auto_reset=False)
    _prepare(envB, warm, k)
    exp, donesB, seen = _expected_buffers(envB, acts, T, obs_type, TR.SENTINEL_BYTE)
    envB.close()
    assert np.array_equal(donesB, c["done"] != 0)
    assert seen["finishes"] == int((k > 0).sum()) > 0
    if coverage:
        assert all(seen[w] > 0 for w in ("missile", "shell", "ship_exploding", "fort_destroyed", "points")), seen
    # A
    envA = _make(sfa, n, obs_type, geometry)
    fin = TR.guarded((n,) + tuple(envA.obs_shape), torch.uint8, dev)
    assert envA.enable_final_frames(out=fin) is fin and envA.final_frames is fin
    _prepare(envA, warm, k)
    torch.cuda.synchronize()
    assert TR.untouched(fin), "a row was written before any env finished"

    def on_tick(t):
        got = _np(fin)
        bad = np.argwhere(got != exp[t])
        assert bad.size == 0, (entry, t, "final buffer: env %d (finished now: %s), %d bytes differ" % (bad[0][0], bool(donesB[t][bad[0][0]]), len(bad)))

    a = _drive(envA, entry, acts_dev, T, on_tick)
    torch.cuda.synchronize()
    TR.margins_intact(fin)
    assert np.array_equal(_np(fin), exp[-1]), (entry, "final buffer after the last tick")
    for key in ("obs", "rew", "done", "info", "events", "acts", "extra"):
        if c[key] is None:
            assert a[key] is None
            continue
        assert a[key].tobytes() == c[key].tobytes(), (entry, key, np.argwhere(a[key] != c[key])[:4])
    assert len(a["rows"]) == len(c["rows"])
    for t, (ra, rc) in enumerate(zip(a["rows"], c["rows"])):
        assert np.array_equal(ra, rc), (entry, "lane rows", t, np.flatnonzero((ra != rc).any(1))[:8])
    statsA = envA.episode_stats()
    assert np.array_equal(statsA, statsC) and statsA[0] == seen["finishes"], (statsA, statsC)
    envA.check_state()
    envA.close()
    assert envA.final_frames is None


# ---------------------------------------------------------------------------------------------------------------
# 1. sf_step
@pytest.mark.parametrize("n", [1, 65, 130])
def test_final_frames_are_the_finished_games_last_frames(sfa, n):
    _case(sfa, n, T=12 if n == 1 else 42, warm=60 if n == 1 else 130, coverage=n > 1)


def test_a_thousand_envs_finish_on_one_tick(sfa):
    n = 1024
    _case(sfa, n, T=4, warm=60, k=np.full(n, 2))


# ---------------------------------------------------------------------------------------------------------------
# 2. the raw surface, another geometry
@pytest.mark.parametrize("obs_type,geometry", [("image-raw", None), ("image", GEOMETRY), ("image-raw", GEOMETRY)],
                         ids=["raw", "geometry", "raw-geometry"])
def test_final_frames_in_every_mode_and_geometry(sfa, obs_type, geometry):
    _case(sfa, 65, T=30, warm=100, obs_type=obs_type, geometry=geometry)


# ---------------------------------------------------------------------------------------------------------------
# 3. the other entry points, a captured graph
@pytest.mark.parametrize("entry", ["sf_step_sampled", "sf_step_record", "sf_rollout", "sf_rollout_noobs", "sf_rollout_sampled",
                                   "sf_rollout_sampled_noobs", "graph"])
def test_every_entry_point_writes_the_same_final_frames(sfa, entry):
    _case(sfa, 65, T=30, warm=80, entry=entry)


# ---------------------------------------------------------------------------------------------------------------
# 4. sf_final_stack_shift
@pytest.mark.parametrize("n", [1, 63, 65])
def test_final_stack_shift_equals_the_model(sfa, n):
    from spacefortress_amd import _lib

    L, dev = _lib.lib(), torch.device("cuda")
    rng = np.random.default_rng(n)
    for S in range(1, 17):
        fb = 7056 if S == 4 else 48
        prev_h = rng.integers(0, 256, (n, S, fb)).astype(np.uint8)
        done_h = rng.choice(np.array([0, 0, 1, 2, 128, 255], np.uint8), n)
        if n > 1:
            done_h[0], done_h[-1] = 0, 255
        prev = TR.guarded((n, S, fb), torch.uint8, dev, prev_h)
        fin = TR.guarded((n, S, fb), torch.uint8, dev)
        done = torch.from_numpy(done_h).to(dev)
        assert L.sf_final_stack_shift(_p(prev), _p(fin), S, fb, _p(done), n, None) == 0, _lib.last_error()
        torch.cuda.synchronize()
        want = FF.shift(prev_h, np.full((n, S, fb), TR.SENTINEL_BYTE, np.uint8), done_h)
        assert np.array_equal(_np(fin), want), (n, S)
        assert np.array_equal(_np(prev), prev_h)
        TR.margins_intact(prev, fin)


def test_final_stack_shift_refusals(sfa):
    from spacefortress_amd import _lib

    L, dev = _lib.lib(), torch.device("cuda")
    n, S, fb = 5, 4, 48
    both = TR.guarded((2 * n * S * fb + 64,), torch.uint8, dev)
    prev, fin = both[:n * S * fb], both[n * S * fb:2 * n * S * fb]
    done = torch.ones(n, dtype=torch.uint8, device=dev)
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    bad = [(vp(prev), vp(fin), 0, fb), (vp(prev), vp(fin), 17, fb), (vp(prev), vp(fin), S, 40), (vp(prev), vp(fin), S, 0),
           (vp(prev, 8), vp(fin), S, fb), (vp(prev), vp(fin, 8), S, fb), (None, vp(fin), S, fb), (vp(prev), None, S, fb),
           (vp(prev), vp(prev), S, fb), (vp(prev), vp(prev, 16 * 7), S, fb), (vp(prev, 16 * 3), vp(prev), S, fb)]
    for pa, fa, s, b in bad:
        assert L.sf_final_stack_shift(pa, fa, s, b, _p(done), n, None) == _lib.SF_ERR_ARG, (s, b)
        assert "sf_final_stack_shift" in _lib.last_error()
    assert L.sf_final_stack_shift(vp(prev), vp(fin), S, fb, None, n, None) == _lib.SF_ERR_ARG
    assert L.sf_final_stack_shift(vp(prev), vp(fin), S, fb, _p(done), 0, None) == _lib.SF_ERR_ARG
    torch.cuda.synchronize()
    assert TR.untouched(both)  # nothing was launched
    assert L.sf_final_stack_shift(vp(prev), vp(fin), S, fb, _p(done), n, None) == 0  # the two ranges may touch
    torch.cuda.synchronize()
    TR.margins_intact(both)


# ---------------------------------------------------------------------------------------------------------------
# 5. both rollouts
def test_rollouts_bootstrap_with_the_final_stack(sfa):
    n, T, S = 65, 24, 4
    k = 1 + (5 * np.arange(n)) % (T - 1)
    k[3::4] = NEVER
    k[0] = 1       # a finish in the first step after the reset: zero history
    k[7] = 2
    again = (3, 7, 2)  # behind step 3, env 7's clock is set again: its second finish, in step 5, is inside the stack of the first
    rng = np.random.default_rng(SEED + 2)
    acts = rng.integers(0, 5, (T, n)).astype(np.uint8)

    def clocks(env, k):
        time = env.get_field("time")
        env.set_field("time", np.where(k > 0, GAME_MS - TICK_MS * k, time).astype(np.int32))

    def second(env):
        k2 = np.zeros(n, np.int64)
        k2[again[1]] = again[2]
        clocks(env, k2)

    # B: the model's frames
    envB = _make(sfa, n, "image", None, auto_reset=False)
    a = torch.from_numpy(acts).to(envB.device)
    model = FF.FinalStackModel(n, S, (84, 84), np.uint8, 0)
    envB.reset()
    model.reset(_np(envB.render("image"))[:, 0])
    clocks(envB, k)
    dones = np.zeros((T, n), bool)
    for t in range(T):
        _, _, done, _ = envB.step_tensors(a[t])
        last = _np(envB.render("image"))[:, 0]
        dones[t] = _np(done) != 0
        if dones[t].any():
            envB.reset_lanes(mask=done)
        model.step(dones[t], last, _np(envB.render("image"))[:, 0])
        if t + 1 == again[0]:
            second(envB)
    envB.close()
    assert dones[:, again[1]].sum() == 2 and dones[0, 0] and dones.any(0).sum() == (k > 0).sum()

    res = {}
    g = torch.Generator().manual_seed(11)
    values, nv, fv = torch.randn(T, n, 1, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g)
    for name in ("DeviceRollout", "FrameRollout"):
        env = _make(sfa, n, "image", None)
        dev = env.device
        ro = getattr(sfa, name)(env, T, num_stack=S, time_limit_bootstrap=True)
        assert env.final_frames is not None and tuple(ro.final_obs().shape) == (n, S, 84, 84)
        ro.reset()
        clocks(env, k)
        ad = torch.from_numpy(acts).to(dev)
        cur = []
        for t in range(T):
            o, _, _ = ro.step(t, ad[t], value_pred=values[t].to(dev))
            if t + 1 == again[0]:
                second(env)
            if t in (0, 5, T - 1):
                cur.append(_np(o).copy())
        with pytest.raises(ValueError):
            ro.compute_returns(nv.to(dev), True, 0.99, 0.95)  # no silent fall-back
        fo = _np(ro.final_obs())
        assert np.array_equal(fo, model.final), (name, np.flatnonzero((fo != model.final).reshape(n, -1).any(1))[:8])
        assert np.array_equal(cur[-1], model.cur), name
        rets = []
        for gae in (True, False):
            ro.compute_returns(nv.to(dev), gae, 0.99, 0.95, final_value=fv.to(dev))
            torch.cuda.synchronize()
            rew, vp, masks = (_np(x[:, :, 0]) for x in (ro.rewards, ro.value_preds, ro.masks))
            assert np.array_equal(masks[1:] == 0, dones)
            want, _ = TL.compute_returns_tl(rew, vp.copy(), masks, nv.numpy(), fv.numpy(), gae, 0.99, 0.95)
            rows = slice(0, T) if gae else slice(0, T + 1)
            got = _np(ro.returns[:, :, 0])
            TR.assert_bits_equal(got[rows], want[rows], "%s returns, gae=%s" % (name, gae))
            rets.append(got[rows].copy())
        res[name] = (fo, cur, rets, _np(ro.rewards), _np(ro.masks))
        env.close()
    d, f = res["DeviceRollout"], res["FrameRollout"]
    assert np.array_equal(d[0], f[0]) and all(np.array_equal(x, y) for x, y in zip(d[1], f[1]))
    assert all(x.tobytes() == y.tobytes() for x, y in zip(d[2], f[2])) and np.array_equal(d[3], f[3]) and np.array_equal(d[4], f[4])


def test_a_rollout_without_a_stack_bootstraps_with_the_final_frame(sfa):
    """S = 1: nothing is shifted; the final frame alone is the final observation."""
    n, T = 65, 6
    k = np.where(np.arange(n) % 2 == 0, 1 + np.arange(n) % 5, NEVER)
    acts = np.random.default_rng(3).integers(0, 5, (T, n)).astype(np.uint8)
    envB = _make(sfa, n, "image", None, auto_reset=False)
    envB.reset()
    envB.set_field("time", np.where(k > 0, GAME_MS - TICK_MS * k, 0).astype(np.int32))
    want = np.zeros((n, 1, 84, 84), np.uint8)
    a = torch.from_numpy(acts).to(envB.device)
    for t in range(T):
        _, _, done, _ = envB.step_tensors(a[t])
        d = _np(done) != 0
        want[d] = _np(envB.render("image"))[d]
        envB.reset_lanes(mask=done)
    envB.close()
    for name in ("DeviceRollout", "FrameRollout"):
        env = _make(sfa, n, "image", None)
        ro = getattr(sfa, name)(env, T, num_stack=1, time_limit_bootstrap=True)
        ro.reset()
        env.set_field("time", np.where(k > 0, GAME_MS - TICK_MS * k, 0).astype(np.int32))
        ad = torch.from_numpy(acts).to(env.device)
        for t in range(T):
            ro.step(t, ad[t])
        assert np.array_equal(_np(ro.final_obs()), want), name
        env.close()


# ---------------------------------------------------------------------------------------------------------------
# 6. refusals; off is off
def _steps(env):
    env.reset()
    env.step_tensors(torch.zeros(env.num_envs, dtype=torch.uint8, device=env.device))
    torch.cuda.synchronize()


def test_refusals_leave_the_batch_stepping(sfa):
    from spacefortress_amd import _lib

    L, n = _lib.lib(), 65
    # the C call: no image observations, no auto-reset
    for kw, word in ((dict(obs_type="features"), "image"), (dict(obs_type="image", auto_reset=False), "SF_FLAG_NO_AUTO_RESET")):
        env = sfa.SFVecEnv(n, **kw)
        buf = TR.guarded((n, 1, 84, 84), torch.uint8, env.device)
        assert L.sf_set_final_frame_output(env._h, _p(buf), 0) == _lib.SF_ERR_ARG
        assert "sf_set_final_frame_output" in _lib.last_error() and word in _lib.last_error()
        with pytest.raises(ValueError):
            env.enable_final_frames()
        with pytest.raises(ValueError):
            env.enable_final_frames(out=buf)
        assert env.final_frames is None
        assert L.sf_set_final_frame_output(env._h, None, 0) == 0  # (off is always possible)
        env.set_field("time", np.full(n, GAME_MS - TICK_MS, np.int32)) if kw["obs_type"] == "image" else None
        _steps(env)
        assert TR.untouched(buf)
        env.close()
    # alignment and stride: sf_render's rules for the mode and geometry
    frame = 84 * 84
    env = sfa.SFVecEnv(n, obs_type="image")
    big = TR.guarded((n * frame + 64,), torch.uint8, env.device)
    for off, stride in ((4, 0), (8, 0), (1, 0), (0, frame - 16), (0, frame + 8), (0, 16)):
        assert L.sf_set_final_frame_output(env._h, C.c_void_p(big.data_ptr() + off), stride) == _lib.SF_ERR_ARG, (off, stride)
    with pytest.raises(ValueError):
        env.enable_final_frames(out=big[4:4 + n * frame].view(n, 1, 84, 84))
    with pytest.raises(ValueError):
        env.enable_final_frames(out=torch.zeros((n, 84, 84), dtype=torch.uint8, device=env.device))
    with pytest.raises(ValueError):
        env.enable_final_frames(out=torch.zeros((n, 1, 84, 84), dtype=torch.float32, device=env.device))
    with pytest.raises(ValueError):
        env.enable_final_obs()  # (image batches still have no final-observation ROWS)
    assert env.final_frames is None
    env.reset()
    env.set_field("time", np.full(n, GAME_MS - TICK_MS, np.int32))  # every env finishes on the next tick: nothing may be written
    env.step_tensors(torch.zeros(n, dtype=torch.uint8, device=env.device))
    torch.cuda.synchronize()
    assert TR.untouched(big)
    env.close()
    for obs_type, offs in (("image", ((1, False), (2, False), (4, True))), ("image-raw", ((1, True), (3, True)))):
        env = sfa.SFVecEnv(n, obs_type=obs_type, image_geometry=GEOMETRY)
        fb = 84 * 84 if obs_type == "image" else env.image_w * env.image_h
        big = torch.zeros(n * fb + 64, dtype=torch.uint8, device=env.device)
        for off, ok in offs:
            assert (L.sf_set_final_frame_output(env._h, C.c_void_p(big.data_ptr() + off), 0) == 0) == ok, (obs_type, off)
        assert L.sf_set_final_frame_output(env._h, _p(big), fb - 1) == _lib.SF_ERR_ARG
        assert L.sf_set_final_frame_output(env._h, None, 0) == 0
        _steps(env)
        env.close()
    # frame_skip > 1, the action repeat and the masked step
    env = sfa.SFVecEnv(n, obs_type="image", frame_skip=2)
    with pytest.raises(ValueError):
        env.enable_final_frames()
    assert env.final_frames is None
    env.reset()
    env.step_tensors(torch.zeros(n, dtype=torch.uint8, device=env.device))
    env.close()
    env = sfa.SFVecEnv(n, obs_type="image")
    fin = TR.guarded((n, 1, 84, 84), torch.uint8, env.device)
    env.enable_final_frames(out=fin)
    env.reset()
    state = env.save_lanes().rows.clone()
    a = torch.zeros(n, dtype=torch.uint8, device=env.device)
    outs = (TR.guarded((n, 1, 84, 84), torch.uint8, env.device), TR.guarded((n,), torch.int32, env.device),
            TR.guarded((n,), torch.uint8, env.device), TR.guarded((n,), torch.uint8, env.device))
    with pytest.raises(ValueError):
        env.step_repeat(a, 2, out=outs)
    with pytest.raises(ValueError):
        env.step_where(a, torch.ones(n, dtype=torch.uint8, device=env.device), out=outs)
    ptrs = [_p(x) for x in outs]
    assert L.sf_step_repeat(env._h, _p(a), 1, 2, *ptrs, None, env._stream()) == _lib.SF_ERR_ARG
    assert "follow-up" in _lib.last_error()
    assert L.sf_step_where(env._h, _p(torch.ones_like(a)), _p(a), 1, 1, *ptrs, None, env._stream()) == _lib.SF_ERR_ARG
    assert "follow-up" in _lib.last_error()
    torch.cuda.synchronize()
    assert TR.untouched(*outs) and TR.untouched(fin) and torch.equal(env.save_lanes().rows, state)  # nothing was launched
    env.step_repeat(a, 1, out=outs)  # repeat 1 is sf_step
    torch.cuda.synchronize()
    assert not TR.untouched(outs[0])
    env.close()
    # the rollouts
    env = sfa.SFVecEnv(n, obs_type="image", auto_reset=False)
    for make in (lambda: sfa.DeviceRollout(env, 4, num_stack=4, time_limit_bootstrap=True),
                 lambda: sfa.DeviceRollout(env, 4, time_limit_bootstrap=True),
                 lambda: sfa.FrameRollout(env, 4, time_limit_bootstrap=True)):
        with pytest.raises(ValueError):
            make()
    _steps(env)
    env.close()
    env = sfa.SFVecEnv(n, obs_type="image")
    for make in (lambda: sfa.DeviceRollout(env, env.max_ticks + 2, num_stack=4, time_limit_bootstrap=True),
                 lambda: sfa.FrameRollout(env, env.max_ticks + 2, time_limit_bootstrap=True)):
        with pytest.raises(ValueError):
            make()
    assert env.final_frames is None
    env.close()
    env = sfa.SFVecEnv(n, obs_type="image", image_geometry=GEOMETRY)
    with pytest.raises(ValueError):
        sfa.FrameRollout(env, 4, time_limit_bootstrap=True)
    assert env.final_frames is None
    _steps(env)
    env.close()


def test_off_is_off(sfa):
    """enable_final_frames(False) restores the plain path: the buffer stays as it is and every byte equals the twin's that never
    had the output."""
    n, T = 65, 6
    k = np.full(n, 3)
    acts = torch.from_numpy(np.random.default_rng(9).integers(0, 5, (T, n)).astype(np.uint8))
    res = []
    for on_then_off in (True, False):
        env = _make(sfa, n, "image", None)
        fin = TR.guarded((n, 1, 84, 84), torch.uint8, env.device)
        if on_then_off:
            env.enable_final_frames(out=fin)
        _prepare(env, 20, k)
        if on_then_off:
            assert env.enable_final_frames(False) is None and env.final_frames is None
        a = acts.to(env.device)
        outs = [env.step_tensors(a[t]) for t in range(T)]
        torch.cuda.synchronize()
        assert TR.untouched(fin)
        res.append(([tuple(_np(x).tobytes() for x in o) for o in outs], _np(env.save_lanes().rows), env.episode_stats()))
        assert res[-1][2][0] == n
        env.close()
    assert res[0][0] == res[1][0] and np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])
