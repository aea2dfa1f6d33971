"""The masked reset (include/sfmi.h: sf_reset_lanes, sfmi_masked.h: sf_eplog_restart_where; SFVecEnv.reset_lanes): env.reset() in the lanes the
caller chooses (ENV:163-178) while every other lane plays on, bit for bit -- against twin batches (one fully reset, one left
alone), against the CPU oracle, against the step kernel's own auto-reset, for feature and image batches.

Everything is compared bit for bit.  A batch is brought to a state worth resetting with seeded random actions that fire half
of the time: the tiles' missile pools then span three and more rows of 64 entries (asserted from get_field where the batch
has the lanes for it: a tile of fewer than seven lanes cannot hold 129 missiles)."""

import numpy as np
import pytest

from eplogref import EpisodeLogModel
from sfcompare import compare_state, obs_close
from sfscript import firing_actions as _actions, largest_pool as _largest_pool
from lockstep import sfa

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SIZES = [1, 63, 64, 65, 129, 4161]
MASKS = ["none", "all", "one", "ends", "per_tile", "tile", "alternating", "half", "bytes"]
WARM = 400


def _make(sfa, n, gametype="youturn", **kw):
    return sfa.SFVecEnv(n, gametype=gametype, action_set=1, spawn_stride=1, **kw)


def _warm(envs, T, seed):
    e0 = envs[0]
    a = torch.from_numpy(_actions(T, e0.num_envs, e0.n_actions, seed)).to(e0.device)
    for e in envs:
        e.rollout(a, want_obs=False)


def _worth_resetting(env):
    pool = _largest_pool(env)
    shells = int((env.get_field("shell_mask") != 0).sum())
    print("largest pool %d entries, lanes with shells %d (%s, %d envs)" % (pool, shells, env.gametype, env.num_envs))
    if env.gametype == "youturn" and env.num_envs >= 63:
        assert pool > 128, "the largest pool holds %d entries: fewer than three rows" % pool
        assert shells > 0
    elif env.num_envs >= 63:  # (the other presets: whatever their play leaves, but something; a lone env may hold none)
        assert pool > 0
    return pool


def _mask(kind, n, rng):
    m = np.zeros(n, np.uint8)
    if kind == "all":
        m[:] = 1
    elif kind == "one":
        m[n // 2] = 1
    elif kind == "ends":
        m[0] = m[-1] = 1
    elif kind == "per_tile":
        for t in range((n + 63) // 64):
            m[min(n - 1, 64 * t + (7 * t + 3) % 64)] = 1
    elif kind == "tile":
        t = 1 if n >= 128 else 0
        m[64 * t:64 * t + 64] = 1
    elif kind == "alternating":
        m[::2] = 1
    elif kind == "half":
        m[rng.random(n) < 0.5] = 1
    elif kind == "bytes":
        sel = rng.random(n) < 0.5
        m[sel] = np.resize(np.array([2, 255, 1], np.uint8), int(sel.sum()))
    return m


def _bits(t):
    if not t.is_floating_point():
        return t
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32)


def _sentinel(env):
    shape = (env.num_envs,) + tuple(env.obs_shape)
    if env.obs_dtype == torch.uint8:
        return torch.randint(0, 256, shape, dtype=torch.uint8, device=env.device)
    return torch.rand(shape, dtype=env.obs_dtype, device=env.device) + 1000.0


def _same_dict(a, b):
    return [f for f in a if np.ascontiguousarray(a[f]).tobytes() != np.ascontiguousarray(b[f]).tobytes()]


def _row_diff(x, y):
    """[n] bool on the device: the lanes whose outputs differ in any bit"""
    d = _bits(x) != _bits(y)
    return d.reshape(d.shape[0], -1).any(1)


# ---------------------------------------------------------------------------------------------- 1. twin batches
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("gametype,n", [("youturn", s) for s in SIZES] + [("autoturn", 129), ("test-youturn", 129)])
def test_twin_batches(sfa, gametype, n, kind):
    """A.reset_lanes(mask), B.reset(), C untouched, from equal states: A's masked lanes are B's, its other lanes C's -- rows,
    observations, and 200 more ticks of play."""
    rng = np.random.default_rng(n + len(kind) + len(gametype))
    A, B, C = (_make(sfa, n, gametype) for _ in range(3))
    _warm((A, B, C), WARM, seed=11)
    _worth_resetting(A)
    m = _mask(kind, n, rng)
    md = torch.from_numpy(m).to(A.device)
    sel = md != 0
    rows_c = C.save_lanes().rows
    assert torch.equal(A.save_lanes().rows, rows_c)
    sd_c = C.state_dict()
    buf = _sentinel(A)
    before = buf.clone()
    out = A.reset_lanes(mask=md, out=buf)
    assert out is buf
    obs_b = B.reset()
    rows_a, rows_b = A.save_lanes().rows, B.save_lanes().rows
    assert torch.equal(rows_a[sel], rows_b[sel])
    assert torch.equal(rows_a[~sel], rows_c[~sel])
    assert torch.equal(_bits(buf)[sel], _bits(obs_b)[sel])
    assert torch.equal(_bits(buf)[~sel], _bits(before)[~sel])
    if kind == "none":
        assert not _same_dict(A.state_dict(), sd_c)
    if kind == "all":
        assert not _same_dict(A.state_dict(), B.state_dict())
    # every env plays the game it would play alone
    acts = torch.from_numpy(_actions(200, n, A.n_actions, seed=12)).to(A.device)
    bad_b = torch.zeros(n, dtype=torch.bool, device=A.device)
    bad_c = torch.zeros(n, dtype=torch.bool, device=A.device)
    for t in range(200):
        ra, rb, rc = A.step_tensors(acts[t]), B.step_tensors(acts[t]), C.step_tensors(acts[t])
        for x, y, z in zip(ra, rb, rc):
            bad_b |= _row_diff(x, y)
            bad_c |= _row_diff(x, z)
    assert not bool((bad_b & sel).any()), torch.nonzero(bad_b & sel).flatten()[:8]
    assert not bool((bad_c & ~sel).any()), torch.nonzero(bad_c & ~sel).flatten()[:8]
    rows_a, rows_b, rows_c = A.save_lanes().rows, B.save_lanes().rows, C.save_lanes().rows
    assert torch.equal(rows_a[sel], rows_b[sel])
    assert torch.equal(rows_a[~sel], rows_c[~sel])
    A.check_state()
    for e in (A, B, C):
        e.close()


# ---------------------------------------------------------------------------------------------- 2. the oracle
@pytest.mark.parametrize("f64", [False, True])
def test_oracle_lock_step(sfa, oracle_mod, f64):
    """130 envs, 600 steps beside OracleVecEnv; every 37th step a fresh random subset is reset in both (the oracle's one env
    at a time: sfo_env_reset).  Every step's outputs and every 50th step's state are compared."""
    O = oracle_mod
    n, T = 130, 600
    rng = np.random.default_rng(2024 + f64)
    env = _make(sfa, n, obs_dtype=torch.float64 if f64 else torch.float32)
    orc = O.OracleVecEnv("youturn", n, action_set=1, spawn_stride=1)
    assert obs_close(env.reset().cpu().numpy(), orc.reset(), f64).all()
    acts = _actions(T, n, env.n_actions, seed=5)
    dacts = torch.from_numpy(acts).to(env.device)
    dead_resets = missile_resets = resets = 0
    for t in range(T):
        o, r, d, i = env.step_tensors(dacts[t])
        oo, orw, od, oi = orc.step(acts[t].astype(np.int32))
        assert np.array_equal(r.cpu().numpy(), orw), t
        assert np.array_equal(d.cpu().numpy().astype(bool), od) and np.array_equal(i.cpu().numpy().astype(bool), oi), t
        assert obs_close(o.cpu().numpy(), oo, f64).all(), t
        if t % 37 == 36:
            snaps = orc.snapshots()
            sub = rng.random(n) < 0.25
            dead = np.flatnonzero(snaps["ship_alive"] == 0)
            armed = np.flatnonzero((snaps["missile_alive"] != 0).any(1))
            if dead.size:
                sub[dead[resets % dead.size]] = True
            if armed.size:
                sub[armed[resets % armed.size]] = True
            dead_resets += int(sub[dead].sum())
            missile_resets += int(sub[armed].sum())
            lanes = np.flatnonzero(sub)
            buf = o.clone()
            if resets % 2:
                env.reset_lanes(lanes=lanes.tolist(), out=buf)
            else:
                env.reset_lanes(mask=torch.from_numpy(sub).to(env.device), out=buf)
            got, had = buf.cpu().numpy(), o.cpu().numpy()
            row = np.empty(orc.obs_dim, np.float64)
            for lane in lanes:
                orc.L.sfo_env_reset(orc.L.sfo_vec_env_at(orc.h, int(lane)), O._ptr(row))
                assert obs_close(got[lane], row, f64).all(), (t, lane)
            assert np.array_equal(got[~sub], had[~sub]), t
            resets += 1
        if t % 50 == 49:
            bad = compare_state(env.state_dict(), orc.snapshots())
            assert not bad, (t, bad)
    assert resets == 16 and dead_resets > 0 and missile_resets > 0, (resets, dead_resets, missile_resets)
    env.close()


# ---------------------------------------------------------------------------------------------- 3. manual == auto
@pytest.mark.parametrize("captured", [False, True])
def test_manual_reset_equals_auto_reset(sfa, captured):
    """A batch without auto-reset whose caller answers every `done` with reset_lanes(mask=done) is the auto-resetting batch:
    observations (the reset rows where done is set), reward, done, info, final rows.  Eagerly, and with step + reset captured
    in one graph and replayed."""
    n, T0, T = 129, 5250, 100
    P, Q = _make(sfa, n), _make(sfa, n, auto_reset=False)
    _warm((P, Q), T0, seed=21)
    assert (P.get_field("time") == 34 * T0).all() and (Q.get_field("time") == 34 * T0).all()
    dev = P.device
    acts = torch.from_numpy(_actions(T, n, P.n_actions, seed=22)).to(dev)
    bufs = (torch.zeros((n, Q.obs_dim), dtype=torch.float32, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
            torch.zeros(n, dtype=torch.uint8, device=dev), torch.zeros(n, dtype=torch.uint8, device=dev))
    a_now = torch.zeros(n, dtype=torch.uint8, device=dev)

    def one():
        Q.step_tensors(a_now, out=bufs)
        Q.reset_lanes(mask=bufs[2], out=bufs[0])

    graph = None
    if captured:
        torch.cuda.synchronize()
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with torch.cuda.graph(graph, stream=side):  # one stream, no parallel branches
                one()
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize()
    bad = torch.zeros(n, dtype=torch.bool, device=dev)
    dones = torch.zeros((), dtype=torch.int64, device=dev)
    for t in range(T):
        a_now.copy_(acts[t])
        if graph is not None:
            graph.replay()
        else:
            one()
        for x, y in zip(P.step_tensors(acts[t]), bufs):
            bad |= _row_diff(x, y)
        dones += bufs[2].sum()
    assert int(dones) == n  # every lane finished once (tick 5295) and went on
    assert not bool(bad.any()), torch.nonzero(bad).flatten()[:8]
    assert torch.equal(P.save_lanes().rows, Q.save_lanes().rows)
    assert (Q.get_field("time") == 34 * (T0 + T - 5295)).all()
    Q.check_state()
    P.close()
    Q.close()


# ---------------------------------------------------------------------------------------------- 4. the mask's bounds
@pytest.mark.parametrize("n", [65, 129])
def test_mask_bytes_behind_the_batch_are_not_read(sfa, n):
    """The mask sits with poisoned (0xFF) bytes right in front of and behind it: the lanes behind the batch in the partial
    last tile have no mask byte, and nothing may be taken for one.  (No field exposes those lanes -- get_field_tensor covers
    the batch's envs -- so what is compared is everything that would show their being reset: with no real lane of the last
    tile marked the tile must stay untouched -- pool order included, which the rows of a rebuilt pool and 60 more ticks
    against the untouched twin would tell --, and with its last real lane marked only that one changes.)"""
    A, C = _make(sfa, n), _make(sfa, n)
    _warm((A, C), WARM, seed=31)
    _worth_resetting(A)
    room = torch.full((1024,), 0xFF, dtype=torch.uint8, device=A.device)
    md = room[512 - n:512]
    md.zero_()
    tail = torch.full((4096,), 0xFF, dtype=torch.uint8, device=A.device)  # (and whatever is allocated next is poisoned too)
    fields = ("missile_mask", "shell_mask", "spawn_cursor", "time", "flags")
    had = {f: A.get_field_tensor(f).clone() for f in fields}
    sd = A.state_dict()
    A.reset_lanes(mask=md)
    assert not _same_dict(A.state_dict(), sd)
    assert torch.equal(A.save_lanes().rows, C.save_lanes().rows)
    for f in fields:
        assert torch.equal(A.get_field_tensor(f), had[f]), f
    md[n - 1] = 255
    A.reset_lanes(mask=md)
    B = _make(sfa, n)
    _warm((B,), WARM, seed=31)
    B.reset()
    ra, rb, rc = A.save_lanes().rows, B.save_lanes().rows, C.save_lanes().rows
    assert torch.equal(ra[n - 1], rb[n - 1]) and torch.equal(ra[:n - 1], rc[:n - 1])
    acts = torch.from_numpy(_actions(60, n, A.n_actions, seed=32)).to(A.device)
    bad = torch.zeros(n, dtype=torch.bool, device=A.device)
    for t in range(60):
        for x, y in zip(A.step_tensors(acts[t]), C.step_tensors(acts[t])):
            bad |= _row_diff(x, y)
    assert not bool(bad[:n - 1].any())
    assert torch.equal(A.save_lanes().rows[:n - 1], C.save_lanes().rows[:n - 1])
    A.check_state()
    assert bool((tail == 0xFF).all()) and bool((room[512:] == 0xFF).all()) and bool((room[:512 - n] == 0xFF).all())
    for e in (A, B, C):
        e.close()


# ---------------------------------------------------------------------------------------------- 5. side effects
def test_episode_stats_do_not_change(sfa):
    """An abandoned game is not a finished episode."""
    n = 65
    env = _make(sfa, n)
    env.reset()
    t = np.full(n, 34 * 5290, np.int32)
    t[::2] = 34 * 100
    env.set_field("time", t)
    _warm((env,), 10, seed=41)
    st = env.episode_stats()
    assert st[0] == n - (n + 1) // 2
    env.reset_lanes(mask=torch.ones(n, dtype=torch.uint8, device=env.device))
    assert np.array_equal(env.episode_stats(), st)
    assert (env.get_field("time") == 0).all()
    env.close()


def test_overflow_count_survives_reset_lanes(sfa):
    """The sticky count of check_state() stays through reset_lanes -- other fields of other envs may have wrapped -- and is
    cleared by reset()."""
    env = sfa.SFVecEnv(64, gametype="autoturn", auto_reset=False)
    env.reset()
    env.set_field("fire_timer", np.full(64, -32760, np.int32))
    noop = torch.zeros(64, dtype=torch.uint8, device=env.device)
    for _ in range(9):
        env.step_tensors(noop)
    with pytest.raises(OverflowError):
        env.check_state()
    env.reset_lanes(mask=torch.ones(64, dtype=torch.bool, device=env.device))
    assert (env.get_field("fire_timer") == 0).all()
    with pytest.raises(OverflowError):
        env.check_state()
    env.reset()
    env.check_state()
    env.close()


def test_a_recording_ends(sfa, tmp_path):
    env = _make(sfa, 64)
    env.start_recording()
    _warm((env,), 5, seed=51)
    with pytest.raises(RuntimeError, match="recording"):
        env.reset_lanes(lanes=[3])
    with pytest.raises(RuntimeError):
        env.save_replay(str(tmp_path / "x.sfr"))
    env.reset_lanes(lanes=[3])  # (the recording is gone: the reset goes through)
    assert env.get_field("time")[3] == 0 and env.get_field("time")[4] == 34 * 5
    env.close()


def test_episode_log_counts_from_the_reset(sfa):
    """A lane reset mid-episode later logs a record whose return, length, kills and shots count from the reset; the other
    lanes' records count from their own start.  Against the numpy model (eplogref.py)."""
    n = 130
    env = _make(sfa, n)
    log = env.enable_episode_log(capacity=1024)
    model = EpisodeLogModel(n)
    rng = np.random.default_rng(61)
    sub = rng.random(n) < 0.4
    for T, seed, reset in ((40, 62, True), (5300, 63, False)):
        a = torch.from_numpy(_actions(T, n, env.n_actions, seed)).to(env.device)
        _, rew, done, info = env.rollout(a, want_obs=False)
        model.update(rew.cpu().numpy(), done.cpu().numpy(), info.cpu().numpy(), a.cpu().numpy())
        if reset:
            env.reset_lanes(mask=torch.from_numpy(sub).to(env.device))
            model.restart_where(sub)
    recs, want = log.drain(), model.as_arrays()
    assert len(want["env"]) == n and recs["dropped"] == 0
    for k in want:
        assert np.array_equal(recs[k], want[k]), k
    late = np.isin(recs["env"], np.flatnonzero(sub))
    assert (recs["end_row"][late] == 40 + 5294).all() and (recs["end_row"][~late] == 5294).all()
    assert (recs["length"] == 5295).all()
    env.close()


def test_eplog_restart_where_alone(sfa):
    """Masked accumulators are zero afterwards, the others untouched; ring, histogram, total and row count untouched."""
    from spacefortress_amd.episodes import EpisodeLog

    n = 300
    dev = torch.device("cuda", torch.cuda.current_device())
    log, model = EpisodeLog(n, dev, capacity=64, hist=(-8, 64)), EpisodeLogModel(n)
    rng = np.random.default_rng(71)

    def feed(K, done_row=None):
        rew = rng.integers(-3, 4, (K, n)).astype(np.int32)
        done = np.zeros((K, n), np.uint8)
        if done_row is not None:
            done[-1] = done_row
        info = (rng.random((K, n)) < 0.2).astype(np.uint8)
        act = rng.integers(0, 3, (K, n)).astype(np.uint8)
        log.update(*(torch.from_numpy(x).to(dev) for x in (rew, done, info, act)))
        model.update(rew, done, info, act)

    feed(5, (np.arange(n) % 7 == 0).astype(np.uint8))
    feed(4)
    before = log.read()
    mask = (rng.random(n) < 0.5).astype(np.uint8) * 255
    log.restart_where(torch.from_numpy(mask).to(dev))
    model.restart_where(mask)
    after = log.read()
    assert before[0] == after[0] and before[1] == after[1]
    assert before[2].tobytes() == after[2].tobytes() and np.array_equal(before[3], after[3])
    feed(3, np.ones(n, np.uint8))  # every accumulator comes out as a record
    recs, want = log.drain(), model.as_arrays()
    assert recs["dropped"] == len(want["env"]) - 64
    for k in want:
        assert np.array_equal(recs[k], want[k][-64:]), k
    with pytest.raises(ValueError):
        log.restart_where(torch.zeros(n - 1, dtype=torch.uint8, device=dev))
    rc = log._L.sf_eplog_restart_where(log._h, None, log._stream())
    assert rc < 0 and b"mask" in log._L.sf_last_error()
    log.close()


# ---------------------------------------------------------------------------------------------- 6. image batches
@pytest.mark.parametrize("n,geometry", [(64, None), (129, None), (65, (.25, (130, 80, 450, 460), 3))])
def test_image_batches(sfa, n, geometry):
    """Frames after reset_lanes: the masked lanes' are the fully reset twin's, the others' the untouched twin's render(), and
    so are the next 50 steps' -- with a lane reset on the very frame its ship's explosion starts (a cached explosion picture
    and a render-order hint exist for that lane at that moment)."""
    A, B, C = (_make(sfa, n, obs_type="image", image_geometry=geometry) for _ in range(3))
    _warm((A, B, C), 300, seed=81)
    dev = A.device
    acts = torch.from_numpy(_actions(400, n, A.n_actions, seed=82)).to(dev)
    died = None
    for t in range(350):
        alive = (A.get_field_tensor("flags").clone() & 1) != 0
        for e in (A, B, C):
            frames = e.step_tensors(acts[t])[0]
        now_dead = alive & ((A.get_field_tensor("flags") & 1) == 0)
        if t >= 5 and bool(now_dead.any()):
            died = int(torch.nonzero(now_dead).flatten()[0])
            break
    assert died is not None, "no ship died in 350 ticks of random play"
    assert A.get_field("ship_death_timer")[died] <= A.tickdur  # (the tick of the death itself: the explosion's first frame)
    assert torch.equal(frames, C.render("image"))  # (the step's frames are render()'s)
    rng = np.random.default_rng(n)
    m = (rng.random(n) < 0.4).astype(np.uint8)
    m[died] = 1
    m[(died + 1) % n] = 0
    md = torch.from_numpy(m).to(dev)
    sel = md != 0
    fa = A.reset_lanes(mask=md).clone()
    fb = B.reset().clone()
    fc = C.render("image")
    assert torch.equal(fa[sel], fb[sel])
    assert torch.equal(fa[~sel], fc[~sel])
    assert torch.equal(A.render("image"), fa)
    rec_a, rec_b, rec_c = A.draw_records(), B.draw_records(from_state=True), C.draw_records()
    assert np.array_equal(rec_a[m != 0], rec_b[m != 0]) and np.array_equal(rec_a[m == 0], rec_c[m == 0])
    t0 = t + 1
    for t in range(t0, t0 + 50):
        xa, xb, xc = A.step_tensors(acts[t]), B.step_tensors(acts[t]), C.step_tensors(acts[t])
        for x, y, z in zip(xa, xb, xc):
            assert torch.equal(x[sel], y[sel]), t
            assert torch.equal(x[~sel], z[~sel]), t
    assert torch.equal(A.save_lanes().rows[sel], B.save_lanes().rows[sel])
    assert torch.equal(A.save_lanes().rows[~sel], C.save_lanes().rows[~sel])
    for e in (A, B, C):
        e.close()


# ---------------------------------------------------------------------------------------------- 7. arguments
def test_arguments(sfa):
    n = 65
    env = _make(sfa, n)
    _warm((env,), 20, seed=91)
    dev = env.device
    ok = torch.zeros(n, dtype=torch.uint8, device=dev)
    with pytest.raises(ValueError):
        env.reset_lanes()
    with pytest.raises(ValueError):
        env.reset_lanes(lanes=[1], mask=ok)
    for bad in (torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.uint8), ok[:-1],
                torch.zeros(n + 1, dtype=torch.uint8, device=dev), torch.zeros((n, 1), dtype=torch.uint8, device=dev), [0] * n):
        with pytest.raises(ValueError):
            env.reset_lanes(mask=bad)
    for bad in ([n], [-1], [0, n], torch.tensor([n], device=dev), np.array([0.5])):
        with pytest.raises(ValueError):
            env.reset_lanes(lanes=bad)
    with pytest.raises(ValueError):
        env.reset_lanes(mask=ok, out=torch.zeros((n, env.obs_dim + 1), device=dev))
    assert (env.get_field("time") == 34 * 20).all()  # (nothing above reset anything)
    sd = env.state_dict()
    env.reset_lanes(lanes=[])  # a no-op
    assert not _same_dict(env.state_dict(), sd)
    env.reset_lanes(lanes=torch.tensor([2, 64], dtype=torch.int32))
    env.reset_lanes(lanes=np.array([5]))
    t = env.get_field("time")
    assert sorted(np.flatnonzero(t == 0).tolist()) == [2, 5, 64]
    rc = env._L.sf_reset_lanes(env._h, None, None, env._stream())
    assert rc < 0 and b"mask" in env._L.sf_last_error()
    env.close()


def test_wrappers_refuse(sfa):
    """The wrappers keep per-env memory with no rule for a masked reset yet: reset_lanes is neither grown nor forwarded."""
    env = _make(sfa, 64)
    img = _make(sfa, 64, obs_type="image")
    wrappers = [sfa.SFVecNormalize(env), sfa.DeviceRollout(env, 4), sfa.FrameStack(img), sfa.FrameRollout(img, 4)]
    for w in wrappers:
        assert not hasattr(w, "reset_lanes")
        with pytest.raises(AttributeError, match="masked reset"):
            w.reset_lanes(lanes=[0])
        with pytest.raises(AttributeError, match="no attribute 'no_such_thing'"):
            w.no_such_thing
    env.close()
    img.close()
