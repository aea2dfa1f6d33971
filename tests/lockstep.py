"""The lock-step harness of the GPU tests: constructed states loaded into a batch, the batch stepped, every tick held to the CPU
oracle's.  One copy of what the step kernel's test files used to carry each:

  * `sfa`, the module-scoped fixture that imports the package (a test module takes it with `from lockstep import sfa`);
  * the oracle's statistics columns, `n_actions`, `missile_table`;
  * the state builders `fresh`, `fuzz_sparse` and `fuzz_crowded` (two fuzzers that draw in different orders: the tests'
    oracle-side event assertions hold for the states each of them makes, so they stay two);
  * `load_state` / `load_both`, `oracle_ticks` / `oracle_trace`;
  * `play`, the device's half: it steps a batch through [T, N] actions and never touches the oracle; asked to, it switches
    the event words on (sfmi.h SF_EV_*) and brings back every tick's;
  * `check_ticks`, the comparing half (the event words, where play() brought them, bit for bit): numpy only, so it runs without a GPU (tests/test_lockstep_model.py holds it to
    account there), and `same_bytes` for two batches that must agree byte for byte.

Nothing here decides WHAT a test compares: the observation rule and the ticks at which the state is fetched are arguments,
and every caller passes its own."""
import os
from collections import namedtuple

import numpy as np
import pytest

from sfcompare import compare_state, obs_close, snapshots_to_fields

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# the oracle's statistics columns (SRC/game.hh:29-43)
ST_BIG, ST_SMALL, ST_SHELL, ST_DEATHS, ST_RESETS, ST_DESTROYED, ST_MISSED, ST_SHOTS = 0, 1, 2, 3, 4, 5, 6, 7
ST_INCS = 11


@pytest.fixture(scope="module")
def sfa():
    import torch

    import spacefortress_amd as m
    from spacefortress_amd import _lib

    assert os.path.exists(_lib.LIB_PATH), "libsfmi.so not built: the GPU tests never fall back"
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return m


def n_actions(gametype):
    return 5 if gametype == "youturn" else 3  # action set 1: NOOP, FIRE, THRUST (, LEFT, RIGHT)


def missile_table():
    return np.load(os.path.join(GOLDEN, "tables.npz"))["missile_vel_by_angle"]


# ---------------------------------------------------------------- state builders

def fresh(O, gametype, n):
    """n new games, every ship parked where nothing happens to it by itself: inside the big hexagon, outside the small one."""
    base = O.OracleVecEnv(gametype, n).snapshots()
    base["ship_x"], base["ship_y"] = 455.0, 315.0
    base["ship_vx"], base["ship_vy"] = 0.0, 0.0
    return base


def fuzz_sparse(O, gametype, n, rng):
    """Constructed states, not reachable by play (as fuzz_crowded, with fewer projectiles so that a tile's pool stays within
    its first rows and the fortress lives long enough to be hit)."""
    base = O.OracleVecEnv(gametype, n).snapshots()
    tab = missile_table()
    base["ship_alive"] = rng.random(n) < 0.8
    base["ship_x"] = np.where(rng.random(n) < 0.5, rng.integers(150, 560, n), rng.uniform(150, 560, n))
    base["ship_y"] = np.where(rng.random(n) < 0.5, rng.integers(135, 495, n), rng.uniform(135, 495, n))
    base["ship_vx"] = rng.uniform(-4, 4, n) * (rng.random(n) < 0.9)
    base["ship_vy"] = rng.uniform(-4, 4, n) * (rng.random(n) < 0.9)
    base["ship_angle"] = rng.integers(0, 360, n)
    base["ship_death_timer"] = rng.integers(0, 1200, n)
    for k in ("fire_timer", "thrust_timer", "left_timer", "right_timer"):
        base[k] = rng.integers(-50, 50, n)
    for k in ("fire_flag", "thrust_flag", "left_flag", "right_flag"):
        base[k] = rng.integers(0, 2, n)
    if gametype != "youturn":
        base["left_flag"] = 0
        base["right_flag"] = 0
    base["fort_alive"] = rng.random(n) < 0.8
    base["fort_angle"] = rng.integers(0, 36, n) * 10
    base["fort_last_angle"] = rng.integers(0, 36, n) * 10
    base["fort_timer"] = rng.integers(0, 1100, n)
    base["fort_death_timer"] = rng.integers(0, 1100, n)
    base["fort_vuln_timer"] = rng.integers(0, 400, n)
    base["vlner"] = rng.integers(0, 14, n)
    base["points"] = rng.integers(0, 5, n).astype(np.float32) * np.float32(0.05)
    base["raw_points"] = base["points"] - np.float32(1.0)
    base["time"] = rng.integers(0, 5000, n) * 34
    base["tick"] = base["time"] // 34
    base["stats"] = rng.integers(0, 50, (n, 13))
    base["stats"][:, ST_DEATHS] = base["stats"][:, :3].sum(1)  # shipDeaths is the sum of killShip's three call sites
    for i in range(n):
        base["missile_alive"][i, rng.choice(20, rng.integers(0, 6), replace=False)] = 1
        base["shell_alive"][i, rng.choice(20, rng.integers(0, 9), replace=False)] = 1
    ang = rng.integers(0, 360, (n, 20))
    near = rng.random((n, 20)) < 0.3  # missiles about to hit the fortress
    base["missile_angle"] = ang
    base["missile_vx"] = tab[ang, 0]
    base["missile_vy"] = tab[ang, 1]
    base["missile_x"] = np.where(near, 355 - tab[ang, 0] + rng.uniform(-25, 25, (n, 20)), rng.uniform(-10, 720, (n, 20)))
    base["missile_y"] = np.where(near, 315 - tab[ang, 1] + rng.uniform(-25, 25, (n, 20)), rng.uniform(-10, 636, (n, 20)))
    base["shell_vx"] = rng.uniform(-6, 6, (n, 20))
    base["shell_vy"] = rng.uniform(-6, 6, (n, 20))
    hit = rng.random((n, 20)) < 0.15  # shells about to hit the ship
    base["shell_x"] = np.where(hit, (base["ship_x"] + base["ship_vx"])[:, None] - base["shell_vx"] + rng.uniform(-14, 14, (n, 20)),
                               rng.uniform(-5, 715, (n, 20)))
    base["shell_y"] = np.where(hit, (base["ship_y"] + base["ship_vy"])[:, None] - base["shell_vy"] + rng.uniform(-14, 14, (n, 20)),
                               rng.uniform(-5, 631, (n, 20)))
    return base, rng.integers(0, 14, n)


def fuzz_crowded(O, gametype, n, rng):
    """Random CONSTRUCTED states (not reachable by play): ships anywhere in the area, arbitrary velocities and timers,
    up to 20 missiles and 20 shells per lane, fortress dead or alive, any vulnerability.  Returns (snapshots, prev_vlner)."""
    base = O.OracleVecEnv(gametype, n).snapshots()
    tab = missile_table()
    base["ship_alive"] = rng.integers(0, 2, n)
    base["ship_x"] = np.where(rng.random(n) < 0.5, rng.integers(150, 560, n), rng.uniform(150, 560, n))
    base["ship_y"] = np.where(rng.random(n) < 0.5, rng.integers(135, 495, n), rng.uniform(135, 495, n))
    base["ship_vx"] = rng.uniform(-4, 4, n) * (rng.random(n) < 0.9)
    base["ship_vy"] = rng.uniform(-4, 4, n) * (rng.random(n) < 0.9)
    base["ship_angle"] = rng.integers(0, 360, n)
    base["ship_death_timer"] = rng.integers(0, 1200, n)
    for k in ("fire_timer", "thrust_timer", "left_timer", "right_timer"):
        base[k] = rng.integers(-50, 50, n)
    for k in ("fire_flag", "thrust_flag", "left_flag", "right_flag"):
        base[k] = rng.integers(0, 2, n)
    if gametype != "youturn" and gametype != "test-youturn":
        base["left_flag"] = 0
        base["right_flag"] = 0
    base["fort_alive"] = rng.random(n) < 0.8
    base["fort_angle"] = rng.integers(0, 36, n) * 10
    base["fort_last_angle"] = rng.integers(0, 36, n) * 10
    base["fort_timer"] = rng.integers(0, 1100, n)
    base["fort_death_timer"] = rng.integers(0, 1100, n)
    base["fort_vuln_timer"] = rng.integers(0, 400, n)
    base["vlner"] = rng.integers(0, 14, n)
    base["points"] = rng.integers(0, 5, n).astype(np.float32) * np.float32(0.05)
    base["raw_points"] = base["points"] - np.float32(1.0)
    base["time"] = rng.integers(0, 5000, n) * 34
    base["tick"] = base["time"] // 34
    base["stats"] = rng.integers(0, 50, (n, 13))
    base["stats"][:, 3] = base["stats"][:, :3].sum(1)  # shipDeaths = bigHex + smallHex + shell deaths (killShip's three call sites); it is not stored
    nm = rng.integers(0, 21, n)
    ns = rng.integers(0, 21, n)
    for i in range(n):
        ms = rng.choice(20, nm[i], replace=False)
        base["missile_alive"][i, ms] = 1
        ss = rng.choice(20, ns[i], replace=False)
        base["shell_alive"][i, ss] = 1
    base["missile_x"] = rng.uniform(-10, 720, (n, 20))
    base["missile_y"] = rng.uniform(-10, 636, (n, 20))
    near = rng.random((n, 20)) < 0.25  # a quarter of the missiles about to hit the fortress
    ang = rng.integers(0, 360, (n, 20))
    base["missile_angle"] = ang
    base["missile_vx"] = tab[ang, 0]
    base["missile_vy"] = tab[ang, 1]
    base["missile_x"] = np.where(near, 355 - tab[ang, 0] + rng.uniform(-25, 25, (n, 20)), base["missile_x"])
    base["missile_y"] = np.where(near, 315 - tab[ang, 1] + rng.uniform(-25, 25, (n, 20)), base["missile_y"])
    base["shell_x"] = rng.uniform(-5, 715, (n, 20))
    base["shell_y"] = rng.uniform(-5, 631, (n, 20))
    base["shell_vx"] = rng.uniform(-6, 6, (n, 20))
    base["shell_vy"] = rng.uniform(-6, 6, (n, 20))
    hit = rng.random((n, 20)) < 0.15  # some shells about to hit the ship
    base["shell_x"] = np.where(hit, (base["ship_x"] + base["ship_vx"])[:, None] - base["shell_vx"] + rng.uniform(-14, 14, (n, 20)), base["shell_x"])
    base["shell_y"] = np.where(hit, (base["ship_y"] + base["ship_vy"])[:, None] - base["shell_vy"] + rng.uniform(-14, 14, (n, 20)), base["shell_y"])
    pv = rng.integers(0, 14, n)
    return base, pv


# ---------------------------------------------------------------- loaders

def load_state(env, base, pv=None, extra=None):
    """Oracle snapshots into a batch, field by field; `pv`: prev_vlner, `extra`: further fields ({name: array})."""
    for k, v in snapshots_to_fields(base).items():
        env.set_field(k, v)
    if pv is not None:
        env.set_field("prev_vlner", np.asarray(pv, np.int32))
    for k, v in (extra or {}).items():
        env.set_field(k, v)


def make_env(sfa, gametype, base, pv=None, extra=None, f64=False, events=False, **kw):
    """A features batch (float32 rows, or float64) in the state `base`; `events`: with its event words switched on."""
    import torch

    env = sfa.SFVecEnv(len(base), gametype=gametype, obs_dtype=torch.float64 if f64 else torch.float32, **kw)
    load_state(env, base, pv, extra)
    if events:
        env.enable_events()
    return env


def load_both(sfa, O, gametype, snaps, prev_vlner=None, **kw):
    """A float64-observation batch and an oracle batch, both in the state `snaps`."""
    import torch

    n = len(snaps)
    env = sfa.SFVecEnv(n, gametype=gametype, obs_dtype=torch.float64, **kw)
    orc = O.OracleVecEnv(gametype, n, **{k: v for k, v in kw.items()
                                         if k in ("action_set", "obs_type", "spawn_stride", "spawn_skip")})
    orc.load_snapshots(snaps, prev_vlner)
    load_state(env, snaps, prev_vlner)
    return env, orc


# ---------------------------------------------------------------- the oracle's half

def oracle_ticks(orc, acts, snap_at=None):
    """Step `orc` through acts [T, n]; yields per tick (obs float64, reward, done, info, snapshots after the tick -- None
    where `snap_at(t)` is false; every tick by default --, the tick's event words uint32 [n] as SF_EV_* bits).  A generator:
    a long run is compared tick by tick, not stored."""
    for t in range(len(acts)):
        out = orc.step(np.asarray(acts[t]).astype(np.int32))
        yield out + (orc.snapshots() if snap_at is None or snap_at(t) else None, orc.events())


def oracle_trace(O, gametype, base, pv, acts, lanes=None, real_shell_count=False):
    """The oracle's side of a lock-step from the state `base` (of `lanes` of it, or of all): per tick (obs float64, reward,
    done, info, snapshots after the tick, event words)."""
    if lanes is not None:
        base, pv, acts = base[lanes], np.asarray(pv)[lanes], np.asarray(acts)[:, lanes]
    orc = O.OracleVecEnv(gametype, len(base))
    if real_shell_count:
        for i in range(len(base)):
            orc.L.sfo_env_set_faithful_bugs(orc.L.sfo_vec_env_at(orc.h, i), 0)
    orc.load_snapshots(base, pv)
    return list(oracle_ticks(orc, acts))


# ---------------------------------------------------------------- the device's half

Ticks = namedtuple("Ticks", "obs reward done info played states events", defaults=(None,))
Ticks.__doc__ = """What play() returns: obs [T, N, D], reward int32 [T, N], done and info uint8 [T, N] as the launch wrote them,
the actions played uint8 [T, N], {tick: state_dict() after that tick}, and -- where play() was asked for them -- the event
words uint32 [T, N] (sfmi.h SF_EV_*), else None."""


def play(env, acts, mode, state_at, out=None, before=None, check_state=False, events=False):
    """Step `env` through acts [T, N] (uint8) and return Ticks; the oracle is not touched.
      mode "step"     one step_tensors per tick;
           "sampled"  one step_sampled per tick: the lanes draw their own actions, `acts` gives only T, and Ticks.played is
                      what they drew (what the oracle is to be given afterwards);
           "fused"    one rollout of all T ticks.
    `state_at(t)`: whether to fetch state_dict() after tick t (None: never; a fused launch has only its last tick's).
    The outputs are written into [T, N] tensors made up front and fetched once at the end: no host round trip per tick
    but the state fetches asked for.  `out`: the four tensors every step is to write into (a caller's arena), copied from
    on the device.  `before(env)`: called right in front of the first launch, behind every upload and allocation.
    `events`: enable_events() first, and return the words of every tick: `env.events` copied on the device after each
    single step, `env.rollout_events` of a fused launch.
    Ends with check_actions(), and with check_state() if asked."""
    import torch

    T, N = np.shape(acts)
    dev = env.device
    want = state_at if state_at is not None else (lambda t: False)
    a = torch.from_numpy(np.array(acts)).to(dev)  # (a copy: a shared case's actions are read-only)
    states = {}
    ev = None
    if events:
        env.enable_events()
    if mode == "fused":
        assert out is None and not any(want(t) for t in range(T - 1)), "a fused launch leaves only its last tick's state"
        if before is not None:
            before(env)
        obs, rew, done, info = env.rollout(a)
        if events:
            ev = env.rollout_events
            assert tuple(ev.shape) == (T, N), tuple(ev.shape)
        if want(T - 1):
            states[T - 1] = env.state_dict()
        played = a
    else:
        assert mode in ("step", "sampled"), mode
        obs = torch.empty((T, N, env.obs_dim), dtype=env.obs_dtype, device=dev)
        rew = torch.empty((T, N), dtype=torch.int32, device=dev)
        done = torch.empty((T, N), dtype=torch.uint8, device=dev)
        info = torch.empty((T, N), dtype=torch.uint8, device=dev)
        played = torch.empty((T, N), dtype=torch.uint8, device=dev) if mode == "sampled" else a
        if events:
            ev = torch.empty((T, N), dtype=torch.int32, device=dev)
        if before is not None:
            before(env)
        for t in range(T):
            into = out if out is not None else (obs[t], rew[t], done[t], info[t])
            if mode == "sampled":
                env.step_sampled(out=into, actions_out=played[t])
            else:
                env.step_tensors(a[t], out=into)
            if out is not None:
                for dst, src in zip((obs[t], rew[t], done[t], info[t]), out):
                    dst.copy_(src)
            if events:
                ev[t].copy_(env.events)
            if want(t):
                states[t] = env.state_dict()
    if dev.type == "cuda":
        torch.cuda.synchronize()
    env.check_actions()
    if check_state:
        env.check_state()
    return Ticks(*(x.cpu().numpy() for x in (obs, rew, done, info, played)), states,
                 None if ev is None else ev.cpu().numpy().view(np.uint32))


def run_device(env, acts_tn):
    """play() for a caller that wants only the four output arrays of single steps: numpy obs / reward / done / info, the
    flags as bool."""
    k = play(env, acts_tn, "step", None)
    return k.obs, k.reward, k.done.astype(bool), k.info.astype(bool)


# ---------------------------------------------------------------- the comparison

def event_names(word):
    """An SF_EV_* word as the set of its names (spacefortress_amd._lib.EVENT_NAMES)."""
    from spacefortress_amd._lib import EVENT_NAMES

    return {nm for b, nm in EVENT_NAMES.items() if int(word) & b}


def _f32_bits(a, b):
    assert a.dtype == np.float32, a.dtype
    return a.view(np.uint32) == b.astype(np.float32).view(np.uint32)


def _rounded_f32_bits(a, b):
    return a.astype(np.float32).view(np.uint32) == b.astype(np.float32).view(np.uint32)


# observation rules: (device rows, the oracle's float64 rows) -> bool per cell
OBS_RULES = {
    "f32_bits": _f32_bits,                              # float32 rows: the bit patterns of the oracle's row rounded to float32
    "rounded_f32_bits": _rounded_f32_bits,              # rows of either width rounded to float32 first, then the bit patterns
    "close_f32": lambda a, b: obs_close(a, b, False),  # sfcompare.obs_close for float32 rows
    "close_f64": lambda a, b: obs_close(a, b, True),   # sfcompare.obs_close for float64 rows: 1e-9 * max(1, |x|)
}


def check_ticks(ticks, trace, obs_rule, lanes=None):
    """Hold what play() returned to the oracle's `trace` (a list or a generator of (obs, reward, done, info, snapshots, event
    words) per tick; of `lanes` of the batch, or of all of it): reward / done / info exactly, observations by `obs_rule` (a
    name of OBS_RULES, or a callable like them), every state in ticks.states through sfcompare.compare_state, and -- whenever
    ticks.events is there -- the event words exactly, every bit of every lane.  Raises AssertionError with the tick and the
    first offending indices (event words: the lanes, and per lane the names the batch has and the names the oracle has)."""
    rule = OBS_RULES[obs_rule] if isinstance(obs_rule, str) else obs_rule
    sel = slice(None) if lanes is None else lanes
    T = 0
    for t, tr in enumerate(trace):
        oo, orw, od, oi, snaps = tr[:5]
        obs, rew, done, info = ticks.obs[t][sel], ticks.reward[t][sel], ticks.done[t][sel], ticks.info[t][sel]
        bad = np.argwhere(~rule(obs, oo))
        assert bad.size == 0, (t, "obs", bad[:5].tolist(), obs[bad[0][0]].tolist(), oo[bad[0][0]].tolist())
        assert np.array_equal(rew, orw), (t, "reward", np.flatnonzero(rew != orw)[:5].tolist())
        assert np.array_equal(done.astype(bool), od), (t, "done", np.flatnonzero(done.astype(bool) != od)[:5].tolist())
        assert np.array_equal(info.astype(bool), oi), (t, "info", np.flatnonzero(info.astype(bool) != oi)[:5].tolist())
        if t in ticks.states:
            assert snaps is not None, (t, "the trace has no snapshots for a tick whose state was fetched")
            bad = compare_state(ticks.states[t], snaps, lanes=lanes)
            assert not bad, (t, "state", bad)
        if ticks.events is not None:
            assert len(tr) > 5 and tr[5] is not None, (t, "the trace has no event words")
            got, want = ticks.events[t][sel], np.asarray(tr[5], np.uint32)
            assert got.dtype == np.uint32 and got.shape == want.shape, (t, "events", got.dtype, got.shape, want.shape)
            bad = np.flatnonzero(got != want)
            assert bad.size == 0, (t, "events", bad[:5].tolist(),
                                   [(sorted(event_names(got[i])), sorted(event_names(want[i]))) for i in bad[:5]])
        T = t + 1
    assert T == len(ticks.obs), (T, len(ticks.obs))


# the kinds of launch a constructed state is played through: name -> (play mode, float64 observations).  A float32 batch
# of up to 65 536 envs is stepped by split launches; float64 rows, step_sampled and a fused rollout each by another instantiation.
LAUNCHES = {"split": ("step", False), "f64": ("step", True), "sampled": ("sampled", False), "fused": ("fused", False)}


def every(k):
    """state_at: the state after every k-th tick"""
    return lambda t: (t + 1) % k == 0


def run_lockstep(sfa, O, gametype, base, pv, acts, launch, state_at, obs_rule, lanes=None, trace=None, extra=None, before=None,
                 check_state=False, events=False, **env_kw):
    """The whole of it, for a test with nothing to do in between: a batch in the state `base` plays `acts` through `launch` (a
    name of LAUNCHES), the oracle (of `lanes`, or of all lanes) plays what the batch played -- or `trace` is the oracle's,
    made beforehand from the same given actions --, and check_ticks compares (`events`: the event words too).  Returns (the
    oracle's trace, Ticks)."""
    mode, f64 = LAUNCHES[launch]
    env = make_env(sfa, gametype, base, pv, extra, f64, **env_kw)
    ticks = play(env, acts, mode, state_at, before=before, check_state=check_state, events=events)
    env.close()
    if trace is None:
        trace = oracle_trace(O, gametype, base, pv, ticks.played, lanes, real_shell_count=not env_kw.get("faithful_bugs", True))
    check_ticks(ticks, trace, obs_rule, lanes)
    return trace, ticks


def fused_equals_steps(sfa, gametype, base, pv, acts):
    """One rollout of all of `acts` against a step per tick from the same state: the same four output arrays, byte for byte."""
    e1, e2 = make_env(sfa, gametype, base, pv), make_env(sfa, gametype, base, pv)
    same_bytes(play(e1, acts, "fused", None), play(e2, acts, "step", None))
    e1.close()
    e2.close()


def same_bytes(ticks_a, ticks_b):
    """Two batches that played the same ticks: every output and every fetched state field, byte for byte; the event words
    too where both have them."""
    for name in ("obs", "reward", "done", "info"):
        x, y = getattr(ticks_a, name), getattr(ticks_b, name)
        assert x.shape == y.shape and x.dtype == y.dtype, (name, x.shape, y.shape, x.dtype, y.dtype)
        if x.tobytes() != y.tobytes():
            bad = np.argwhere(x.view(np.uint8) != y.view(np.uint8))
            raise AssertionError((int(bad[0][0]), name, bad[:5].tolist()))
    if ticks_a.events is not None and ticks_b.events is not None:  # (one side without them: events on against events off)
        x, y = ticks_a.events, ticks_b.events
        assert x.shape == y.shape and x.dtype == y.dtype, ("events", x.shape, y.shape)
        bad = np.argwhere(x != y)
        assert bad.size == 0, (int(bad[0][0]), "events", bad[:5].tolist())
    assert sorted(ticks_a.states) == sorted(ticks_b.states), (sorted(ticks_a.states), sorted(ticks_b.states))
    for t in sorted(ticks_a.states):
        sa, sb = ticks_a.states[t], ticks_b.states[t]
        assert sorted(sa) == sorted(sb), t
        for k in sa:
            x, y = np.ascontiguousarray(sa[k]), np.ascontiguousarray(sb[k])
            assert x.tobytes() == y.tobytes(), (t, k, np.argwhere(x != y)[:5].tolist())
