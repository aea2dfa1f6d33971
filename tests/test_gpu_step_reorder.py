"""The split launches of the step kernel (a games' wave and a missile wave per tile, hand-over through LDS) against the CPU
oracle, in the scenarios in which the ORDER of the games' wave's tail matters: what the missile wave's events still change
(fortress alive, vlner, kill_ready, the missile count and feature 14 where it mirrors it) against what is final once the
shells are done (the ship, the bearings, the shell count, the key timers), and lanes that start a new game while their
neighbours play on.  Written with a reordering of that tail (the independent part in front of the poll of the missile wave's
word; measured, not kept: profiles/step_handover_fill.md); they hold any order to the oracle's results.  The missile wave
asks only for the pool rows it has: tiles without a missile, with one row and with several rows are all here.

At the smallest shapes that run the split instantiations -- 64 and 256 envs (64 envs per workgroup: one tile, four tiles),
16 448 (128 per workgroup) and 32 832 (256) -- in lock-step with the oracle:

  * observation rows as float32 BIT PATTERNS (the oracle's float64 row rounded to float32: the integers are exact, and the
    three bearings' doubles agree to 1e-13 relative, which moves a float32 rounding once in 1e7 values),
  * reward / done / info exactly,
  * the state bit for bit (sfcompare.compare_state: shell positions to 1e-9, as everywhere).

Each scenario asserts, from the ORACLE's side, that the event it is about happened in the compared ticks."""
import os

import numpy as np
import pytest

from lockstep import (ST_BIG, ST_DESTROYED, ST_INCS, ST_MISSED, ST_RESETS, ST_SHELL, ST_SHOTS, ST_SMALL, every, fresh, fuzz_sparse,
                      missile_table, n_actions, oracle_trace, run_lockstep, sfa)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GAMETYPES = ["youturn", "autoturn"]
SMALL = [64, 256]


def _lockstep(sfa, gametype, base, pv, acts, trace, real_shell_count=False, lanes=None):
    """Load `base` into a float32 features batch (what split launches serve), play `acts`, compare every tick with `trace`
    (the oracle's, of `lanes` of the batch or of all of it): rows as float32 bit patterns, the event words bit for bit; small batches: the state after
    every tick, the others after the last."""
    run_lockstep(sfa, None, gametype, base, pv, acts, "split", every(1 if len(base) <= 256 else len(acts)), "f32_bits", lanes=lanes,
                 trace=trace, events=True, faithful_bugs=not real_shell_count)


# ---------------------------------------------------------------- 1. lanes of one tile finishing on different ticks

def _setup_finish(O, gametype, n, together):
    rng = np.random.default_rng(100 + n + len(gametype) + int(together))
    base, pv = fuzz_sparse(O, gametype, n, rng)
    left = np.array([2, 3, 5, 400])[np.arange(n) % 4] if not together else np.full(n, 2)  # ticks to game over
    base["time"] = 180000 - 34 * left
    base["tick"] = base["time"] // 34
    return base, pv, rng.integers(0, n_actions(gametype), (7, n)).astype(np.uint8)


def _events_finish(trace, n, together):
    done = np.array([tr[2] for tr in trace])  # [T, n]
    tiles = done.reshape(len(trace), n // 64, 64)
    if together:
        assert tiles[1].all() and done.sum() == n
    else:
        for t in (1, 2, 4):  # each of these ticks ends some lanes of every tile, not all
            assert (tiles[t].any(1) & ~tiles[t].all(1)).all(), t
        assert done.sum() == 3 * (n // 4)


@pytest.mark.parametrize("together", [False, True])
@pytest.mark.parametrize("n", SMALL)
@pytest.mark.parametrize("gametype", GAMETYPES)
def test_new_games_inside_a_tile(sfa, oracle_mod, gametype, n, together):
    """Ticks t, t + 1 and t + 3 each end some lanes of a tile but not all (then: the whole tile in one tick).  The new games'
    rows and ship chunks are the oracle's, the neighbours' rows untouched."""
    base, pv, acts = _setup_finish(oracle_mod, gametype, n, together)
    trace = oracle_trace(oracle_mod, gametype, base, pv, acts)
    _events_finish(trace, n, together)
    _lockstep(sfa, gametype, base, pv, acts, trace)


# ---------------------------------------------------------------- 2. the ship's state changes in the shells phase

def _setup_ship(O, gametype, n):
    """Lane i % 8: 0 a shell kills the ship, 1 the big hexagon, 2 the small hexagon, 3 a dead ship respawns, 4 a shell kills
    it while another leaves the area, 5 a shell passes a DEAD ship, 6 and 7 fly on."""
    rng = np.random.default_rng(200 + n)
    base = fresh(O, gametype, n)
    kind = np.arange(n) % 8
    for i in range(n):
        k = kind[i]
        if k in (0, 4, 5):
            s = int(rng.integers(0, 6))
            base["shell_alive"][i, s] = 1
            base["shell_vx"][i, s], base["shell_vy"][i, s] = rng.uniform(-6, 6, 2)
            base["shell_x"][i, s] = 455.0 - base["shell_vx"][i, s] + rng.uniform(-3, 3)
            base["shell_y"][i, s] = 315.0 - base["shell_vy"][i, s] + rng.uniform(-3, 3)
            if k == 4:
                base["shell_alive"][i, s + 7] = 1
                base["shell_x"][i, s + 7], base["shell_y"][i, s + 7] = 709.5, 300.0
                base["shell_vx"][i, s + 7], base["shell_vy"][i, s + 7] = 5.0, 0.5
            if k == 5:
                base["ship_alive"][i] = 0
                base["ship_death_timer"][i] = 34 * 3
        elif k == 1:
            base["ship_x"][i], base["ship_y"][i] = 355.0 + rng.integers(-40, 40), 143.0
            base["ship_vy"][i] = -4.0
        elif k == 2:
            base["ship_x"][i], base["ship_y"][i] = 355.0, 352.0
            base["ship_vy"][i] = -4.0
        elif k == 3:
            base["ship_alive"][i] = 0
            base["ship_death_timer"][i] = 1000 + 34 * int(rng.integers(0, 3))
    acts = np.zeros((3, n), np.uint8)  # nobody thrusts: the ships move as set up
    acts[:, kind >= 6] = rng.integers(0, n_actions(gametype), (3, int((kind >= 6).sum())))
    return base, np.zeros(n, np.int32), acts


def _events_ship(base, trace, n):
    kind = np.arange(n) % 8
    d = trace[0][4]["stats"] - base["stats"]  # what the first tick counted
    assert (d[kind == 0, ST_SHELL] == 1).all() and (d[kind == 4, ST_SHELL] == 1).all()
    assert (d[kind == 1, ST_BIG] == 1).all() and (d[kind == 2, ST_SMALL] == 1).all()
    assert (trace[0][4]["ship_alive"][np.isin(kind, (0, 1, 2, 4))] == 0).all()
    assert (trace[0][4]["ship_alive"][kind == 3] == 1).all()                          # respawned in the compared tick
    assert (trace[0][4]["shell_alive"][kind == 4].sum(1) == 0).all()                  # one hit, one left the area
    assert (trace[0][4]["shell_alive"][kind == 5].sum(1) == 1).all() and (d[kind == 5, ST_SHELL] == 0).all()
    assert (trace[0][0][np.isin(kind, (0, 1, 2, 4)), 0] == 0).all()                   # feature 0 of the same tick


@pytest.mark.parametrize("n", SMALL)
@pytest.mark.parametrize("gametype", GAMETYPES)
def test_ship_dies_and_respawns_in_the_compared_tick(sfa, oracle_mod, gametype, n):
    """Feature 0 and the death timer of a ship killed by a shell, by each hexagon, and of one that respawns."""
    base, pv, acts = _setup_ship(oracle_mod, gametype, n)
    trace = oracle_trace(oracle_mod, gametype, base, pv, acts)
    _events_ship(base, trace, n)
    _lockstep(sfa, gametype, base, pv, acts, trace)


# ---------------------------------------------------------------- 3. missile outcomes: what the late features must still see

def _setup_missiles(O, gametype, n):
    """Lane i % 8: 0 a vlner increment, 1 a vlner reset, 2 a fortress destruction, 3 a miss, 4 increment then reset (two hits
    in one tick), 5 a hit and a miss in one tick, 6 a hit on a dead fortress, 7 nothing."""
    rng = np.random.default_rng(300 + n)
    base = fresh(O, gametype, n)
    tab = missile_table()
    kind = np.arange(n) % 8

    def put(i, s, hit):
        ang = int(rng.integers(0, 360))
        base["missile_alive"][i, s] = 1
        base["missile_angle"][i, s] = ang
        base["missile_vx"][i, s], base["missile_vy"][i, s] = tab[ang]
        if hit:  # on the fortress after this tick's move
            base["missile_x"][i, s] = 355 - tab[ang, 0] + rng.uniform(-5, 5)
            base["missile_y"][i, s] = 315 - tab[ang, 1] + rng.uniform(-5, 5)
        else:    # outside the area after this tick's move, whatever the heading
            base["missile_x"][i, s], base["missile_y"][i, s] = -50.0, 300.0

    for i in range(n):
        k, s = kind[i], int(rng.integers(0, 8))
        base["fort_vuln_timer"][i] = 300 if k in (0, 4) else 100
        base["vlner"][i] = 12 if k == 2 else 5
        if k in (0, 1, 2, 4, 5, 6):
            put(i, s, True)
        if k in (4,):
            put(i, s + 5, True)
        if k in (3, 5):
            put(i, s + 9, False)
        if k == 6:
            base["fort_alive"][i] = 0
            base["fort_death_timer"][i] = 34
    acts = np.zeros((2, n), np.uint8)
    acts[1] = rng.integers(0, n_actions(gametype), n)
    return base, base["vlner"].astype(np.int32), acts


def _events_missiles(base, trace, n):
    kind = np.arange(n) % 8
    d = trace[0][4]["stats"] - base["stats"]
    s1 = trace[0][4]
    assert (d[kind == 0, ST_INCS] == 1).all() and (s1["vlner"][kind == 0] == 6).all()
    assert (d[kind == 1, ST_RESETS] == 1).all() and (s1["vlner"][kind == 1] == 0).all()
    assert (d[kind == 2, ST_DESTROYED] == 1).all() and (s1["fort_alive"][kind == 2] == 0).all()
    assert (d[kind == 3, ST_MISSED] == 1).all()
    assert (d[kind == 4, ST_INCS] == 1).all() and (d[kind == 4, ST_RESETS] == 1).all() and (s1["vlner"][kind == 4] == 0).all()
    assert (d[kind == 5, ST_RESETS] == 1).all() and (d[kind == 5, ST_MISSED] == 1).all()
    assert (d[kind == 6][:, [ST_INCS, ST_RESETS, ST_DESTROYED]] == 0).all() and (s1["missile_alive"][kind == 6].sum(1) == 0).all()
    assert (s1["missile_alive"][kind != 7].sum(1) == 0).all()        # feature 13 (and 14, its mirror) fell in the compared tick
    assert (trace[0][0][kind == 2, 9] == 0).all() and trace[0][1][kind == 2].min() > 0  # fortress gone, and rewarded


@pytest.mark.parametrize("n", SMALL)
@pytest.mark.parametrize("gametype", GAMETYPES)
def test_missile_outcomes_reach_the_late_features(sfa, oracle_mod, gametype, n):
    """Fortress alive, vlner, kill_ready and the missile count depend on what the missile wave hands over: every outcome of a
    missile, and two of them in one lane and tick."""
    base, pv, acts = _setup_missiles(oracle_mod, gametype, n)
    trace = oracle_trace(oracle_mod, gametype, base, pv, acts)
    _events_missiles(base, trace, n)
    _lockstep(sfa, gametype, base, pv, acts, trace)


# ---------------------------------------------------------------- 4. key timers

def _setup_keys(O, gametype, n):
    """Every key pressed in one tick and released in the next, lane i starting i % 8 ticks into the sequence; the timers start
    at values of their own, so that a missed zeroing shows."""
    base = fresh(O, gametype, n)
    rng = np.random.default_rng(400 + n)
    for k in ("fire_timer", "thrust_timer", "left_timer", "right_timer"):
        base[k] = -rng.integers(3, 40, n)  # released for a while
    seq = np.array([1, 0, 2, 0, 3, 0, 4, 0] if gametype == "youturn" else [1, 0, 2, 0, 1, 2, 0, 0], np.uint8)
    T = 12
    acts = np.stack([seq[(t + np.arange(n)) % 8] for t in range(T)])
    return base, np.zeros(n, np.int32), acts


def _events_keys(base, trace, gametype):
    keys = ("fire", "thrust", "left", "right")[:4 if gametype == "youturn" else 2]
    for k in keys:
        fl = np.array([base[k + "_flag"]] + [tr[4][k + "_flag"] for tr in trace])      # [T + 1, n]
        tm = np.array([tr[4][k + "_timer"] for tr in trace])
        press = (fl[1:-1] == 1) & (fl[:-2] == 0) & (fl[2:] == 0)                          # pressed in tick t, released in t + 1
        assert press.any(0).all(), k                                                      # ... in every lane
        t, i = np.nonzero(press)
        assert (tm[t, i] == 1).all() and (tm[t + 1, i] == -1).all(), k                   # an edge zeroes, then +-1


@pytest.mark.parametrize("n", SMALL)
@pytest.mark.parametrize("gametype", GAMETYPES)
def test_key_timers_on_press_and_release_edges(sfa, oracle_mod, gametype, n):
    """Features 15-18 (15-16) on a press and a release edge of every key in consecutive ticks."""
    base, pv, acts = _setup_keys(oracle_mod, gametype, n)
    trace = oracle_trace(oracle_mod, gametype, base, pv, acts)
    _events_keys(base, trace, gametype)
    _lockstep(sfa, gametype, base, pv, acts, trace)


# ---------------------------------------------------------------- 5. feature 14: the shell count, or the missile count's mirror

@pytest.mark.parametrize("real_shell_count", [False, True])
@pytest.mark.parametrize("gametype", GAMETYPES)
def test_feature_14_real_and_mirrored(sfa, oracle_mod, gametype, real_shell_count):
    """SFVecEnv(faithful_bugs=False) reports the shells (final once the shells are done); the default mirrors the missile
    count, which the missile wave's events still change."""
    n = 256
    rng = np.random.default_rng(500 + len(gametype))
    base, pv = fuzz_sparse(oracle_mod, gametype, n, rng)
    acts = rng.integers(0, n_actions(gametype), (6, n)).astype(np.uint8)
    trace = oracle_trace(oracle_mod, gametype, base, pv, acts, real_shell_count=real_shell_count)
    f13 = np.array([tr[0][:, 13] for tr in trace])
    f14 = np.array([tr[0][:, 14] for tr in trace])
    assert (np.diff(f13, axis=0) < 0).any()  # missiles left in compared ticks
    if real_shell_count:
        assert (f14 != f13).any() and (np.diff(f14, axis=0) != 0).any()
        assert all(np.array_equal(f14[t], tr[4]["shell_alive"].sum(1)) for t, tr in enumerate(trace))
    else:
        assert np.array_equal(f14, f13)
    _lockstep(sfa, gametype, base, pv, acts, trace, real_shell_count)


# ---------------------------------------------------------------- 6. the larger workgroups

@pytest.mark.parametrize("n", [16448, 32832])
@pytest.mark.parametrize("gametype", GAMETYPES)
def test_forty_ticks_at_128_and_256_envs_per_workgroup(sfa, oracle_mod, gametype, n):
    """Forty random ticks from constructed states at the two larger split shapes (one tile past 16 384 / 32 768 envs), a
    seeded sample of 256 lanes against the oracle, the last tile's lanes among them."""
    rng = np.random.default_rng(600 + n + len(gametype))
    T = 40
    base, pv = fuzz_sparse(oracle_mod, gametype, n, rng)
    base["time"][rng.random(n) < 0.02] = 180000 - 34 * 20  # a few lanes start a new game on the way
    base["tick"] = base["time"] // 34
    acts = rng.integers(0, n_actions(gametype), (T, n)).astype(np.uint8)
    lanes = np.sort(np.concatenate([rng.choice(n - 64, 224, replace=False), n - 64 + rng.choice(64, 32, replace=False)]))
    trace = oracle_trace(oracle_mod, gametype, base, pv, acts, lanes)
    d = trace[-1][4]["stats"] - base["stats"][lanes]
    assert np.array([tr[2] for tr in trace]).any()  # new games among the sampled lanes (their statistics start over)
    assert (d[:, [ST_SHELL, ST_RESETS, ST_MISSED, ST_SHOTS]] > 0).any(0).all()
    _lockstep(sfa, gametype, base, pv, acts, trace, lanes=lanes)


# ---------------------------------------------------------------- the batches above are stepped by split launches

_SAYS_SPLIT = """
import sys, numpy as np, torch
sys.path.insert(0, sys.argv[1])
import spacefortress_amd as m
env = m.SFVecEnv(int(sys.argv[2]), gametype=sys.argv[3], faithful_bugs=sys.argv[4] == "1")
env.set_field("time", np.zeros(env.num_envs, np.int32))
env.step_tensors(torch.zeros(env.num_envs, dtype=torch.uint8, device=env.device))
torch.cuda.synchronize()
print("stepped", file=sys.stderr, flush=True)
env.close()
"""


@pytest.mark.parametrize("gametype,n,faithful", [("youturn", 64, 1), ("autoturn", 32832, 0)])
def test_these_batches_step_by_split_launches(gametype, n, faithful):
    """Everything above is about the split instantiations: a batch made the way _lockstep makes it (float32 features, fields
    set, either shell count) must be stepped by one.  With SFMI_FORCE_SPLIT=2 the launcher says so on stderr the first time
    it splits (these batches are within the bound at which it splits by itself; the variable forces nothing here): in a
    child process, where that first time is this batch's first step (the launcher says it once per process)."""
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", _SAYS_SPLIT, root, str(n), gametype, str(faithful)], env=dict(os.environ, SFMI_FORCE_SPLIT="2"),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lanes = (n + 255) // 256 * 256
    said, stepped = r.stderr.find("sfmi: split launch (%d lanes)" % lanes), r.stderr.find("stepped")
    assert 0 <= said < stepped, r.stderr[-2000:]
