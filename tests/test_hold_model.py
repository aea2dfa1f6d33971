"""The masked step's two CPU-side foundations (include/sfmi_hold.h: sf_step_where).  No GPU.

1. The inert recipe against the oracle.  sf_hold_begin_kernel swaps a held lane for a game "in which nothing can happen"
   while its tile-mates tick (holdref.inert: ship dead with death timer -(1 << 24), no projectiles, time 0, vlner =
   prev_vlner = 0, counters and key timers zero).  Snapshots of every golden run are made inert and played for 255 ticks --
   the longest window -- under every action of both action tables, held down, and under random actions: reward 0, no kill, no
   game over, no projectile, no respawn, no death, hit or miss counted, the score and the ship where they were.
2. The model against itself (holdref.HoldModel): a lane's c-th active step is step c of the same lane played alone.
3. The header and the binding name the same entry point with the same arguments.
"""
import json
import os
import re

import numpy as np
import pytest

import holdref as H
from conftest import GOLDEN, golden_names

# the statistics no inert tick may move (SRC/game.hh:29-43): deaths (0-3), resets, destroyed, missed; vlner incs, max vlner
QUIET_STATS = (0, 1, 2, 3, 4, 5, 6, 11, 12)
FROZEN = ("ship_x", "ship_y", "ship_vx", "ship_vy", "points", "raw_points", "vlner", "ship_alive")


def _golden_snapshots(name, k=6):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    meta = json.loads(str(z["meta"]))
    snaps = z["snaps"]
    # k of them spread over the run, and the ones with the most projectiles and a dead ship where there are any
    pick = set(np.linspace(0, len(snaps) - 1, k).astype(int).tolist())
    pick.add(int(np.argmax(snaps["missile_alive"].sum(1) + snaps["shell_alive"].sum(1))))
    dead = np.flatnonzero(snaps["ship_alive"] == 0)
    if len(dead):
        pick.add(int(dead[0]))
    return meta["gametype"], snaps[sorted(pick)]


@pytest.mark.parametrize("action_set", [0, 1])
@pytest.mark.parametrize("name", golden_names())
def test_an_inert_game_stays_inert_for_a_whole_window(oracle_mod, name, action_set):
    O = oracle_mod
    gametype, snaps = _golden_snapshots(name)
    n_act = O.OracleVecEnv(gametype, 1, action_set=action_set)
    n_act = n_act.L.sfo_env_n_actions(n_act.L.sfo_vec_env_at(n_act.h, 0))
    S = len(snaps)
    # lane = (snapshot, schedule): every action held down, then one random schedule (key edges on every tick)
    base = H.inert(np.repeat(snaps, n_act + 1))
    n = len(base)
    orc = O.OracleVecEnv(gametype, n, action_set=action_set)
    orc.load_snapshots(base, np.zeros(n, np.int32))
    rng = np.random.default_rng([5, len(name), action_set])
    const = np.tile(np.arange(n_act + 1), S)
    for t in range(255):
        acts = np.where(const < n_act, const, rng.integers(0, n_act, n)).astype(np.int32)
        obs, rew, done, info = orc.step(acts)
        assert not rew.any() and not done.any() and not info.any(), (t, np.flatnonzero(rew), np.flatnonzero(done))
        if t in (0, 1, 31):  # (`collisions`: the tick's own four collision flags)
            assert not orc.snapshots()["collisions"].any(), t
    s = orc.snapshots()
    assert not s["collisions"].any()
    assert not s["ship_alive"].any() and not s["missile_alive"].any() and not s["shell_alive"].any()
    assert (s["time"] == 255 * 34).all() and (s["ship_death_timer"] == H.INERT_DEATH + 255 * 34).all()
    assert not s["stats"][:, QUIET_STATS].any(), np.argwhere(s["stats"][:, QUIET_STATS])[:5]
    assert (orc.prev_vlner() == 0).all()
    for k in FROZEN:
        assert s[k].tobytes() == base[k].tobytes(), k


def test_the_longest_window_is_far_from_a_respawn_and_from_game_over():
    """the two margins the recipe rests on: 255 ticks add 8 670 ms to a death timer that starts at -(1 << 24), and a game
    that starts at time 0 is over after 5 295 ticks"""
    assert H.INERT_DEATH + 255 * 34 < 0 and 255 * 34 < 180000 and -(-180000 // 34) == 5295


@pytest.mark.parametrize("gametype,auto_reset,K", [("youturn", True, 1), ("autoturn", True, 4), ("youturn", False, 1)])
def test_a_lanes_active_steps_are_the_lane_played_alone(oracle_mod, gametype, auto_reset, K):
    from lockstep import fuzz_crowded

    O = oracle_mod
    n, T = 72, 60
    rng = np.random.default_rng([11, len(gametype), K])
    base, pv = fuzz_crowded(O, gametype, n, rng)
    base["time"] = 180000 - 34 * rng.integers(1, 30, n)  # most lanes finish inside the run
    base["time"][::5] = 3400
    base["tick"] = base["time"] // 34
    masked = H.HoldModel(gametype, base, pv, auto_reset=auto_reset)
    alone = H.HoldModel(gametype, base, pv, auto_reset=auto_reset)
    acts = rng.integers(0, masked.n_actions, (T, n))
    masks = H.draw_masks(rng, n, T, stretch=7)
    every = np.ones(n, bool)
    plain = [alone.step_where(acts[c], every, K) for c in range(T)]
    for t in range(T):
        c = masked.steps.copy()
        a = acts[c, np.arange(n)]  # lane i plays the action of ITS c-th step
        before = masked.snapshots()
        out = masked.step_where(a, masks[t], K)
        after = masked.snapshots()
        for i in range(n):
            if masks[t, i]:
                want = plain[c[i]]
                for k in ("rew", "done", "info", "ticks"):
                    assert out[k][i] == want[k][i], (t, i, k)
                assert out["obs"][i].tobytes() == want["obs"][i].tobytes(), (t, i)
                assert np.array_equal(out["final"][i], want["final"][i], equal_nan=True), (t, i)
            else:
                assert out["rew"][i] == 0 and not out["done"][i] and not out["info"][i] and out["ticks"][i] == 0
                assert before[i].tobytes() == after[i].tobytes(), (t, i)
    assert masked.steps.min() >= 5 and (masked.steps < T).any()
    if auto_reset:
        assert len(masked.ep_returns) >= n // 2


def test_header_and_binding_agree():
    from spacefortress_amd import _lib as lib
    from spacefortress_amd import build as sfbuild

    path = os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "sfmi_hold.h")
    text = open(path).read()
    bare = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert set(re.findall(r"\b(sf_[a-z_0-9]+)\s*\(", bare)) == set(lib.HOLD_SYMBOLS) == {"sf_step_where"}
    m = re.search(r"sf_step_where\(([^)]*)\)", bare)
    assert m and len(m.group(1).split(",")) == len(lib.HOLD_SYMBOLS["sf_step_where"][1]) == 11
    assert os.path.abspath(path) in [os.path.abspath(h) for h in sfbuild.HEADERS if os.path.isabs(h)]
    for word in ("may or may not be counted", "SF_FLAG_NO_AUTO_RESET", "captured"):
        assert word in text, word
