"""The CPU oracle (oracle/sf_oracle.c) against the golden vectors generated
from the real reference engine (tests/golden/make_golden.py), and against the
reference itself: live where the reference build is present (build container),
elsewhere as digests of the same runs (tests/golden/make_live_golden.py).

Bar: every field bit-exact (the oracle makes the same libm calls on the same
host libm as the reference did)."""
import hashlib
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden_names
from sfscript import aimed_hunter_actions, open_loop_actions

# extras are stale heap in the reference until the first tick (SRC/game.cpp:78, SURVEY 8a note 4)
RESET_MASKED = ("vdir", "fdist", "ndist", "aim")


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    return z, json.loads(str(z["meta"]))


def fields_differing(a, b, skip=()):
    return [f for f in a.dtype.names if f not in skip and a[f].tobytes() != b[f].tobytes()]


def shaped_reward(eng, vlner, shaped):
    """ENV:233-244 applied to an engine-reward / vulnerability series (numpy restatement
    used only to cross-check the C one)."""
    out = np.empty_like(eng)
    prev = 0
    for t in range(len(eng)):
        r = int(eng[t])
        kill = r > 0
        if shaped:
            if vlner[t] <= 10 and not kill:
                r += int(vlner[t]) - prev
            r = max(-1, min(1, r)) + 2 * int(kill)
            prev = int(vlner[t])
        out[t] = r
    return out


@pytest.mark.parametrize("name", golden_names())
def test_oracle_replays_golden(oracle_mod, name):
    O = oracle_mod
    z, meta = load(name)
    env = O.OracleEnv(meta["gametype"], action_set=meta["action_set"], seed=meta["seed"],
                      spawn_skip=meta["spawn_skip"])
    keys = np.array(env.action_keys(), np.uint8)
    assert np.array_equal(keys[z["actions"]], z["keys"])
    bad = fields_differing(env.snapshot(), z["reset_snaps"][0], RESET_MASKED)
    assert not bad, ("initial state", bad)
    out = env.replay(z["actions"])
    assert np.array_equal(out["reward"], z["reward"])
    assert np.array_equal(out["done"], z["done"].astype(bool))
    assert np.array_equal(out["info"], z["info"].astype(bool))
    s = out["snaps"]
    for k in ("ship_x", "ship_y", "vlner", "points", "raw_points"):
        assert s[k].tobytes() == z["scal_" + k].astype(s[k].dtype).tobytes(), (name, k)
    assert np.array_equal(s["missile_alive"].sum(1), z["scal_n_missiles"])
    assert np.array_equal(s["shell_alive"].sum(1), z["scal_n_shells"])
    every = meta["snap_every"]
    sub = s[every - 1::every]
    assert len(sub) == len(z["snaps"])
    bad = fields_differing(sub, z["snaps"])
    assert not bad, (name, bad)
    assert len(out["reset_snaps"]) == len(z["reset_snaps"]) - 1
    bad = fields_differing(out["reset_snaps"], z["reset_snaps"][1:], RESET_MASKED)
    assert not bad, (name, "reset", bad)


def test_oracle_features_follow_state(oracle_mod):
    """ENV:134-157 feature vector from the golden state (features obs)."""
    O = oracle_mod
    z, meta = load("youturn_hunter")
    env = O.OracleEnv("youturn")
    out = env.replay(z["actions"])
    s = z["snaps"]
    nm = s["missile_alive"].sum(1)
    exp = np.stack([s["ship_alive"], s["ship_x"], s["ship_y"], s["ship_vx"], s["ship_vy"], s["ship_angle"],
                    s["aim"], s["vdir"], s["ndist"], s["fort_alive"], s["fort_angle"], s["vlner"],
                    ((s["vlner"] > 10) & (s["fort_vuln_timer"] < 250)).astype(np.float64), nm, nm,
                    s["fire_timer"], s["thrust_timer"], s["left_timer"], s["right_timer"]], 1).astype(np.float64)
    assert out["obs"].shape == (len(s), 19)
    assert np.array_equal(out["obs"], exp)
    z, meta = load("autoturn_destroy")
    out = O.OracleEnv("autoturn").replay(z["actions"])
    assert out["obs"].shape[1] == 17
    assert np.array_equal(out["obs"][:, 11], z["snaps"]["vlner"])
    assert out["obs"][:, 12].max() == 1  # kill-ready seen during the burst


def test_other_obs_types(oracle_mod):
    """ENV:96-133 on the oracle: shapes, clipping, and the relations to `features`."""
    O = oracle_mod
    z, meta = load("youturn_hunter")
    f = O.OracleEnv("youturn", obs_type="features").replay(z["actions"])["obs"]
    n = O.OracleEnv("youturn", obs_type="normalized-features").replay(z["actions"])["obs"]
    m = O.OracleEnv("youturn", obs_type="monitors").replay(z["actions"])["obs"]
    assert n.shape == f.shape and m.shape == (len(f), 10)
    assert n.min() >= -1 and n.max() <= 1
    assert np.array_equal(n[:, 1], np.clip(f[:, 1] / 90, -1, 1))
    assert np.array_equal(n[:, 5], f[:, 5] / 360)
    assert np.array_equal(n[:, 7], np.mod(f[:, 7], 360) / 360)
    assert np.array_equal(n[:, 11], np.ones(len(f)))  # max(vlner, 10)/10 >= 1, clipped (ENV:122,133)
    assert np.array_equal(n[:, 15], np.clip(f[:, 15] / 5294.0, -1, 1))
    assert set(np.unique(m)) <= {-0.5, 0.5}
    assert np.array_equal(m[:, 0] > 0, f[:, 13] > 0)
    assert np.array_equal(m[:, 6] > 0, f[:, 8] > .75)


def test_action_tables_match_numpy_meshgrid(oracle_mod):
    """ENV:67-89: the frozen meshgrid tables equal numpy's own."""
    O = oracle_mod
    from golden.make_golden import action_table

    for gt in ("youturn", "autoturn", "test-youturn", "test-autoturn"):
        for aset in (1, 0, -1):
            env = O.OracleEnv(gt, action_set=aset)
            assert env.action_keys() == action_table(gt, aset), (gt, aset)


def test_rng_matches_libc(oracle_mod):
    """glibc TYPE_3 restatement against libc rand() itself and the golden spawns."""
    import ctypes

    O = oracle_mod
    libc = ctypes.CDLL("libc.so.6")
    for seed in (1, 2, 12345, 0xFFFFFFFF):
        libc.srand(seed)
        r = O.OracleRng(seed)
        assert [libc.rand() for _ in range(2000)] == [r.rand() for _ in range(2000)]
    libc.srand(1)
    tab = np.load(os.path.join(GOLDEN, "tables.npz"))
    for seed in (1, 12345):
        env = O.OracleEnv("youturn", seed=seed)
        for i in range(1024):
            s = env.snapshot()
            assert (int(s["ship_x"]), int(s["ship_y"]), int(s["ship_angle"])) == tuple(tab["spawns_seed%d" % seed][i])
            env.new_game()


def test_tables(oracle_mod):
    O = oracle_mod
    tab = np.load(os.path.join(GOLDEN, "tables.npz"))
    env = O.OracleEnv("youturn")
    assert np.array_equal(env.hex_points(), tab["hex_points"])
    s = env.snapshot()
    assert (s["ship_vx"], s["ship_vy"]) == tuple(tab["start_vel"])
    assert float(tab["start_vel"][0]).hex() == "0x1.0000000000001p-1"  # SURVEY 3.2 [probe]
    assert float(tab["start_vel"][1]).hex() == "-0x1.bb67ae8584caap-1"
    # first spawns of the unseeded stream, SURVEY 8c [probe]
    assert [tuple(r) for r in tab["spawns_seed1"][:3]] == [(287, 295, 113), (425, 436, 12), (419, 151, 122)]


def test_wrapper_known_answers():
    """SURVEY 8a/a13 [probe] pins observed on the real Python wrapper: +1 on each of
    vlner 1..10, 0 on the 11th, 3 with info=True on destroy; points 1.0, raw 0.35."""
    z, meta = load("autoturn_destroy")
    r, info = z["reward"], z["info"]
    nz = np.flatnonzero(r)[:11]
    assert list(r[nz]) == [1] * 10 + [3] and list(info[nz]) == [0] * 10 + [1]
    k = nz[-1]
    assert z["scal_vlner"][k] == 0 and z["scal_vlner"][k - 1] == 11
    assert z["scal_points"][k] == np.float32(1.0)
    # raw points: one f32 add of -0.05f per missile, then +1 (SRC/game.cpp:97-102); 13 missiles
    # would give the survey's 0.34999990463256836, this script's 14 give 0.29999..
    acc = np.float32(0)
    for _ in range(int(z["snaps"][k]["stats"][7])):
        acc = np.float32(acc + np.float32(-0.05))
    assert z["scal_raw_points"][k] == np.float32(acc + np.float32(1))
    acc13 = np.float32(0)
    for _ in range(13):
        acc13 = np.float32(acc13 + np.float32(-0.05))
    assert float(np.float32(acc13 + np.float32(1))) == 0.34999990463256836
    # truncation case: a press on the kill tick hides the kill (-0.05 + 1 -> (int) 0)
    z2, _ = load("autoturn_destroy_truncated")
    assert z2["snaps"][-1]["stats"][5] >= 1 and z2["info"].sum() == 0
    k2 = np.flatnonzero(z2["reward"])[10]
    assert z2["reward"][k2] == -1 and z2["eng_reward"][k2] == 0


def test_episode_length():
    z, meta = load("youturn_random_ep")
    assert np.flatnonzero(z["done"]).tolist() == [5294]  # 5295 steps per episode


def digest(snaps, *arrays):
    """sha256 over every snapshot field (fields_differing's view of a snapshot: the fields' bytes, no padding) and the
    arrays' values as int64 -- the form in which tests/golden/live_reference.json keeps runs of the real engine."""
    h = hashlib.sha256()
    for f in snaps.dtype.names:
        h.update(np.ascontiguousarray(snaps[f]).tobytes())
    for x in arrays:
        h.update(np.asarray(x, np.int64).tobytes())
    return h.hexdigest()


def live_record(gametype):
    """The live runs below as the real engine played them (tests/golden/make_live_golden.py): for a box without oracle/_ref."""
    with open(os.path.join(GOLDEN, "live_reference.json")) as f:
        return json.load(f)[gametype]


def live_random_runs(O, gametype):
    """test_oracle_vs_reference_live's lock-step random rollouts: (action set, OracleEnv, key table, actions), in order."""
    rng = np.random.default_rng(sum(map(ord, gametype)))
    for aset, T in ((1, 12000), (0, 6000)):
        o = O.OracleEnv(gametype, action_set=aset)
        keys = np.array(o.action_keys(), np.uint8)
        yield aset, o, keys, rng.integers(0, len(keys), T).astype(np.uint8)


def live_kill_runs(O, gametype, T=40000):
    """test_oracle_vs_reference_live_kills' runs: (policy, OracleEnv, key table, actions), in order."""
    rng = np.random.default_rng(1000 + sum(map(ord, gametype)))
    for policy in ("hunter", "charger"):
        o = O.OracleEnv(gametype, action_set=1)
        keys = np.array(o.action_keys(), np.uint8)
        if policy == "hunter":  # closed loop (nothing else aims the ship in a youturn game), played on a second oracle env
            acts = aimed_hunter_actions(O.OracleEnv(gametype, action_set=1), T, rng)
        else:
            acts = open_loop_actions(policy, T, len(keys), rng, phase=int(rng.integers(0, 96)))
        yield policy, o, keys, acts


@pytest.mark.parametrize("gametype", ["youturn", "autoturn", "test-youturn", "test-autoturn"])
def test_oracle_vs_reference_live(oracle_mod, gametype):
    """Lock-step random rollouts, every field bit-exact: against the real engine where oracle/_ref exists, elsewhere against
    the digests of the same runs of it (tests/golden/live_reference.json)."""
    O = oracle_mod
    rec = None if O.have_ref() else live_record(gametype)
    shaped = gametype in ("youturn", "autoturn")
    for aset, o, keys, acts in live_random_runs(O, gametype):
        oo = o.replay(acts)
        if rec is not None:
            assert digest(oo["snaps"], oo["done"], oo["reward"]) == rec["random_aset%d" % aset], (gametype, aset)
            continue
        rr = O.RefGame(gametype).replay(keys[acts])
        assert not fields_differing(oo["snaps"], rr["snaps"]), (gametype, aset)
        assert np.array_equal(oo["done"], rr["done"])
        assert np.array_equal(oo["reward"], shaped_reward(rr["eng_reward"], rr["snaps"]["vlner"], shaped))
    o = O.OracleEnv(gametype)
    if rec is not None:
        assert o.rollout(500000, 11) == rec["rollout"] and digest(o.snapshot()) == rec["rollout_snapshot"]
        return
    r = O.RefGame(gametype)
    assert o.rollout(500000, 11) == r.rollout(500000, 11)
    assert o.snapshot().tobytes() == r.snapshot().tobytes()


@pytest.mark.parametrize("gametype", ["youturn", "autoturn", "test-youturn", "test-autoturn"])
def test_oracle_vs_reference_live_kills(oracle_mod, gametype):
    """The live check on the paths random play does not reach: the vlner state machine, destroy, the fortress's respawn,
    shell and hexagon deaths -- 40 000 hunter + 40 000 charger steps per preset (7.5 episodes each, new Game at game over)
    through the REAL engine (oracle/_ref; elsewhere the digests of the same runs of it, tests/golden/live_reference.json)
    and through the C restatement, every snapshot field of every tick bit-identical, wrapper rewards (ENV:233-244) included."""
    O = oracle_mod
    rec = None if O.have_ref() else live_record(gametype)
    shaped = gametype in ("youturn", "autoturn")
    T = 40000
    for policy, o, keys, acts in live_kill_runs(O, gametype, T):
        oo = o.replay(acts, want_obs=False, max_resets=16)
        if rec is not None:
            assert digest(oo["snaps"], oo["done"], oo["reward"]) == rec["kills_" + policy], (gametype, policy)
            snaps, done, kills = oo["snaps"], oo["done"], rec["kills_%s_engine_rewards" % policy]
        else:
            rr = O.RefGame(gametype).replay(keys[acts])
            assert not fields_differing(oo["snaps"], rr["snaps"]), (gametype, policy)
            assert np.array_equal(oo["done"], rr["done"])
            assert np.array_equal(oo["reward"], shaped_reward(rr["eng_reward"], rr["snaps"]["vlner"], shaped))
            snaps, done, kills = rr["snaps"], rr["done"], int((np.asarray(rr["eng_reward"]) > 0).sum())
        assert oo["done"].sum() == T // 5295
        st = snaps["stats"]
        ends = np.flatnonzero(done)
        # per-episode counters (a new Game zeroes them): summed over the finished episodes, plus the running one
        tot = st[ends].sum(axis=0) + st[-1]
        if policy == "hunter":
            # stats: 4 resets, 5 destroyed, 11 vlner increments, 12 max vlner (SRC/game.hh:29-43)
            assert tot[5] >= 20 and tot[4] >= 20 and tot[11] >= 400 and st[:, 12].max() >= 11, (gametype, tot)
            assert oo["info"].sum() == kills >= 20
        else:
            # 0 big-hex, 1 small-hex, 2 shell deaths, 3 ship deaths (autoturn ships charge INTO the small hexagon)
            assert tot[0] + tot[1] >= 100 and tot[0] >= 1 and tot[1] >= 1 and tot[2] >= 1 and tot[3] == tot[:3].sum(), (gametype, tot)


@pytest.mark.parametrize("gametype", ["youturn", "autoturn"])
def test_vec_oracle_lanes_are_single_envs(oracle_mod, gametype):
    """OracleVecEnv hands lane i a copy of ONE libc stream advanced lane by lane (O(n * stride) to create instead of seeding
    every lane anew and skipping spawn_skip + i * spawn_stride spawns: 65 536 lanes in a second instead of minutes).  Lane i
    must be OracleEnv(spawn_skip = spawn_skip + i * spawn_stride): same first spawn, same game over 400 random steps
    (ship deaths draw further spawns from the lane's own copy), same snapshot."""
    O = oracle_mod
    n, skip, stride, T = 24, 2, 3, 400
    rng = np.random.default_rng(3)
    v = O.OracleVecEnv(gametype, n, spawn_skip=skip, spawn_stride=stride)
    n_act = 5 if gametype == "youturn" else 3
    acts = np.where(rng.random((T, n)) < 0.5, 2, rng.integers(0, n_act, (T, n))).astype(np.int32)  # (thrust: deaths, respawns)
    ob0 = v.reset()
    outs = [v.step(acts[t]) for t in range(T)]
    snaps = v.snapshots()
    for i in (0, 1, 5, 23):
        e = O.OracleEnv(gametype, spawn_skip=skip + i * stride)
        assert np.array_equal(e.reset(), ob0[i])
        for t in range(T):
            o, r, d, info = e.step(int(acts[t, i]))
            assert np.array_equal(o, outs[t][0][i]) and r == outs[t][1][i] and bool(d) == bool(outs[t][2][i]), (i, t)
            if d:
                e.reset()
        assert e.snapshot().tobytes() == snaps[i].tobytes(), i
    assert int(snaps["stats"][:, 3].sum()) > 0  # ships died: the respawn draws were exercised

