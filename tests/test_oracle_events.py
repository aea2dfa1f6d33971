"""The oracle's event word (oracle/sf_oracle.c: add_event at every call site of the reference's Game::addEvent, and the
project's two own bits), pinned on the CPU before any device word is held to it (tests/test_gpu_event_words.py):

  * on the recorded runs of the REAL engine -- the nine of tests/golden/getters/*.npz (the `events` getter per tick) and the
    three of tests/golden/telemetry/dumps.npz (the strings in Game.dump()) --, replayed through OracleEnv from the run's
    `keys`: every tick the same set of game events; the key names are the key-state changes of `keys`, a subset of the
    strings the reference logged (it logs every press / release CALL); missile-left where the recorded missedShots counts,
    game-over where the recording's is_game_over holds;
  * against the real engine itself (oracle/_ref/libsfref.so, skipped where it is not built) on CONSTRUCTED states -- the two
    fuzzers of tests/lockstep.py at 256 lanes each and every kind of eventcases.MULTI, both game types, 8 ticks of the same
    random keys --: every tick the same set of strings and the same state.  The recordings have no tick with more than one
    hit; these do (asserted).

The oracle reports NAMES from an enumeration of its own order; the comparison with the device goes through
spacefortress_amd._lib.EVENT_NAMES, so the last test pins that the two name sets are one."""
import glob
import json
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN
from eventcases import MULTI, MULTI_KINDS, multi_event_lane
from lockstep import fuzz_crowded, fuzz_sparse, n_actions
from sfcompare import compare_state, snapshots_to_fields

GETTERS = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, "getters", "*.npz")))
DUMPS = ["autoturn_destroy", "youturn_deaths", "youturn_rapid_fire"]
KEY_BITS = ((1, "fire"), (2, "thrust"), (4, "left"), (8, "right"))
# every string Game::addEvent is given but the eight key strings (SRC/game.cpp:155,169,186,202,342,348,363,371,381,385,393,417)
GAME_STRINGS = {"ship-respawn", "fortress-fired", "missile-fired", "fortress-respawn", "explode-bighex", "explode-smallhex",
                "hit-fortress", "vlner-increased", "fortress-destroyed", "vlner-reset", "hit-dead-fortress", "shell-hit-ship"}
SEEN = {}  # run -> the game strings the oracle reported on it (filled by the recorded-run tests, read by the census below)


def _is_key(name):
    return name.startswith(("press-", "release-"))


def _key_changes(keys, prev, youturn):
    want = set()
    for bit, nm in KEY_BITS[:4 if youturn else 2]:
        if (keys & bit) and not (prev & bit):
            want.add("press-" + nm)
        if not (keys & bit) and (prev & bit):
            want.add("release-" + nm)
    return want


def _replay(O, name, ref_sets, missed=None, over=None):
    """The run `name` through OracleEnv at engine level; ref_sets[t]: the reference's strings of tick t."""
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    meta = json.loads(str(z["meta"]))
    env = O.OracleEnv(meta["gametype"], action_set=meta["action_set"], seed=meta["seed"], spawn_skip=meta["spawn_skip"])
    own = set(O.OWN_EVENT_NAMES)
    prev, seen, prev_missed = 0, set(), 0
    assert len(ref_sets) == len(z["keys"])
    for t, keys in enumerate(z["keys"].tolist()):
        env.apply_keys(keys, env.youturn)
        env.step_one_tick(34)
        got = env.event_names(engine=True)
        ref = ref_sets[t]
        game = {e for e in got if not _is_key(e) and e not in own}
        assert game == {e for e in ref if not _is_key(e)}, (name, t, sorted(got), sorted(ref))
        keys_got = {e for e in got if _is_key(e)}
        assert keys_got == _key_changes(keys, prev, env.youturn), (name, t, sorted(keys_got), keys, prev)
        assert keys_got <= ref, (name, t)  # the reference logged those calls too (and the ones that changed nothing)
        if missed is not None:  # the project's two bits, against what the real engine recorded beside its strings
            assert ("missile-left" in got) == (missed[t] > prev_missed), (name, t)
            prev_missed = missed[t]
        assert ("game-over" in got) == bool(z["done"][t] if over is None else over[t]), (name, t)
        assert env.is_game_over() == ("game-over" in got)
        prev = keys
        seen |= game
        if env.is_game_over():
            env.new_game()
            prev, prev_missed = 0, 0
    SEEN[name] = seen
    return seen


@pytest.mark.parametrize("name", GETTERS)
def test_recorded_getter_runs(oracle_mod, name):
    assert len(GETTERS) == 9
    g = np.load(os.path.join(GOLDEN, "getters", name + ".npz"))
    ref = [set(e.split(",")) - {""} for e in g["events"].tolist()]
    _replay(oracle_mod, name, ref, missed=g["stats_i"][:, 6], over=g["game_over"])


@pytest.mark.parametrize("name", DUMPS)
def test_recorded_dump_runs(oracle_mod, name):
    dumps = np.load(os.path.join(GOLDEN, "telemetry", "dumps.npz"))[name]
    ref = [set(re.findall(r'"([a-z\-]+)"', d.decode())) for d in dumps[1:]]
    seen = _replay(oracle_mod, name, ref)
    if name == "autoturn_destroy":
        assert {"missile-fired", "hit-fortress", "vlner-increased", "fortress-destroyed"} <= seen
    if name == "youturn_deaths":
        assert {"explode-bighex", "ship-respawn", "fortress-fired"} <= seen


def test_the_recorded_runs_together_show_every_game_string(oracle_mod):
    for name in GETTERS:
        if name not in SEEN:  # (run alone, or in another order: replay what is missing)
            g = np.load(os.path.join(GOLDEN, "getters", name + ".npz"))
            _replay(oracle_mod, name, [set(e.split(",")) - {""} for e in g["events"].tolist()])
    seen = set().union(*(SEEN[n] for n in GETTERS))
    assert seen == GAME_STRINGS, sorted(GAME_STRINGS - seen)


# ---------------------------------------------------------------- the real engine on constructed states

def _multi_states(O, gametype, rng):
    """Every kind of MULTI eight times over a fuzzed batch (the fuzzed rest of the lane stays: shells, timers, key flags)."""
    n = 8 * len(MULTI_KINDS)
    base, pv = fuzz_sparse(O, gametype, n, rng)
    for i in range(n):
        multi_event_lane(base, i, MULTI_KINDS[i % len(MULTI_KINDS)], rng)
    return base, base["vlner"].astype(np.int32)


@pytest.mark.parametrize("what", ["crowded", "sparse", "multi"])
@pytest.mark.parametrize("gametype", ["youturn", "autoturn"])
def test_constructed_states_against_the_real_engine(oracle_mod, gametype, what):
    O = oracle_mod
    if not O.have_ref():
        pytest.skip("oracle/_ref/libsfref.so is not built here (the reference's sources are not on this machine)")
    rng = np.random.default_rng({"crowded": 3100, "sparse": 3200, "multi": 3300}[what] + len(gametype))
    if what == "multi":
        base, pv = _multi_states(O, gametype, rng)
    else:
        base, pv = (fuzz_crowded if what == "crowded" else fuzz_sparse)(O, gametype, 256, rng)
        base["time"][:6] = 180000 - 34 * np.array([1, 2, 3, 4, 8, 9])  # games that end inside the run, and at its end
    n, T = len(base), 8
    youturn = gametype == "youturn"
    key_of = [0, 1, 2, 4, 8][:n_actions(gametype)]
    acts = rng.integers(0, n_actions(gametype), (T, n))
    own = set(O.OWN_EVENT_NAMES)
    seen, several, most_hits = set(), 0, 0
    for i in range(n):
        ref, orc = O.RefGame(gametype), O.OracleEnv(gametype)
        ref.load_snapshot(base[i])
        orc.load_snapshot(base[i], pv[i])
        prev_missed = base["stats"][i, 6]
        for t in range(T):
            keys = key_of[acts[t, i]]
            ref.apply_keys(keys, youturn)
            orc.apply_keys(keys, youturn)
            assert ref.step_one_tick(34) == orc.step_one_tick(34), (i, t)
            strings = re.findall(r'"([a-z\-]+)"', ref.dump().rsplit("[", 1)[1])
            got = orc.event_names(engine=True)
            assert {s for s in strings if not _is_key(s)} == {e for e in got if not _is_key(e) and e not in own}, (i, t, strings, sorted(got))
            assert {e for e in got if _is_key(e)} <= set(strings), (i, t)
            rs, os_ = ref.snapshot(), orc.snapshot()
            bad = compare_state(snapshots_to_fields(rs.reshape(1)), os_.reshape(1), shell_tol=0.0)
            assert not bad and rs["collisions"] == os_["collisions"], (i, t, bad)
            assert ("missile-left" in got) == (rs["stats"][6] > prev_missed), (i, t)  # (the REFERENCE's missedShots)
            prev_missed = rs["stats"][6]
            hits = sum(s in ("hit-fortress", "hit-dead-fortress") for s in strings)
            several += hits >= 2
            most_hits = max(most_hits, hits)
            seen |= set(strings)
            over = ref.is_game_over()
            assert over == orc.is_game_over() == ("game-over" in got), (i, t)
            if over:
                ref.new_game()
                orc.new_game()
                prev_missed = 0
    # what the recordings do not have: ticks with several hits -- and with them every string of the missile walk
    assert several > 0 and most_hits >= (3 if what != "sparse" else 2), (several, most_hits)
    assert {"hit-fortress", "vlner-increased", "vlner-reset", "fortress-destroyed", "hit-dead-fortress"} <= seen, sorted(seen)
    if what == "multi":
        assert set(MULTI) == set(MULTI_KINDS) and n == 8 * len(MULTI)


# ---------------------------------------------------------------- the scenarios the GPU tests play, with the oracle alone

@pytest.mark.parametrize("fuzzer", ["crowded", "sparse"])
@pytest.mark.parametrize("gametype", ["youturn", "autoturn"])
def test_the_mixed_batches_hold_what_the_gpu_tests_say_they_hold(oracle_mod, gametype, fuzzer):
    """The seeds of eventcases.mixed_batch under the given actions: every bit, every same-tick combination, games ending
    on each of the first three ticks in every tile (eventcases.mixed_census) -- checked here before a device plays them."""
    from spacefortress_amd._lib import EVENT_NAMES

    from eventcases import MIXED_MULTI_LANES, mixed_batch, mixed_census
    from lockstep import oracle_trace

    base, pv, acts = mixed_batch(oracle_mod, gametype, fuzzer)
    assert len(base) == 200 and acts.shape == (12, 200)
    trace = oracle_trace(oracle_mod, gametype, base, pv, acts)
    mixed_census(gametype, base, trace, {nm: b for b, nm in EVENT_NAMES.items()})
    # the constructed lanes, whatever is played: lane j is kind j % 10, its first tick's missile bits are the kind's
    want = {"inc_then_resets": {"hit-fortress", "vlner-increased", "vlner-reset"},
            "inc_destroy_dead": {"hit-fortress", "vlner-increased", "fortress-destroyed", "hit-dead-fortress"},
            "inc_destroy": {"hit-fortress", "vlner-increased", "fortress-destroyed"},
            "resets_only": {"hit-fortress", "vlner-reset"},
            "reset_miss_reset": {"hit-fortress", "vlner-reset", "missile-left"},
            "dead_hits_and_miss": {"hit-dead-fortress", "missile-left"},
            "miss_destroy_miss": {"hit-fortress", "fortress-destroyed", "missile-left"},
            "four_resets": {"hit-fortress", "vlner-reset"},
            "one_miss": {"missile-left"},
            "hit_and_leave_same_slot_order": {"hit-fortress", "vlner-increased", "missile-left"}}
    assert sorted(want) == sorted(MULTI)
    walk = {"hit-fortress", "vlner-increased", "vlner-reset", "fortress-destroyed", "hit-dead-fortress", "missile-left"}
    for j, i in enumerate(MIXED_MULTI_LANES):
        got = oracle_mod.names_of_sf_word(trace[0][5][i]) & walk
        assert got == want[MULTI_KINDS[j % len(MULTI_KINDS)]], (i, MULTI_KINDS[j % len(MULTI_KINDS)], sorted(got))


def test_the_oracles_names_are_the_packages_names(oracle_mod):
    from spacefortress_amd._lib import EVENT_NAMES

    names = oracle_mod.event_names()
    assert len(names) == len(set(names)) == 22 and sorted(names) == sorted(EVENT_NAMES.values())
    assert set(names) == GAME_STRINGS | set(oracle_mod.KEY_EVENT_NAMES) | set(oracle_mod.OWN_EVENT_NAMES)
    # one bit at a time through the translation, and all at once
    for i, nm in enumerate(names):
        w = int(oracle_mod.to_sf_events(np.uint32(1 << i)))
        assert EVENT_NAMES[w] == nm and oracle_mod.names_of_sf_word(w) == {nm}
    assert int(oracle_mod.to_sf_events(np.uint32((1 << 22) - 1))) == sum(EVENT_NAMES)
    # the word is the last tick's: cleared at the start of the next one
    env = oracle_mod.OracleEnv("youturn")
    env.step(1)
    assert env.event_names() == {"press-fire", "missile-fired"}
    env.step(1)
    assert env.event_names() == set()
    env.step(0)
    assert env.event_names() == {"release-fire"}


def test_a_finishing_ticks_word_is_its_own(oracle_mod):
    """OracleVecEnv resets a finished env inside step(): the word it reports is the finishing tick's, game-over included."""
    O = oracle_mod
    v = O.OracleVecEnv("autoturn", 3)
    s = v.snapshots()
    s["time"] = [180000 - 34, 180000 - 68, 0]
    v.load_snapshots(s)
    _, _, done, _ = v.step([1, 1, 0])
    w = v.events()
    assert done.tolist() == [True, False, False] and w.dtype == np.uint32
    assert [sorted(O.names_of_sf_word(x)) for x in w] == [["game-over", "missile-fired", "press-fire"], ["missile-fired", "press-fire"], []]
    assert v.snapshots()["time"][0] == 0  # (the new game)
    _, _, done, _ = v.step([0, 0, 0])
    assert done.tolist() == [False, True, False]
    assert [sorted(O.names_of_sf_word(x)) for x in v.events()] == [[], ["game-over", "release-fire"], []]
