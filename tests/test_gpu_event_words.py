"""The per-tick event word (sf_set_event_output / SFVecEnv.enable_events, sfmi.h SF_EV_*) against the CPU oracle's, per lane
and per tick, in every launch form.  The oracle's word is the reference's strings restated at their call sites -- the missile
bits set in the slot-order walk, not derived from counts as the kernel derives them -- and is itself held to the real engine
by tests/test_oracle_events.py.  Every scenario asserts from the ORACLE's side that what it is about happened.

  * a mixed batch (eventcases.mixed_batch: fuzzed states, lanes with several missile events in one tick astride a tile
    boundary and in the partial last tile, games ending inside the run): 200 envs, 12 ticks, both game types, both fuzzers,
    the four launches of lockstep.LAUNCHES;
  * one tile in which every lane owns another number of hitting and leaving missiles, rotated by 0, 1 and 37 lanes;
  * the 200-lane state tiled to 65 736 envs (past the split launches), 3 ticks: the first 200 lanes against the oracle,
    every copy against its original;
  * single bits at their thresholds (eventcases.edge_lanes), every previous key state against every action;
  * step_repeat (the OR of the played ticks' words, stopping at a finishing tick) and step_where (held lanes read 0);
  * events on against events off: the same outputs and state, byte for byte, in every launch form."""
import numpy as np
import pytest

from eventcases import MIXED_ENDING, edge_lanes, key_edge_lanes, mixed_batch, mixed_census, owners_tile
from lockstep import (LAUNCHES, check_ticks, every, event_names, make_env, n_actions, oracle_trace, play, run_lockstep, same_bytes,
                      sfa)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GAMETYPES = ["youturn", "autoturn"]
FUZZERS = ["crowded", "sparse"]


def _bit_of():
    from spacefortress_amd._lib import EVENT_NAMES

    return {nm: b for b, nm in EVENT_NAMES.items()}


def _rule(launch):
    return "close_f64" if LAUNCHES[launch][1] else "close_f32"  # (the rows are other tests' subject: sfcompare's tolerances)


# ---------------------------------------------------------------- 1. the mixed batch, every launch form

@pytest.mark.parametrize("launch", list(LAUNCHES))
@pytest.mark.parametrize("fuzzer", FUZZERS)
@pytest.mark.parametrize("gametype", GAMETYPES)
def test_mixed_batch_in_every_launch_form(sfa, oracle_mod, gametype, fuzzer, launch):
    base, pv, acts = mixed_batch(oracle_mod, gametype, fuzzer)
    T = len(acts)
    trace, ticks = run_lockstep(sfa, oracle_mod, gametype, base, pv, acts, launch, every(T if launch == "fused" else 4),
                                _rule(launch), events=True)
    assert ticks.events.shape == (T, 200)
    # from the oracle's side, of what the batch played (a sampled launch: of what its lanes drew)
    mixed_census(gametype, base, trace, _bit_of())


# ---------------------------------------------------------------- 2. owners

@pytest.mark.parametrize("rot", [0, 1, 37])
@pytest.mark.parametrize("gametype", GAMETYPES)
def test_every_lane_of_a_tile_owns_another_number_of_missiles(sfa, oracle_mod, gametype, rot):
    """The missile wave ORs a slot's hit / out bit into its OWNER's word: 0..6 hitting and 0..6 leaving missiles per lane,
    permuted over the tile and rotated -- a word kept under the lane instead of the owner shows."""
    base, pv, pat = owners_tile(oracle_mod, gametype, rot)
    acts = np.zeros((2, 64), np.uint8)
    trace = oracle_trace(oracle_mod, gametype, base, pv, acts)
    bit = _bit_of()
    w = trace[0][5]
    assert np.array_equal((w & (bit["hit-fortress"] | bit["hit-dead-fortress"])) != 0, pat[:, 0] > 0)
    assert np.array_equal((w & bit["missile-left"]) != 0, pat[:, 1] > 0)
    assert len({tuple(p) for p in pat}) == 49 and len(set(w.tolist())) >= 12 and (base["missile_alive"].sum(1) == pat.sum(1)).all()
    assert (trace[0][4]["missile_alive"] == 0).all()  # every missile went in the compared tick
    run_lockstep(sfa, None, gametype, base, pv, acts, "split", every(1), "f32_bits", trace=trace, events=True)


# ---------------------------------------------------------------- 3. beyond one launch shape

@pytest.mark.parametrize("gametype", GAMETYPES)
def test_the_mixed_batch_tiled_past_the_split_launches(sfa, oracle_mod, gametype):
    n, T = 65536 + 200, 3
    small, pv_s, acts_s = mixed_batch(oracle_mod, gametype, "crowded", ticks=T)
    base, pv, acts = np.resize(small, n), np.resize(pv_s, n), np.stack([np.resize(a, n) for a in acts_s])
    first = np.arange(200)
    trace = oracle_trace(oracle_mod, gametype, small, pv_s, acts_s)
    env = make_env(sfa, gametype, base, pv)
    ticks = play(env, acts, "step", None, events=True)
    env.close()
    check_ticks(ticks, trace, "close_f32", first)
    words = np.array([tr[5] for tr in trace])
    assert len({int(x) for x in words.reshape(-1)}) > 30 and np.array([tr[2] for tr in trace]).any(1).all()  # (not idle; a game ends on every tick)
    want = words[:, np.arange(n) % 200]  # every copy its original
    bad = np.argwhere(ticks.events != want)
    assert bad.size == 0, (bad[:5].tolist(), [(sorted(event_names(ticks.events[t, i])), sorted(event_names(want[t, i]))) for t, i in bad[:5]])


# ---------------------------------------------------------------- 4. edges of single bits

@pytest.mark.parametrize("launch", ["split", "f64"])
@pytest.mark.parametrize("gametype", GAMETYPES)
def test_single_bits_at_their_thresholds(sfa, oracle_mod, gametype, launch):
    base, pv, expect = edge_lanes(oracle_mod, gametype)
    acts = np.zeros((1, len(base)), np.uint8)
    trace = oracle_trace(oracle_mod, gametype, base, pv, acts)
    bit = _bit_of()
    for i, name, want in expect:
        assert bool(trace[0][5][i] & bit[name]) == want, (i, name, want, sorted(event_names(trace[0][5][i])))
    assert {nm for _, nm, _ in expect} == {"missile-left", "game-over", "fortress-respawn", "ship-respawn", "explode-bighex",
                                           "explode-smallhex", "fortress-fired"}
    run_lockstep(sfa, None, gametype, base, pv, acts, launch, every(1), _rule(launch), trace=trace, events=True)


@pytest.mark.parametrize("gametype", GAMETYPES)
def test_every_previous_key_state_against_every_action(sfa, oracle_mod, gametype):
    base, acts, lanes = key_edge_lanes(oracle_mod, gametype)
    assert lanes == (80 if gametype == "youturn" else 12)
    pv = np.zeros(len(base), np.int32)
    trace = oracle_trace(oracle_mod, gametype, base, pv, acts)
    bit = _bit_of()
    na, keys_of = n_actions(gametype), [0, 1, 2, 4, 8]  # action set 1: NOOP, FIRE, THRUST, LEFT, RIGHT (ENV:71-78,84-89)
    for i in range(lanes):  # the state changes, computed here from the flags and the action
        prev, now, want = i // na, keys_of[i % na], 0
        for b, nm in enumerate(("fire", "thrust", "left", "right")[:4 if gametype == "youturn" else 2]):
            was, is_ = (prev >> b) & 1, (now >> b) & 1
            want |= bit["press-" + nm] if is_ and not was else bit["release-" + nm] if was and not is_ else 0
        assert int(trace[0][5][i]) & 0xFF == want, (i, prev, now, sorted(event_names(trace[0][5][i])))
    run_lockstep(sfa, None, gametype, base, pv, acts, "split", every(1), "close_f32", trace=trace, events=True)


# ---------------------------------------------------------------- 5. action repeat and the masked step

@pytest.mark.parametrize("fuzzer", FUZZERS)
@pytest.mark.parametrize("gametype", GAMETYPES)
def test_step_repeat_ors_the_played_ticks_words(sfa, oracle_mod, gametype, fuzzer):
    """step_repeat(actions, 3): an env's word is the OR of the oracle's words of the ticks it played -- all three, or up to
    and including the tick that finished its game (the new game is not played on)."""
    base, pv, acts = mixed_batch(oracle_mod, gametype, fuzzer)
    n = len(base)
    orc = oracle_mod.OracleVecEnv(gametype, n)
    orc.load_snapshots(base, pv)
    playing, want, played = np.ones(n, bool), np.zeros(n, np.uint32), np.zeros(n, np.int64)
    ended_at = {}
    for k in range(3):
        _, _, done, _ = orc.step(acts[0].astype(np.int32))
        want |= np.where(playing, orc.events(), np.uint32(0)).astype(np.uint32)
        played += playing
        for i in np.flatnonzero(done & playing):
            ended_at[int(i)] = k + 1
        playing &= ~done
    assert ended_at == MIXED_ENDING and set(ended_at.values()) == {1, 2, 3}  # lanes that finish on each tick of the window
    bit = _bit_of()
    assert all(want[i] & bit["game-over"] for i in ended_at) and not (want[playing] & bit["game-over"]).any()
    # (lanes whose word is not any single tick's: the OR is of several)
    env = make_env(sfa, gametype, base, pv, events=True)
    out = env.step_repeat(torch.from_numpy(acts[0].copy()).to(env.device), 3)
    got = env.events.cpu().numpy().view(np.uint32)
    ticks_played = env.last_ticks.cpu().numpy()
    done = out[2].cpu().numpy().astype(bool)
    env.close()
    assert np.array_equal(ticks_played, played) and np.array_equal(done, ~playing)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:5].tolist(), [(sorted(event_names(got[i])), sorted(event_names(want[i]))) for i in bad[:5]])


@pytest.mark.parametrize("gametype", GAMETYPES)
def test_step_where_active_lanes_have_the_oracles_word_and_held_lanes_zero(sfa, oracle_mod, gametype):
    base, pv, acts = mixed_batch(oracle_mod, gametype, "sparse")
    n = len(base)
    rng = np.random.default_rng(77)
    active = rng.random(n) < 0.6
    active[[59, 60, 63, 64, 190, 199]] = [True, False, True, False, True, False]  # multi-event lanes on both sides, both ends of a tile
    orc = oracle_mod.OracleVecEnv(gametype, n)
    orc.load_snapshots(base, pv)
    orc.step(acts[0].astype(np.int32))
    want = np.where(active, orc.events(), np.uint32(0)).astype(np.uint32)
    assert (orc.events()[~active] != 0).sum() > 20 and (want != 0).sum() > 50  # held lanes that WOULD have had events
    env = make_env(sfa, gametype, base, pv, events=True)
    env.events.fill_(-1)  # (a held lane's word is written, not left)
    env.step_where(torch.from_numpy(acts[0].copy()).to(env.device), torch.from_numpy(active).to(env.device))
    got = env.events.cpu().numpy().view(np.uint32)
    env.close()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (bad[:5].tolist(), [(sorted(event_names(got[i])), sorted(event_names(want[i]))) for i in bad[:5]])


# ---------------------------------------------------------------- 6. switching the words on changes nothing else

@pytest.mark.parametrize("launch", list(LAUNCHES))
@pytest.mark.parametrize("gametype", GAMETYPES)
def test_events_on_and_events_off_play_the_same_bytes(sfa, oracle_mod, gametype, launch):
    """What lets the scenario files carry the word as one more compared column: the same constructed state and actions with
    events on and off give the same outputs and the same state, byte for byte (sf_launch_step picks the instantiation without
    looking at the event pointer: profiles/event_tests.md)."""
    base, pv, acts = mixed_batch(oracle_mod, gametype, "sparse")
    mode, f64 = LAUNCHES[launch]
    T = len(acts)
    runs = []
    for on in (False, True):
        env = make_env(sfa, gametype, base, pv, f64=f64)
        if mode == "sampled":
            env.seed_actions(4242)
        runs.append(play(env, acts, mode, every(T if mode == "fused" else 4), check_state=True, events=on))
        env.close()
    off, on = runs
    assert off.events is None and on.events is not None and (on.events != 0).sum() > 100
    assert np.array_equal(off.played, on.played)
    same_bytes(off, on)
