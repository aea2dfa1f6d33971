"""What a tick's missile events and shells do to an env, where the step kernel does not walk them in the reference's order:
the missile events are counted and resolved in closed form (spacefortress_amd/csrc/sf_events.h; the host side of that is
tests/test_event_replay_model.py); the shells' outcomes depend on the slot order only through "the lowest colliding slot
leaves with the ship", which these scenarios hold any walk of the slots to (written with a walk per lane instead of per slot,
measured and not kept: profiles/step_outcomes.md).  In lock-step with the CPU oracle, through the harness of
tests/lockstep.py:

  * observation rows as float32 BIT PATTERNS, reward / done / info exactly, the state through sfcompare.compare_state, the
    event word of every lane and tick (sfmi.h SF_EV_*) bit for bit;
  * every scenario asserts, from the ORACLE's trace, that its event happened in the compared tick.

Shapes: 64 and 256 envs (one tile; four tiles in one workgroup), youturn and autoturn, stepped by split launches; the same
scenarios at 64 envs through a float64-observation batch (the non-split instantiation), step_sampled, and a fused rollout of
four ticks against four steps; three ticks of constructed states at 16 448, 32 832, 65 536 (128 and 256 envs per workgroup,
the latter with the staggered start) and 65 600 envs (non-split) on a fixed sample of lanes."""
import numpy as np
import pytest

from lockstep import (ST_DEATHS, ST_DESTROYED, ST_INCS, ST_MISSED, ST_RESETS, ST_SHELL, ST_SHOTS, every, fresh, fused_equals_steps,
                      fuzz_sparse, missile_table, n_actions, oracle_trace, run_lockstep, sfa)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GAMETYPES = ["youturn", "autoturn"]
SMALL = [64, 256]
OTHER = ["f64", "sampled", "fused"]
T = 4  # ticks: the scenario's tick (every lane plays NOOP), then random play


def _acts(rng, gametype, n):
    acts = rng.integers(0, n_actions(gametype), (T, n)).astype(np.uint8)
    acts[0] = 0
    return acts


# ---------------------------------------------------------------- 1. missile events

# (fort_vuln_timer, vlner) -> what n >= 3 hits in one tick do: (incs, resets, destroyed)
CELLS = [((300, 9), lambda n: (1, n - 1, 0)),   # increment to 10, then resets
         ((300, 10), lambda n: (1, 0, 1)),      # increment to 11, the second hit destroys, the rest meet a dead fortress
         ((300, 11), lambda n: (1, 0, 1)),
         ((100, 10), lambda n: (0, n, 0)),      # inside the window below the threshold: resets only
         ((100, 11), lambda n: (0, 0, 1)),      # the first hit destroys
         ((249, 12), lambda n: (0, 0, 1))]      # (the window's last millisecond)


def _n_hits(i):
    return 3 + (i // 16) % 3  # 3, 4 and 5 hits, by group of 16 lanes


def _setup_missile_events(O, gametype, n):
    """Lane i % 16: 0..5 the cells of CELLS under 3, 4 or 5 hits; 6, 7, 8 two hits and a miss, the miss in the lowest, the
    middle, the highest slot; 9 three hits on a dead fortress; 10 an increment to vlner 11 and the destroying hit; 11 the same
    with a miss between them and a third hit behind; 12 a destroying hit between two misses; 13 nothing; 14 hit, miss, hit,
    miss, hit, miss; 15 one miss."""
    rng = np.random.default_rng(1100 + n + len(gametype))
    base = fresh(O, gametype, n)
    tab = missile_table()
    kind = np.arange(n) % 16

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
        k = int(kind[i])
        vt, vl, seq = 100, 5, ""
        if k < 6:
            (vt, vl), seq = CELLS[k][0], "h" * _n_hits(i)
        elif k in (6, 7, 8):
            vt, seq = 300, ("mhh", "hmh", "hhm")[k - 6]
        elif k == 9:
            seq = "hhh"
            base["fort_alive"][i] = 0
            base["fort_death_timer"][i] = 34
        elif k == 10:
            vt, vl, seq = 300, 10, "hh"
        elif k == 11:
            vt, vl, seq = 300, 10, "hmhh"
        elif k == 12:
            vl, seq = 12, "mhm"
        elif k == 14:
            seq = "hmhmhm"
        elif k == 15:
            seq = "m"
        base["fort_vuln_timer"][i], base["vlner"][i] = vt, vl
        slots = np.sort(rng.choice(20, len(seq), replace=False))
        for s, e in zip(slots, seq):
            put(i, int(s), e == "h")
    return base, base["vlner"].astype(np.int32), _acts(rng, gametype, n)


def _events_missile_events(base, trace, n):
    kind = np.arange(n) % 16
    d = trace[0][4]["stats"] - base["stats"]
    s1 = trace[0][4]
    got = d[:, [ST_INCS, ST_RESETS, ST_DESTROYED, ST_MISSED]]
    for i in range(n):
        k = int(kind[i])
        if k < 6:
            want = CELLS[k][1](_n_hits(i)) + (0,)
        else:
            want = {6: (1, 1, 0, 1), 7: (1, 1, 0, 1), 8: (1, 1, 0, 1), 9: (0, 0, 0, 0), 10: (1, 0, 1, 0), 11: (1, 0, 1, 1),
                    12: (0, 0, 1, 2), 13: (0, 0, 0, 0), 14: (0, 3, 0, 3), 15: (0, 0, 0, 1)}[k]
        assert tuple(got[i]) == want, (i, k, got[i].tolist(), want)
        assert s1["fort_alive"][i] == (0 if (want[2] or k == 9) else 1), (i, k)
    assert (s1["missile_alive"][base["missile_alive"] == 1] == 0).all()  # every missile of the scenario left in the compared tick
    assert (s1["vlner"][np.isin(kind, (6, 7, 8))] == 0).all()           # increment, then reset: wherever the miss stands
    assert (s1["fort_vuln_timer"][kind == 9] == 100 + 34).all()         # a dead fortress: the timer runs on
    assert (s1["fort_death_timer"][np.isin(kind, (10, 11, 12))] == 34).all()
    quiet = (kind == 10) & (d[:, ST_SHOTS] == 0)  # (a shot's penalty in the same tick takes the reward below 1: truncated to 0)
    assert quiet.any() and trace[0][1][quiet].min() > 0
    assert {3, 4, 5} <= {_n_hits(i) for i in range(n)}


@pytest.mark.parametrize("n", SMALL)
@pytest.mark.parametrize("gametype", GAMETYPES)
def test_missile_events_of_one_tick(sfa, oracle_mod, gametype, n):
    """Up to six events of one env in one tick -- several hits inside and outside the vulnerability window, misses among
    them, a dead fortress -- by split launches."""
    base, pv, acts = _setup_missile_events(oracle_mod, gametype, n)
    trace = oracle_trace(oracle_mod, gametype, base, pv, acts)
    _events_missile_events(base, trace, n)
    run_lockstep(sfa, None, gametype, base, pv, acts, "split", every(1), "f32_bits", trace=trace, events=True)


# ---------------------------------------------------------------- 2. shells

FLYING = {0: (0,), 1: (5,), 2: (19,), 3: (0, 7), 4: (3, 19), 5: (0, 1, 2), 6: (1, 4, 9, 13, 18)}
MANY = (0, 2, 5, 9, 10, 14, 17, 19)


def _setup_shells(O, gametype, n, lone=False):
    """Lane i % 16: 0..6 shells that fly on in the slots of FLYING; 7 two shells collide with a live ship (slots 2 and 11); 8 a
    colliding shell and a dead ship; 9 the fortress fires into slot 0, below a live shell in slot 3; 10 a shell kills the ship
    (slot 4), a higher one leaves the area (12); 11 the lower one leaves, the higher one kills; 12 eight shells, of which slot
    9 kills and slot 14 leaves; 13..15 none.  `lone`: only lane 37 of every tile has shells (slots 0, 6 and 19; 6 kills)."""
    rng = np.random.default_rng(1200 + n + len(gametype) + int(lone))
    base = fresh(O, gametype, n)
    kind = np.arange(n) % 16

    def fly(i, s):  # well inside the area, far from the ship and the fortress' line of fire
        base["shell_alive"][i, s] = 1
        base["shell_x"][i, s], base["shell_y"][i, s] = rng.uniform(200, 300), rng.uniform(180, 250)
        base["shell_vx"][i, s], base["shell_vy"][i, s] = rng.uniform(-6, 6, 2)

    def strike(i, s):  # on the ship after this tick's move (radius 13; a thrusting ship moves 0.3)
        base["shell_alive"][i, s] = 1
        base["shell_vx"][i, s], base["shell_vy"][i, s] = rng.uniform(-6, 6, 2)
        base["shell_x"][i, s] = base["ship_x"][i] - base["shell_vx"][i, s] + rng.uniform(-3, 3)
        base["shell_y"][i, s] = base["ship_y"][i] - base["shell_vy"][i, s] + rng.uniform(-3, 3)

    def leave(i, s):
        base["shell_alive"][i, s] = 1
        base["shell_x"][i, s], base["shell_y"][i, s] = 709.5, 300.0
        base["shell_vx"][i, s], base["shell_vy"][i, s] = 5.0, 0.5

    for i in range(n):
        k = int(kind[i])
        if lone:
            if i % 64 == 37:
                fly(i, 0), strike(i, 6), fly(i, 19)
            continue
        if k in FLYING:
            for s in FLYING[k]:
                fly(i, s)
        elif k == 7:
            strike(i, 2), strike(i, 11)
        elif k == 8:
            strike(i, int(rng.integers(0, 20)))
            base["ship_alive"][i] = 0
            base["ship_death_timer"][i] = 34 * 3
        elif k == 9:
            fly(i, 3)
            # the bearing of the ship is 5 degrees, sector 10 (a thrusting ship stays in it): the fortress keeps its aim and fires
            base["ship_y"][i] = 315.0 + 9.0
            base["fort_angle"][i] = base["fort_last_angle"][i] = 10
            base["fort_timer"][i] = 1000
        elif k == 10:
            strike(i, 4), leave(i, 12)
        elif k == 11:
            leave(i, 4), strike(i, 12)
        elif k == 12:
            for s in MANY:
                (strike if s == 9 else leave if s == 14 else fly)(i, s)
    return base, np.zeros(n, np.int32), _acts(rng, gametype, n)


def _events_shells(base, trace, n, lone=False):
    kind = np.arange(n) % 16
    d = trace[0][4]["stats"] - base["stats"]
    s1, sh0, sh1 = trace[0][4], base["shell_alive"], trace[0][4]["shell_alive"]
    if lone:
        me = np.arange(n) % 64 == 37
        assert (d[me, ST_SHELL] == 1).all() and (s1["ship_alive"][me] == 0).all()
        assert (sh1[me][:, [0, 6, 19]] == [1, 0, 1]).all() and (sh1[me].sum(1) == 2).all()
        assert (sh1[~me] == 0).all() and (d[~me, ST_SHELL] == 0).all()
        return
    fl = np.isin(kind, list(FLYING))
    assert np.array_equal(sh1[fl], sh0[fl]) and (d[fl, ST_SHELL] == 0).all() and (s1["ship_alive"][fl] == 1).all()
    assert {tuple(np.flatnonzero(r)) for r in sh0[fl]} == set(FLYING.values())
    k7 = kind == 7
    assert (d[k7, ST_SHELL] == 1).all() and (d[k7, ST_DEATHS] == 1).all() and (s1["ship_alive"][k7] == 0).all()
    assert (sh1[k7, 2] == 0).all() and (sh1[k7, 11] == 1).all()          # the lower slot goes, the other stays
    k8 = kind == 8
    assert (d[k8, ST_SHELL] == 0).all() and np.array_equal(sh1[k8], sh0[k8]) and (sh0[k8].sum(1) == 1).all()
    k9 = kind == 9
    assert (sh0[k9].sum(1) == 1).all() and (sh1[k9][:, [0, 3]] == 1).all() and (sh1[k9].sum(1) == 2).all()
    for k in (10, 11):
        m = kind == k
        assert (d[m, ST_SHELL] == 1).all() and (sh1[m].sum(1) == 0).all() and (s1["ship_alive"][m] == 0).all()
    k12 = kind == 12
    assert (d[k12, ST_SHELL] == 1).all() and (sh1[k12].sum(1) == len(MANY) - 2).all()
    assert (sh1[k12][:, [9, 14]] == 0).all()


@pytest.mark.parametrize("lone", [False, True])
@pytest.mark.parametrize("n", SMALL)
@pytest.mark.parametrize("gametype", GAMETYPES)
def test_shell_outcomes_of_one_tick(sfa, oracle_mod, gametype, n, lone):
    """Shells in low, high and many slots of a lane, two collisions in one tick, a collision with a dead ship, the new shell
    below a live one, a shell leaving as another kills -- and one lane with shells among 63 without -- by split launches."""
    base, pv, acts = _setup_shells(oracle_mod, gametype, n, lone)
    trace = oracle_trace(oracle_mod, gametype, base, pv, acts)
    _events_shells(base, trace, n, lone)
    run_lockstep(sfa, None, gametype, base, pv, acts, "split", every(1), "f32_bits", trace=trace, events=True)


# ---------------------------------------------------------------- 3. the same scenarios through the other launches

@pytest.mark.parametrize("mode", OTHER)
@pytest.mark.parametrize("what", ["missiles", "shells"])
@pytest.mark.parametrize("gametype", GAMETYPES)
def test_the_scenarios_through_the_other_launches(sfa, oracle_mod, gametype, what, mode):
    """64 envs through a float64-observation batch (the non-split instantiation), step_sampled (the lanes draw their own
    actions: the scenarios' events do not depend on them) and a fused rollout of four ticks, which must equal four steps."""
    O, n = oracle_mod, 64
    setup, events = (_setup_missile_events, _events_missile_events) if what == "missiles" else (_setup_shells, _events_shells)
    base, pv, acts = setup(O, gametype, n)
    # (rows rounded to float32 as bit patterns; the state after every tick, of a fused launch after the last)
    trace, _ = run_lockstep(sfa, O, gametype, base, pv, acts, mode, every(T if mode == "fused" else 1), "rounded_f32_bits",
                            events=True)
    events(base, trace, n)
    if mode == "fused":
        fused_equals_steps(sfa, gametype, base, pv, acts)


# ---------------------------------------------------------------- 4. the larger workgroups

def _setup_large(O, gametype, n):
    rng = np.random.default_rng(1300 + n + len(gametype))
    small, pv_s = fuzz_sparse(O, gametype, 512, rng)
    idx = np.arange(n) % 512
    base, pv = small[idx].copy(), pv_s[idx]
    acts = rng.integers(0, n_actions(gametype), (3, n)).astype(np.uint8)
    lanes = np.sort(np.concatenate([rng.choice(n - 64, 224, replace=False), n - 64 + rng.choice(64, 32, replace=False)]))
    return base, pv, acts, lanes


def _events_large(base, trace, lanes):
    prev, several = base["stats"][lanes], 0
    for tr in trace:
        d = tr[4]["stats"] - prev
        prev = tr[4]["stats"]
        several += int((d[:, [ST_INCS, ST_RESETS, ST_DESTROYED, ST_MISSED]].sum(1) >= 2).sum())
    assert several > 0                                                   # lanes with more than one missile event in a tick
    d = trace[-1][4]["stats"] - base["stats"][lanes]
    assert (d[:, [ST_SHELL, ST_RESETS, ST_MISSED]] > 0).any(0).all()
    assert (base["shell_alive"][lanes].sum(1) >= 4).any()


@pytest.mark.parametrize("n", [16448, 32832, 65536, 65600])
@pytest.mark.parametrize("gametype", GAMETYPES)
def test_three_ticks_of_constructed_states_at_the_larger_shapes(sfa, oracle_mod, gametype, n):
    """128 and 256 envs per workgroup, the split launch with the staggered start (65 536) and the smallest non-split plain
    launch (65 600): a seeded sample of 256 lanes against the oracle, the last tile's among them."""
    base, pv, acts, lanes = _setup_large(oracle_mod, gametype, n)
    trace, _ = run_lockstep(sfa, oracle_mod, gametype, base, pv, acts, "split", every(len(acts)), "rounded_f32_bits", lanes=lanes,
                            events=True)
    _events_large(base, trace, lanes)
