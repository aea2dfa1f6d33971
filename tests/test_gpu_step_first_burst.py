"""The front of the step kernel's tick -- what the wave loads first and what it loads late, where the late words are first
read, the staged cos/sin and atan tables -- against the CPU oracle, in the scenarios in which a word that arrives LATE (or
is unpacked late) is consumed on that very tick, and in which every consumer of the staged tables runs on the first tick of
a launch.  Written with three reorderings of that front (timers_b into the late set, the tables in front of the state, the
staggered start behind the barrier: measured, not kept) and one that was kept (the late set unpacked behind the two
bearings, one tick per launch; in front of the tick loop in a fused launch): profiles/step_first_burst.md.  The tests hold
any order to the oracle's results.

In lock-step with the oracle, as tests/test_gpu_step_reorder.py: observation rows as float32 bit patterns, reward / done /
info exactly, the state through sfcompare.compare_state (shell positions to 1e-9).  Every scenario asserts from the ORACLE's
side that its event happened in the compared ticks.

Shapes: 64 and 256 envs (64 per workgroup: one tile, four), 384 where 360 headings need as many lanes, 16 448 (128 per
workgroup), 32 832 (256), 65 536 (the smallest split launch that takes the staggered start: it runs above 65 280 envs) and
65 600 (the smallest non-split plain one that does).  The non-split instantiations at 64 and 256 envs through float64
observations and through step_sampled; a fused rollout of four ticks, which shares the prologue, against four steps."""
import numpy as np
import pytest

from lockstep import (ST_DESTROYED, ST_INCS, ST_RESETS, ST_SHOTS, every, fresh, fused_equals_steps, fuzz_sparse, missile_table, n_actions,
                      run_lockstep, sfa)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GAMETYPES = ["youturn", "autoturn"]
SMALL = [64, 256]
MODES = ["split", "f64", "sampled", "fused"]  # float32 step (split launch) | float64 obs | step_sampled | rollout of all ticks
LOCK, RESPAWN, VULN, TICK = 1000, 1000, 250, 34  # sf_layout.h: lock_time, fort_respawn, vuln_time, tick_ms


def _run(sfa, O, gametype, base, pv, acts, mode="split", lanes=None, extra=None, before=None):
    """Load `base`, play len(acts) ticks (mode "sampled": the lanes draw their own actions, the oracle plays what they drew),
    compare every tick with the oracle (of `lanes` or of the whole batch): rows rounded to float32 as bit patterns, the event words bit for bit; the state
    after every tick of a batch of up to 512 envs, else (and of a fused launch) after the last.  `before(env)`: called right
    in front of the first step, for a launch that is to be the second of a pair.  Returns the oracle's trace [(obs, rew,
    done, info, snapshots)] and the device's final state_dict."""
    T = len(acts)
    trace, ticks = run_lockstep(sfa, O, gametype, base, pv, acts, mode, every(1 if (len(base) <= 512 and mode != "fused") else T),
                                "rounded_f32_bits", lanes=lanes, extra=extra, before=before, events=True)
    return trace, ticks.states[T - 1]


# ---------------------------------------------------------------- 1. the words of timers_b, consumed on this tick

def _setup_timers_b(O, gametype, n):
    """Lane i % 16: 0-2 fort_timer one tick below / at / above the lock time (ship and fortress alive); 3-5 a dead fortress with
    fort_death_timer below / at / above the respawn threshold; 6-11 a missile that hits this tick with (fort_vuln_timer, vlner)
    = (216, 10) reset, (216, 11) destroy, (250, 10) and (250, 11) increment, (284, 11) increment, (249, 11) destroy; 12 a RIGHT
    press edge and 13 a RIGHT release edge with non-zero right_timer (youturn); 14 a ship that respawns this tick with
    fort_timer running; 15 nothing."""
    rng = np.random.default_rng(700 + n)
    base = fresh(O, gametype, n)
    tab = missile_table()
    kind = np.arange(n) % 16
    base["fort_timer"] = 300
    base["fort_timer"][kind < 3] = np.array([LOCK - TICK, LOCK, LOCK + TICK])[kind[kind < 3]]
    dead = (kind >= 3) & (kind < 6)
    base["fort_alive"][dead] = 0
    base["fort_death_timer"][dead] = np.array([RESPAWN - TICK, RESPAWN, RESPAWN + TICK])[kind[dead] - 3]
    vt = {6: (216, 10), 7: (216, 11), 8: (250, 10), 9: (250, 11), 10: (284, 11), 11: (249, 11)}
    for i in range(n):
        if kind[i] in vt:
            base["fort_vuln_timer"][i], base["vlner"][i] = vt[kind[i]]
            s, ang = int(rng.integers(0, 8)), int(rng.integers(0, 360))
            base["missile_alive"][i, s] = 1
            base["missile_angle"][i, s] = ang
            base["missile_vx"][i, s], base["missile_vy"][i, s] = tab[ang]
            base["missile_x"][i, s] = 355 - tab[ang, 0] + rng.uniform(-5, 5)
            base["missile_y"][i, s] = 315 - tab[ang, 1] + rng.uniform(-5, 5)
    base["right_timer"][kind == 12] = -17
    base["right_flag"][kind == 13] = 1 if gametype == "youturn" else 0
    base["right_timer"][kind == 13] = 23
    base["ship_alive"][kind == 14] = 0
    base["ship_death_timer"][kind == 14] = 1000 + TICK
    base["fort_timer"][kind == 14] = 700
    acts = np.zeros((2, n), np.uint8)
    if gametype == "youturn":
        acts[:, kind == 12] = 4  # RIGHT pressed, held
    # ep_return: both halves non-trivial; the destroying lanes' reward carries across bit 16, upwards and from below zero
    ep = rng.integers(-3_000_000, 3_000_000, n).astype(np.int32)
    ep[kind == 7] = 0x0001FFFF
    ep[kind == 11] = -0x00010001
    return base, base["vlner"].astype(np.int32), acts, kind, ep


def _events_timers_b(base, trace, kind, gametype, ep, sd, mode):
    s1, s2 = trace[0][4], trace[1][4]
    d = s1["stats"] - base["stats"]
    n_sh = s1["shell_alive"].sum(1)
    given = mode != "sampled"  # (drawn actions move the ship, and with it the fortress's sector: those lanes are compared, not asserted)
    if given:
        assert (n_sh[kind == 0] == 0).all() and (s1["fort_timer"][kind == 0] == LOCK).all()  # below: no shell, timer runs on
        assert (s2["shell_alive"].sum(1)[kind == 0] == 1).all()                              # ... and fires a tick later
        assert (n_sh[(kind == 1) | (kind == 2)] == 1).all() and (s1["fort_timer"][(kind == 1) | (kind == 2)] == TICK).all()
    assert (s1["fort_alive"][(kind == 3) | (kind == 4)] == 0).all() and (s1["fort_alive"][kind == 5] == 1).all()
    assert (s2["fort_alive"][kind == 3] == 0).all() and (s2["fort_alive"][kind == 4] == 1).all()
    assert (d[kind == 6, ST_RESETS] == 1).all() and (s1["vlner"][kind == 6] == 0).all()
    assert (d[(kind == 7) | (kind == 11), ST_DESTROYED] == 1).all() and (s1["fort_alive"][(kind == 7) | (kind == 11)] == 0).all()
    assert (d[np.isin(kind, (8, 9, 10)), ST_INCS] == 1).all() and (s1["vlner"][kind == 8] == 11).all()
    assert (s1["vlner"][kind == 9] == 12).all() and (s1["vlner"][kind == 10] == 12).all()
    assert (s1["fort_vuln_timer"][np.isin(kind, (6, 7, 8, 9, 10, 11))] == TICK).all()
    if gametype == "youturn" and given:
        assert (s1["right_timer"][kind == 12] == 1).all() and (s2["right_timer"][kind == 12] == 2).all()   # press edge: 0, +1
        assert (s1["right_timer"][kind == 13] == -1).all()                                                 # release edge: 0, -1
    assert (s1["ship_alive"][kind == 14] == 1).all() and (s1["fort_timer"][kind == 14] == TICK).all()  # respawn zeroes it
    if given:
        assert (s1["fort_timer"][kind == 15] == 300 + TICK).all()
    rews = np.array([tr[1] for tr in trace]).astype(np.int64)
    assert not np.array([tr[2] for tr in trace]).any()
    want = (ep.astype(np.int64) + rews.sum(0)).astype(np.int32)
    if given:  # (a drawn FIRE costs its penalty in the same tick)
        assert (rews[0][(kind == 7) | (kind == 11)] > 0).all()  # the carry across bit 16 happens in the compared tick
        assert ((want[kind == 7] >> 16) == 2).all() and ((want[kind == 11] >> 16) == -1).all()
    assert np.array_equal(np.asarray(sd["ep_return"]).astype(np.int32), want)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("n", SMALL)
@pytest.mark.parametrize("gametype", GAMETYPES)
def test_timers_b_words_consumed_on_the_tick_they_arrive(sfa, oracle_mod, gametype, n, mode):
    """fort_timer, fort_death_timer, fort_vuln_timer, right_timer and the high half of ep_return, each at its threshold,
    mixed in one tile with lanes where nothing happens; through every kind of launch."""
    base, pv, acts, kind, ep = _setup_timers_b(oracle_mod, gametype, n)
    if mode == "fused":
        acts = np.concatenate([acts, acts])  # K = 4
    trace, sd = _run(sfa, oracle_mod, gametype, base, pv, acts, mode, extra={"ep_return": ep})
    _events_timers_b(base, trace, kind, gametype, ep, sd, mode)


# ---------------------------------------------------------------- 2. the staged tables on the first tick of a launch

def _setup_headings():
    """384 youturn lanes thrusting (and, every third, firing a tick later) at headings 0..359."""
    n = 384
    return n, np.arange(n) % 360


def test_thrust_and_fire_at_all_360_headings(sfa, oracle_mod):
    """The cos/sin table's every entry through the ship's thrust and through a missile fired this tick."""
    O = oracle_mod
    n, ang = _setup_headings()
    base = fresh(O, "youturn", n)
    base["ship_angle"] = ang
    acts = np.full((2, n), 2, np.uint8)  # THRUST
    acts[0, ::3] = 1                      # FIRE: a missile created this tick at the ship's heading
    trace, _ = _run(sfa, O, "youturn", base, np.zeros(n, np.int32), acts)
    s1 = trace[0][4]
    assert (s1["stats"][::3, ST_SHOTS] - base["stats"][::3, ST_SHOTS] == 1).all() and (s1["missile_alive"][::3].sum(1) == 1).all()
    thr = np.ones(n, bool)
    thr[::3] = False
    assert len(set(zip(s1["ship_vx"][thr].tolist(), s1["ship_vy"][thr].tolist()))) >= 230  # the headings' own velocities
    assert set(s1["missile_angle"][::3][s1["missile_alive"][::3].astype(bool)].tolist()) == set(ang[::3].tolist())


def _setup_pool(O, gametype):
    """256 lanes, four tiles whose missile pools hold 0, 40 (one row), 192 (three rows) and 256 entries (a fourth row: the
    dependent-load loop), at headings that run through 0..359."""
    n = 256
    base = fresh(O, gametype, n)
    tab = missile_table()
    per_lane = np.concatenate([np.zeros(64, int), (np.arange(64) < 40).astype(int), np.full(64, 3), np.full(64, 4)])
    k = 0
    for i in range(n):
        for s in range(per_lane[i]):
            a = (k * 7) % 360  # (7 and 360 are coprime: every heading within 360 entries)
            k += 1
            base["missile_alive"][i, 2 * s] = 1
            base["missile_angle"][i, 2 * s] = a
            base["missile_vx"][i, 2 * s], base["missile_vy"][i, 2 * s] = tab[a]
            base["missile_x"][i, 2 * s], base["missile_y"][i, 2 * s] = 200.0 + (k % 50), 120.0 + (k % 40)
    assert k == 40 + 192 + 256
    return n, base, per_lane


@pytest.mark.parametrize("second_of_a_pair", [False, True])
@pytest.mark.parametrize("mode", ["split", "f64"])
@pytest.mark.parametrize("gametype", GAMETYPES)
def test_pool_rows_at_all_headings(sfa, oracle_mod, gametype, mode, second_of_a_pair):
    """Tiles with zero, one, three and more than three pool rows; from a fresh launch and as the second launch of a pair."""
    O = oracle_mod
    n, base, per_lane = _setup_pool(O, gametype)
    acts = np.zeros((2, n), np.uint8)
    acts[0, ::5] = 1  # FIRE
    other, before = None, None
    if second_of_a_pair:
        other = sfa.SFVecEnv(n, gametype=gametype)
        other.reset()
        z = torch.zeros(n, dtype=torch.uint8, device=other.device)
        before = lambda env: other.step_tensors(z)  # no synchronisation in between: the next launch follows this one
    trace, _ = _run(sfa, O, gametype, base, np.zeros(n, np.int32), acts, mode, before=before)
    if other is not None:
        other.close()
    s1 = trace[0][4]
    moved = s1["missile_alive"].astype(bool) & base["missile_alive"].astype(bool)
    assert moved.sum() >= 40 + 192 + 256 - 8 and (s1["missile_x"][moved] != base["missile_x"][moved]).any()
    assert len(set(base["missile_angle"][base["missile_alive"].astype(bool)].tolist())) == 360
    assert (s1["missile_alive"][::5].sum(1) == per_lane[::5] + 1).all()  # the missile fired this tick


def _setup_bearings(O, n):
    """Autoturn ships on a grid around the fortress that includes both axes and exact-degree rays (45, 135, ... degrees)."""
    offs = [(dx, dy) for dx in (-100, -80, -60, 0, 60, 80, 100) for dy in (-100, -80, -60, 0, 60, 80, 100) if (dx, dy) != (0, 0)]
    base = fresh(O, "autoturn", n)
    o = np.array(offs)[np.arange(n) % len(offs)]
    base["ship_x"], base["ship_y"] = 355.0 + o[:, 0], 315.0 + o[:, 1]
    return base, o


@pytest.mark.parametrize("second_of_a_pair", [False, True])
@pytest.mark.parametrize("n", SMALL)
def test_autoturn_bearings_on_axes_and_exact_degree_rays(sfa, oracle_mod, n, second_of_a_pair):
    """The atan table's first consumers: the autoturn heading, the fortress sector and the bearing features."""
    O = oracle_mod
    base, o = _setup_bearings(O, n)
    acts = np.zeros((2, n), np.uint8)
    acts[1] = 2  # THRUST at the fortress: along the ray
    other, before = None, None
    if second_of_a_pair:
        other = sfa.SFVecEnv(n, gametype="autoturn")
        other.reset()
        z = torch.zeros(n, dtype=torch.uint8, device=other.device)
        before = lambda env: other.step_tensors(z)
    trace, _ = _run(sfa, O, "autoturn", base, np.zeros(n, np.int32), acts, before=before)
    if other is not None:
        other.close()
    s1 = trace[0][4]
    assert (s1["ship_alive"] == 1).all()
    on_axis = (o[:, 0] == 0) | (o[:, 1] == 0)
    diag = np.abs(o[:, 0]) == np.abs(o[:, 1])
    assert on_axis.any() and diag.any()
    assert set(s1["ship_angle"][on_axis].tolist()) == {0, 90, 180, 270}
    assert set(s1["ship_angle"][diag].tolist()) == {45, 135, 225, 315}
    assert len(set(s1["ship_angle"].tolist())) >= 20


# ---------------------------------------------------------------- 3. the larger workgroups and the staggered start

@pytest.mark.parametrize("n", [16448, 32832, 65536, 65600])
@pytest.mark.parametrize("gametype", GAMETYPES)
def test_three_ticks_at_the_larger_shapes(sfa, oracle_mod, gametype, n):
    """Three random ticks from constructed states: 128 and 256 envs per workgroup, the split launch that takes the staggered
    start (65 536) and the smallest non-split plain launch that does (65 600); a seeded sample of 256 lanes against the
    oracle, the last tile's among them."""
    O = oracle_mod
    rng = np.random.default_rng(800 + n + len(gametype))
    small, pv_s = fuzz_sparse(O, gametype, 512, rng)
    idx = np.arange(n) % 512
    base, pv = small[idx].copy(), pv_s[idx]
    acts = rng.integers(0, n_actions(gametype), (3, n)).astype(np.uint8)
    lanes = np.sort(np.concatenate([rng.choice(n - 64, 224, replace=False), n - 64 + rng.choice(64, 32, replace=False)]))
    trace, _ = _run(sfa, O, gametype, base, pv, acts, lanes=lanes)
    d = trace[-1][4]["stats"] - base["stats"][lanes]
    assert (d[:, [ST_RESETS, ST_SHOTS]] > 0).any(0).all()
    assert any((tr[4]["shell_alive"].sum(1) != base["shell_alive"][lanes].sum(1)).any() for tr in trace)


# ---------------------------------------------------------------- 4. constructed states through every kind of launch

@pytest.mark.parametrize("mode", ["f64", "sampled", "fused"])
@pytest.mark.parametrize("n", SMALL)
@pytest.mark.parametrize("gametype", GAMETYPES)
def test_fuzzed_states_through_the_other_launches(sfa, oracle_mod, gametype, n, mode):
    """Four ticks from constructed states through the non-split instantiations (float64 observations, step_sampled) and
    through a fused rollout of K = 4, which must equal four steps -- and the oracle's."""
    O = oracle_mod
    rng = np.random.default_rng(900 + n + len(gametype))
    base, pv = fuzz_sparse(O, gametype, n, rng)
    acts = rng.integers(0, n_actions(gametype), (4, n)).astype(np.uint8)
    trace, _ = _run(sfa, O, gametype, base, pv, acts, mode)
    d = trace[-1][4]["stats"] - base["stats"]
    assert (d[:, ST_RESETS] > 0).any() and (d[:, ST_SHOTS] > 0).any()
    if mode == "fused":  # ... and four single steps give the same arrays as the one fused launch
        fused_equals_steps(sfa, gametype, base, pv, acts)
