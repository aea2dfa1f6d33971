"""Constructed states for the event-word tests (tests/test_oracle_events.py on the CPU, tests/test_gpu_event_words.py on the
device): the builders only -- what is compared with what is the test files' business.  Every state is an oracle snapshot
array (oracle.SNAPSHOT_DTYPE) as tests/lockstep.py's builders make them, so it loads into the oracle, the reference engine
and a batch alike.

  * `multi_event_lane`   several missiles of ONE env one step from the fortress or from the border, with a chosen fortress
                         state: the ticks in which the closed form of spacefortress_amd/csrc/sf_events.h has something to
                         get wrong (MULTI lists the kinds);
  * `mixed_batch`        a fuzzed batch with such lanes across a tile boundary and in the partial last tile, and lanes whose
                         game ends within three ticks;
  * `owners_tile`        one tile in which every lane owns another number of hitting and of leaving missiles;
  * `edge_lanes`         single bits at their thresholds, the neighbour just short of it in the next lane;
  * `key_edge_lanes`     every previous key state against every action;
  * `combos`             which same-tick combinations a trace of event words holds (the oracle-side assertions)."""
import numpy as np

from lockstep import fresh, fuzz_crowded, fuzz_sparse, missile_table, n_actions

GAME_TIME, TICK_MS = 180000, 34  # SRC/configs.cpp:55,66,78,86; ENV:61
# where a ship at rest is left alone: between the hexagons, and off the fortress's row and column (a thrust along those puts
# vdir within rounding of +-180 degrees, one angle with two names: tests/test_gpu_step_constants.py, _sampled_rule)
PARK = (440.25, 250.5)

# kind -> (fort_alive, fort_vuln_timer, vlner, the missiles in slot order: h hits the fortress, m leaves the area)
MULTI = {
    "inc_then_resets": (1, 300, 9, "hhh"),        # vlner-increased and vlner-reset, three hits on a live fortress
    "inc_destroy_dead": (1, 300, 10, "hhh"),      # increment to 11, the second hit destroys, the third meets the dead fortress
    "inc_destroy": (1, 300, 10, "hh"),            # ... and without a third: destroyed, and NO hit-dead-fortress
    "resets_only": (1, 100, 5, "hh"),             # every hit a reset: live hits that are neither increments nor destructions
    "reset_miss_reset": (1, 100, 5, "hmh"),       # hits with a missile-left between them
    "dead_hits_and_miss": (0, 100, 5, "hhm"),     # a dead fortress: hit-dead-fortress alone, and a miss
    "miss_destroy_miss": (1, 100, 11, "mhm"),     # the one hit destroys, between two misses
    "four_resets": (1, 249, 3, "hhhh"),           # the window's last millisecond
    "one_miss": (1, 100, 5, "m"),
    "hit_and_leave_same_slot_order": (1, 300, 2, "mh"),
}
MULTI_KINDS = list(MULTI)


def clear_missiles(base, i):
    for k in ("missile_alive", "missile_x", "missile_y", "missile_vx", "missile_vy", "missile_angle"):
        base[k][i] = 0


def put_missile(base, i, s, what, rng, tab=None):
    """Slot s of lane i: "h" on the fortress after this tick's move, "m" outside the area after it whatever the heading, "f"
    in flight far from both."""
    tab = missile_table() if tab is None else tab
    ang = int(rng.integers(0, 360))
    base["missile_alive"][i, s] = 1
    base["missile_angle"][i, s] = ang
    base["missile_vx"][i, s], base["missile_vy"][i, s] = tab[ang]
    if what == "h":
        base["missile_x"][i, s] = 355 - tab[ang, 0] + rng.uniform(-5, 5)
        base["missile_y"][i, s] = 315 - tab[ang, 1] + rng.uniform(-5, 5)
    elif what == "m":
        base["missile_x"][i, s], base["missile_y"][i, s] = -50.0, 300.0
    else:
        base["missile_x"][i, s], base["missile_y"][i, s] = rng.uniform(100, 250), rng.uniform(60, 120)


def multi_event_lane(base, i, kind, rng, tab=None):
    """Lane i becomes the kind `kind` of MULTI: its missiles replaced, the fortress as the kind says; the ship parked where
    nothing happens to it by itself, so that the missile events are the lane's own whatever is played."""
    alive, vt, vl, seq = MULTI[kind]
    clear_missiles(base, i)
    base["ship_alive"][i] = 1
    base["ship_x"][i], base["ship_y"][i], base["ship_vx"][i], base["ship_vy"][i] = PARK + (0.0, 0.0)
    base["shell_alive"][i] = 0
    base["fort_alive"][i], base["fort_vuln_timer"][i], base["vlner"][i] = alive, vt, vl
    base["fort_death_timer"][i] = 34
    base["time"][i], base["tick"][i] = 34 * 100, 100
    slots = np.sort(rng.choice(20, len(seq), replace=False))
    for s, e in zip(slots, seq):
        put_missile(base, i, int(s), e, rng, tab)


# where the constructed lanes of a 200-lane mixed batch stand: across the boundary of tiles 0 and 1, and in the partial tile
MIXED_N = 200
MIXED_MULTI_LANES = list(range(59, 69)) + list(range(188, 198))
# lanes whose game ends on the run's first, second and third tick (time = game_time - k * 34), in every tile
MIXED_ENDING = {5: 1, 69: 2, 70: 2, 129: 1, 130: 3, 198: 1, 199: 3}
# lanes whose fortress has its aim and fires on the run's third tick (a fuzzed fortress turns on the first tick, which starts
# its timer over: it fires no sooner than 30 ticks later)
MIXED_FIRING = (20, 85, 150, 170)


MIXED_SEEDS = {"crowded": 5100, "sparse": 5200}  # + len(gametype); tests/test_oracle_events.py holds them to mixed_census on the CPU


def mixed_batch(O, gametype, fuzzer, seed=None, n=MIXED_N, ticks=12):
    """(base, prev_vlner, actions [ticks, n]): `fuzzer` ("crowded" / "sparse") states from default_rng(seed), MULTI lanes at
    MIXED_MULTI_LANES (every kind twice: once astride the first tile boundary, once in the partial last tile), and the lanes
    of MIXED_ENDING one to three ticks from game over."""
    rng = np.random.default_rng(MIXED_SEEDS[fuzzer] + len(gametype) if seed is None else seed)
    base, pv = (fuzz_crowded if fuzzer == "crowded" else fuzz_sparse)(O, gametype, n, rng)
    tab = missile_table()
    assert len(MIXED_MULTI_LANES) == 2 * len(MULTI_KINDS)
    for j, i in enumerate(MIXED_MULTI_LANES):
        multi_event_lane(base, i, MULTI_KINDS[j % len(MULTI_KINDS)], rng, tab)
    pv = np.asarray(pv).copy()
    pv[MIXED_MULTI_LANES] = base["vlner"][MIXED_MULTI_LANES]
    for i, k in MIXED_ENDING.items():
        assert i not in MIXED_MULTI_LANES and i < n
        base["time"][i] = GAME_TIME - k * TICK_MS
        base["tick"][i] = base["time"][i] // TICK_MS
    for i in MIXED_FIRING:  # the ship's bearing is 5.1 degrees, sector 10, and stays there under any three actions
        assert i not in MIXED_MULTI_LANES and i not in MIXED_ENDING
        base["ship_alive"][i], base["fort_alive"][i] = 1, 1
        base["ship_x"][i], base["ship_y"][i], base["ship_vx"][i], base["ship_vy"][i] = 455.0, 324.0, 0.0, 0.0
        base["shell_alive"][i] = 0
        clear_missiles(base, i)  # (none that could destroy the fortress first)
        base["fort_angle"][i] = base["fort_last_angle"][i] = 10
        base["fort_timer"][i] = 1000 - 2 * TICK_MS
    acts = rng.integers(0, n_actions(gametype), (ticks, n)).astype(np.uint8)
    return base, pv, acts


def mixed_census(gametype, base, trace, bit_of):
    """The oracle-side assertions of a mixed batch, from its trace alone; returns the counts ({name: cells}) for the record.
    Every bit the game type can show occurs (autoturn has no left / right keys: 18 of the 22), and every same-tick
    combination that the closed form of sf_events.h could get wrong occurs in some lane."""
    words = np.array([tr[5] for tr in trace])
    count = {nm: int(((words & np.uint32(b)) != 0).sum()) for nm, b in bit_of.items()}
    absent = {nm for nm, c in count.items() if c == 0}
    assert absent == (set() if gametype == "youturn" else {"press-left", "press-right", "release-left", "release-right"}), sorted(absent)
    count.update(combos(words, bit_of))
    hits, live = hit_counts(base, trace)
    count["two hits or more"] = int((hits >= 2).sum())
    count["three live hits or more"] = int((live >= 3).sum())
    for nm in ("increase+reset", "destroyed+hit-dead", "hit+missile-left", "two hits or more", "three live hits or more"):
        assert count[nm] > 0, (nm, count)
    done = np.array([tr[2] for tr in trace])
    assert done[0].any() and done[1].any() and done[2].any()  # games that end on the first, the second, the third tick
    assert set(np.flatnonzero(done.any(0)) // 64) == {0, 1, 2, 3}  # ... in every tile, the partial last one too
    return count


def owners_tile(O, gametype, rot, seed=2200):
    """One tile: the lane that stands `rot` places behind lane p's owns p % 7 hitting and (p // 7) % 7 leaving missiles (p a
    seeded permutation of 0..63: 49 different pairs, the rest again), in seeded slots, with a fortress that differs from
    lane to lane.  Returns (base, prev_vlner, the pattern [64, 2] per lane: hits, leaves)."""
    rng = np.random.default_rng(seed)
    base = fresh(O, gametype, 64)
    tab = missile_table()
    perm = rng.permutation(64)
    pat = np.zeros((64, 2), np.int64)
    for l0 in range(64):
        i, p = (l0 + rot) % 64, int(perm[l0])
        h, m = p % 7, (p // 7) % 7
        pat[i] = h, m
        base["fort_alive"][i] = p % 5 != 0
        base["fort_death_timer"][i] = 34
        base["fort_vuln_timer"][i] = 300 if p % 2 else 100
        base["vlner"][i] = 8 + p % 5
        seq = rng.permutation(np.array(list("h" * h + "m" * m)))
        for s, e in zip(np.sort(rng.choice(20, h + m, replace=False)), seq):
            put_missile(base, i, int(s), str(e), rng, tab)
    return base, base["vlner"].astype(np.int32), pat


def _start_for(end, vel):
    """A start s with s + vel == end exactly (the tick's `pos += vel`, one rounding)."""
    s = end - vel
    for _ in range(8):
        if s + vel == end:
            return s
        s = np.nextafter(s, np.inf if s + vel < end else -np.inf)
    raise AssertionError((end, vel))


def _hex_edge_points(radius):
    """Per edge of the hexagon of SRC/hexagon.cpp:13-34 its midpoint -- ON the line, which counts as inside (:36-48) -- and
    the same point one ulp further from the centre in every coordinate that differs from the centre's: outside."""
    s = np.sin(np.pi * 2 / 3)
    x1, x2, x3, x4 = np.floor(355 - radius), np.floor(355 - radius * 0.5), np.floor(355 + radius * 0.5), np.floor(355 + radius)
    y1, y2, y3 = 315.0, np.floor(315 - radius * s), np.floor(315 + radius * s)
    pts = [(x1, y1), (x2, y2), (x3, y2), (x4, y1), (x3, y3), (x2, y3)]
    out = []
    for k in range(6):
        (ax, ay), (bx, by) = pts[k], pts[(k + 1) % 6]
        mx, my = (ax + bx) / 2, (ay + by) / 2
        # the other side of the line: one ulp away from the centre along the axis the edge's normal leans to most
        if abs(by - ay) >= abs(bx - ax):
            ox, oy = np.nextafter(mx, np.inf if mx > 355 else -np.inf), my
        else:
            ox, oy = mx, np.nextafter(my, np.inf if my > 315 else -np.inf)
        out.append(((mx, my), (ox, oy)))
    return out


def edge_lanes(O, gametype):
    """(base, prev_vlner, expect): one lane per case on a `fresh` batch (ship parked, NOOP played); expect = [(lane, bit name,
    whether the oracle is to set it in the first tick)], the neighbour just short of a threshold in the next lane."""
    tab = missile_table()
    cases = []  # (setter(base, i), bit name, expected)

    def missile_from(ang, axis, start):
        def set_(base, i):
            base["missile_alive"][i, 7] = 1
            base["missile_angle"][i, 7] = ang
            base["missile_vx"][i, 7], base["missile_vy"][i, 7] = tab[ang]
            base["missile_x"][i, 7], base["missile_y"][i, 7] = (start, 100.0) if axis == "x" else (200.0, start)
        return set_

    # the four borders of outside_game_area (SRC/game.cpp:129-131: x < 0, x > 710, y > 626, y < 0), a missile heading at
    # each: from the start that ends the step exactly ON the border it stays, as it does from the next double inside and
    # from a whole step (20) inside; from the next double beyond and from a whole step beyond it leaves.  (What is expected
    # is the tick's own `pos += vel` in numpy's float64 and the four comparisons, nothing of the oracle's.)
    for ang, axis, border, outward in ((180, "x", 0.0, -1.0), (0, "x", 710.0, 1.0), (90, "y", 626.0, 1.0), (270, "y", 0.0, -1.0)):
        v = float(tab[ang, 0 if axis == "x" else 1])
        assert v * outward > 19.0, (ang, v)
        on = _start_for(border, v)
        for start, out in ((on, False), (np.nextafter(on, on - outward), False), (on - outward * 20.0, False),
                           (np.nextafter(on, on + outward), True), (on + outward * 20.0, True)):
            end = start + v
            assert ((end < 0) if border == 0.0 else (end > border)) == out, (ang, start, end)
            cases.append((missile_from(ang, axis, float(start)), "missile-left", out))

    def field(**kw):
        def set_(base, i):
            for k, v in kw.items():
                base[k][i] = v
        return set_

    # isGameOver: time >= game_time once the tick has added its 34 ms (:475, :487-489)
    cases.append((field(time=GAME_TIME - 2 * TICK_MS, tick=(GAME_TIME - 2 * TICK_MS) // TICK_MS), "game-over", False))
    cases.append((field(time=GAME_TIME - TICK_MS, tick=(GAME_TIME - TICK_MS) // TICK_MS), "game-over", True))
    # the fortress respawns when its death timer reads > 1000 (:199), before the tick's 34 ms are added
    cases.append((field(fort_alive=0, fort_death_timer=1000), "fortress-respawn", False))
    cases.append((field(fort_alive=0, fort_death_timer=1001), "fortress-respawn", True))
    # the ship respawns when its death timer reads >= explode_duration = 1000 (:152)
    cases.append((field(ship_alive=0, ship_death_timer=1000 - TICK_MS), "ship-respawn", False))
    cases.append((field(ship_alive=0, ship_death_timer=999), "ship-respawn", False))
    cases.append((field(ship_alive=0, ship_death_timer=1000), "ship-respawn", True))
    # the ship at rest on every edge of the two hexagons, and an ulp outside it: on the line is inside (:36-48), so the big
    # hexagon kills the second and the small one the first
    for radius, name in ((200, "explode-bighex"), (40, "explode-smallhex")):
        for (inx, iny), (outx, outy) in _hex_edge_points(radius):
            cases.append((field(ship_x=inx, ship_y=iny), name, radius == 40))
            cases.append((field(ship_x=outx, ship_y=outy), name, radius == 200))
    # the fortress fires at fort_timer >= lock_time = 1000 (:208) while its aim holds: the ship's bearing is 5.1 degrees,
    # sector 10
    aim = dict(ship_y=324.0, fort_angle=10, fort_last_angle=10)
    cases.append((field(fort_timer=999, **aim), "fortress-fired", False))
    cases.append((field(fort_timer=1000, **aim), "fortress-fired", True))

    n = 64 * ((len(cases) + 63) // 64)
    base = fresh(O, gametype, n)
    expect = []
    for i, (set_, name, want) in enumerate(cases):
        set_(base, i)
        expect.append((i, name, want))
    return base, np.zeros(n, np.int32), expect


def key_edge_lanes(O, gametype):
    """(base, actions [1, n], lanes): every previous key state -- fire / thrust (/ left / right) flags, 16 for youturn, 4 for
    autoturn -- against every action of action set 1: 80 or 12 lanes of a `fresh` batch of 128 or 64; the rest play NOOP."""
    nk = 4 if gametype == "youturn" else 2
    na = n_actions(gametype)
    lanes = (1 << nk) * na
    n = 64 * ((lanes + 63) // 64)
    base = fresh(O, gametype, n)
    base["ship_x"], base["ship_y"] = PARK
    acts = np.zeros((1, n), np.uint8)
    for i in range(lanes):
        prev, a = i // na, i % na
        for b, k in enumerate(("fire_flag", "thrust_flag", "left_flag", "right_flag")[:nk]):
            base[k][i] = (prev >> b) & 1
        acts[0, i] = a
    return base, acts, lanes


def combos(words, bit_of):
    """What the issue asks a mixed batch to hold, counted over a trace's event words [T, n] (SF_EV_* bits; bit_of: name ->
    bit).  Returns {name: count of (tick, lane) cells}.  The count of hits of a cell is not in its word: `hits` gives it,
    [T, n], from the oracle's statistics and missile masks (see hit_counts)."""
    w = np.asarray(words, np.uint32)
    has = lambda nm: (w & np.uint32(bit_of[nm])) != 0
    return {
        "increase+reset": int((has("vlner-increased") & has("vlner-reset")).sum()),
        "destroyed+hit-dead": int((has("fortress-destroyed") & has("hit-dead-fortress")).sum()),
        "hit+missile-left": int(((has("hit-fortress") | has("hit-dead-fortress")) & has("missile-left")).sum()),
    }


def hit_counts(base, trace):
    """Per tick and lane, from the oracle's snapshots alone: (missiles that hit the fortress, dead or alive; hits on a live
    fortress).  A missile leaves its slot by hitting or by leaving the area; the leavers are the tick's missed_shots."""
    ST_RESETS, ST_DESTROYED, ST_MISSED, ST_INCS = 4, 5, 6, 11
    prev, hits, live = base, [], []
    for tr in trace:
        s, done = tr[4], tr[2]
        d = s["stats"].astype(np.int64) - prev["stats"]
        # (the tick's own shot takes a slot that was free, so a slot alive before and free after is a missile that went; a
        #  shot that hits in the tick it is fired is not seen here: the counts are lower bounds)
        gone = ((prev["missile_alive"] != 0) & (s["missile_alive"] == 0)).sum(1)
        h = gone - d[:, ST_MISSED]
        lv = d[:, ST_INCS] + d[:, ST_RESETS] + d[:, ST_DESTROYED]
        hits.append(np.where(done, 0, h))  # (a finishing tick's snapshot is the new game's: not counted)
        live.append(np.where(done, 0, lv))
        prev = s
    return np.array(hits), np.array(live)
