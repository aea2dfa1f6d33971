"""The shell the fortress fires, in split launches of the step kernel: the games' wave decides (slot, mask bit, timer, event),
the tile's missile wave computes the velocity and stores the shell's two chunks, and the new shell takes no part in the games'
wave's shell walk on the tick it is fired (spacefortress_amd/csrc/sf_kernels.hip: updateFortress, "the tile's MISSILE wave";
the geometry that allows it: tests/test_shell_fire_model.py; the record: profiles/step_shell_fire.md).

Every run steps TWO batches from the same constructed state with the same actions -- float32 features (split launches) and
the same with the final-observation output enabled (the non-split XTRA / FOBS instantiation, whose games' wave still does
all of it) -- and holds them

  * to each other bit for bit: observation, reward, done, info after every tick, every state field's bytes (the shell
    slots' among them, live or not: the game-over tick's memory image);
  * to the CPU oracle in lock-step: observation rows as float32 bit patterns, reward / done / info exactly, the state
    through sfcompare.compare_state; every scenario asserts from the ORACLE's trace that its event happened;
  * check_state() passes afterwards: no hand-over poll gave up.

Shapes: 64 envs (one tile, 64 envs per workgroup), 16 448 (the first multiple of 64 above 16 384: 128 per workgroup) and
32 832 (the first above 32 768: 256 per workgroup).  A tile is one of four blocks: `mixed` (lane % 16 = the scenarios of
_block), `all` (every lane fires a missile AND a shell on the first tick), `one` (lane 37 alone fires a shell), `none`."""
import numpy as np
import pytest

from lockstep import ST_SHELL, ST_SMALL, check_ticks, fresh, make_env, n_actions, oracle_trace, play, same_bytes, sfa

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GAMETYPES = ["youturn", "autoturn"]
BLOCKS = ["mixed", "all", "one", "none"]
SPF = 6       # sf_kernels.hip: SF_SPF, the shell slots the games' wave prefetches; slots beyond take its dependent-load loop
LOCK = 1000   # sf_layout.h: lock_time
MANY = (0, 2, 5, 9, 10, 14, 17, 19)


def _block(O, gametype, who, seed):
    """64 lanes.  Every ship stands at bearing 5 degrees of the fortress (sector 10, which the fortress already aims at), so a
    fort_timer at the lock time fires on the first tick.  `mixed`, lane % 16:
      0 a shot into slot 0;  1 into SPF - 1;  2 into SPF;  3 into 19;  4 all 20 slots full: no shot, the timer starts over;
      5 the ship dies by the small hexagon on this tick: no shot;  6 a shell (slot 3) kills the ship on this tick: the shot
      (slot 0) is fired, the ship was alive behind updateShip;  7 the ship respawns on this tick with fort_timer at the lock time: the respawn
      starts the timer over, nothing is fired;  8 the game ends on this tick;  9 three shells, slots 0 and 2 collide (the
      lowest leaves), the shot goes into 3;  10 four shells, a middle one (5) collides, the shot goes into 1;  11 eight
      shells, the highest (19) collides;  12 slot 4 leaves the area, slot 12 kills;  13 a missile and a shell in one tick;
      14 a dead fortress;  15 fort_timer three ticks below the lock time and a shell in slot 0: the shot comes on tick 3, into
      slot 1.
    Lanes 5, 7 and 15 play NOOP throughout."""
    rng = np.random.default_rng(seed)
    base = fresh(O, gametype, 64)
    base["ship_y"] = 315.0 + 9.0
    base["fort_angle"] = base["fort_last_angle"] = 10
    base["fort_timer"] = LOCK if who in ("mixed", "all") else 300
    acts0 = np.zeros(64, np.uint8)
    noop = np.zeros(64, bool)  # lanes that play NOOP throughout

    def fly(i, s):  # well inside the area, far from the ship and the fortress' line of fire
        base["shell_alive"][i, s] = 1
        base["shell_x"][i, s], base["shell_y"][i, s] = rng.uniform(200, 300), rng.uniform(180, 250)
        base["shell_vx"][i, s], base["shell_vy"][i, s] = rng.uniform(-1, 1, 2)

    def strike(i, s):  # on the ship after this tick's move (radius 13; a thrusting ship moves 0.3)
        base["shell_alive"][i, s] = 1
        base["shell_vx"][i, s], base["shell_vy"][i, s] = rng.uniform(-6, 6, 2)
        base["shell_x"][i, s] = base["ship_x"][i] - base["shell_vx"][i, s] + rng.uniform(-3, 3)
        base["shell_y"][i, s] = base["ship_y"][i] - base["shell_vy"][i, s] + rng.uniform(-3, 3)

    def leave(i, s):
        base["shell_alive"][i, s] = 1
        base["shell_x"][i, s], base["shell_y"][i, s] = 709.5, 300.0
        base["shell_vx"][i, s], base["shell_vy"][i, s] = 5.0, 0.5

    for i in range(64):
        if who == "all":
            acts0[i] = 1  # FIRE
            for s in ((), (0,), tuple(range(SPF)), (1, 4, 9, 13, 18))[i % 4]:
                fly(i, s)
        elif who == "one":
            if i == 37:
                base["fort_timer"][i] = LOCK
                fly(i, 0), fly(i, 7)
            elif i % 5 == 0:
                fly(i, i % 20)
        elif who == "none":
            if i % 3 == 0:
                fly(i, i % 20), fly(i, (i + 7) % 20)
        else:
            k = i % 16
            if k in (1, 2, 3, 4):
                for s in range({1: SPF - 1, 2: SPF, 3: 19, 4: 20}[k]):
                    fly(i, s)
            elif k == 5:
                base["ship_x"][i], base["ship_y"][i], base["ship_vy"][i] = 355.0, 352.0, -4.0
                noop[i] = True
            elif k == 6:
                strike(i, 3)
            elif k == 7:
                base["ship_alive"][i] = 0
                base["ship_death_timer"][i] = 1000 + 34
                noop[i] = True
            elif k == 8:
                base["time"][i] = 180000 - 34
            elif k == 9:
                strike(i, 0), fly(i, 1), strike(i, 2)
            elif k == 10:
                fly(i, 0), fly(i, 2), strike(i, 5), fly(i, 7)
            elif k == 11:
                for s in MANY:
                    (strike if s == 19 else fly)(i, s)
            elif k == 12:
                leave(i, 4), strike(i, 12)
            elif k == 13:
                acts0[i] = 1
            elif k == 14:
                base["fort_alive"][i] = 0
                base["fort_death_timer"][i] = 34
            elif k == 15:
                base["fort_timer"][i] = LOCK - 3 * 34
                fly(i, 0)
                noop[i] = True
    base["tick"] = base["time"] // 34
    return base, acts0, noop


def _batch(O, gametype, n, blocks, T):
    """Tile t of the batch is block blocks[t % len(blocks)]; tick 0 plays the blocks' actions, the rest random play."""
    rng = np.random.default_rng(1700 + n + len(gametype) + len(blocks[0]))
    parts = [_block(O, gametype, w, 1800 + k) for k, w in enumerate(blocks)]
    small = np.concatenate([p[0] for p in parts])
    idx = np.arange(n) % len(small)
    base = small[idx].copy()
    acts = rng.integers(0, n_actions(gametype), (T, n)).astype(np.uint8)
    acts[0] = np.concatenate([p[1] for p in parts])[idx]
    acts[:, np.concatenate([p[2] for p in parts])[idx]] = 0
    who = np.array([blocks[(i // 64) % len(blocks)] for i in range(n)])
    return base, acts, who


def _play(sfa, O, gametype, base, acts, lanes=None):
    """Both batches play `acts`; they are held to each other byte for byte and the first to the oracle (of `lanes` or of all
    lanes; the event words of every tick among it): the state after every tick of a batch of up to 256 envs, else after the first and the last.  Returns the oracle's
    trace."""
    n, T = len(base), len(acts)
    pv = np.zeros(n, np.int32)
    e1, e2 = make_env(sfa, gametype, base, pv), make_env(sfa, gametype, base, pv)
    e2.enable_final_obs()  # (the step leaves the split launch: the XTRA / FOBS instantiation, the same outputs)
    state_at = lambda t: n <= 256 or t in (0, T - 1)
    k1 = play(e1, acts, "step", state_at, check_state=True, events=True)  # (check_state: no hand-over poll gave up)
    k2 = play(e2, acts, "step", state_at, check_state=True, events=True)
    e1.close()
    e2.close()
    same_bytes(k1, k2)
    trace = oracle_trace(O, gametype, base, pv, acts, lanes)
    check_ticks(k1, trace, "f32_bits", lanes)
    return trace


def _events(base, acts, trace, who):
    """From the oracle's side: the scenarios happened in the compared ticks.  `base`, `acts`, `who`: of the traced lanes."""
    s1 = trace[0][4]
    d = s1["stats"] - base["stats"]
    sh0, sh1 = base["shell_alive"].astype(int), s1["shell_alive"].astype(int)
    n0, n1 = sh0.sum(1), sh1.sum(1)
    lane = np.arange(len(base)) % 64
    m = who == "all"
    if m.any():
        assert (n1[m] == n0[m] + 1).all() and (s1["missile_alive"][m].sum(1) == 1).all()  # a shell and a missile, every lane
        assert set((sh1[m] - sh0[m]).argmax(1).tolist()) == {0, 1, SPF}  # the slots the shots went into
    m = who == "one"
    if m.any():
        assert (n1[m & (lane == 37)] == 3).all() and (sh1[m & (lane == 37), 1] == 1).all()
        assert np.array_equal(sh1[m & (lane != 37)], sh0[m & (lane != 37)])
    m = who == "none"
    if m.any():
        assert np.array_equal(sh1[m], sh0[m]) and n0[m].sum() > 0
    mixed = who == "mixed"
    if not mixed.any():
        return
    K = lambda k: mixed & (lane % 16 == k)
    for k, slot in ((0, 0), (1, SPF - 1), (2, SPF), (3, 19)):
        assert (sh1[K(k), slot] == 1).all() and (sh0[K(k), slot] == 0).all() and (n1[K(k)] == slot + 1).all(), k
        assert (s1["fort_timer"][K(k)] == 34).all(), k
    assert (n0[K(4)] == 20).all() and (n1[K(4)] == 20).all() and (s1["fort_timer"][K(4)] == 34).all()
    assert (d[K(5), ST_SMALL] == 1).all() and (s1["ship_alive"][K(5)] == 0).all() and (n1[K(5)] == 0).all()
    assert (d[K(6), ST_SHELL] == 1).all() and (s1["ship_alive"][K(6)] == 0).all()
    assert (sh1[K(6), 0] == 1).all() and (sh1[K(6), 3] == 0).all()                       # fired, then killed by the older shell
    assert (s1["ship_alive"][K(7)] == 1).all() and (n1[K(7)] == 0).all() and (s1["fort_timer"][K(7)] == 34).all()
    assert trace[0][2][K(8)].all() and not trace[0][2][~K(8)].any() and (n1[K(8)] == 0).all()   # the game-over tick
    assert (d[K(9), ST_SHELL] == 1).all() and (sh1[K(9)][:, :4] == [0, 1, 1, 1]).all()
    assert (d[K(10), ST_SHELL] == 1).all() and (sh1[K(10)][:, [0, 1, 2, 5, 7]] == [1, 1, 1, 0, 1]).all()
    assert (d[K(11), ST_SHELL] == 1).all() and (sh1[K(11), 19] == 0).all() and (sh1[K(11), 1] == 1).all() and (n1[K(11)] == len(MANY)).all()
    assert (d[K(12), ST_SHELL] == 1).all() and (sh1[K(12)][:, [0, 4, 12]] == [1, 0, 0]).all() and (n1[K(12)] == 1).all()
    assert (s1["missile_alive"][K(13)].sum(1) == 1).all() and (n1[K(13)] == 1).all() and (acts[0][K(13)] == 1).all()
    assert (n1[K(14)] == 0).all() and (n1[K(15)] == 1).all() and (s1["fort_timer"][K(15)] == LOCK - 2 * 34).all()
    late = lambda t: trace[t][4]["shell_alive"][K(15)].astype(int)
    assert (late(2).sum(1) == 1).all() and (late(3)[:, :2] == 1).all() and (late(3).sum(1) == 2).all()  # the shot of tick 3


@pytest.mark.parametrize("who", BLOCKS)
@pytest.mark.parametrize("gametype", GAMETYPES)
def test_one_tile(sfa, oracle_mod, gametype, who):
    """64 envs, 36 ticks: every scenario of _block; a shot in every lane, in one lane and in none."""
    base, acts, w = _batch(oracle_mod, gametype, 64, [who], 36)
    trace = _play(sfa, oracle_mod, gametype, base, acts)
    _events(base, acts, trace, w)


@pytest.mark.parametrize("n", [16448, 32832])
@pytest.mark.parametrize("gametype", GAMETYPES)
def test_128_and_256_envs_per_workgroup(sfa, oracle_mod, gametype, n):
    """The first batch sizes above 16 384 and 32 768: the four blocks tile by tile for eight ticks; both batches in full
    against each other, the first four tiles and the last four against the oracle."""
    base, acts, w = _batch(oracle_mod, gametype, n, BLOCKS, 8)
    lanes = np.concatenate([np.arange(256), np.arange(n - 256, n)])
    trace = _play(sfa, oracle_mod, gametype, base, acts, lanes)
    _events(base[lanes], acts[:, lanes], trace, w[lanes])
    assert set(w[lanes][-64:].tolist()) == {"mixed"} and set(w[lanes].tolist()) == set(BLOCKS)
