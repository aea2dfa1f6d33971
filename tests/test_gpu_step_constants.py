"""Where the step kernel's fp64 constants come from -- compiled in, or read as data from the constants block a split launch
stages into LDS (the hexagon edges, the atan table, the kernel constants row; profiles/step_constants.md) -- must not show
in any result.  Three checks, at the smallest batches that select the 64-, 128- and 256-env split workgroups (256, 16 640
and 33 024 envs):

  * edge census: ships put (set_field) exactly on the 12 hexagon edge lines, one ulp to either side in x and in y, and on
    the 12 vertices, at rest and arriving there by one step of velocity; NOOP for two ticks; ship-alive flag, the three
    death counters, reward and ship_death_timer against the CPU oracle, every lane, exactly.  The same cases through
    launches that leave the split path: with given actions through the final-observation launch (it must give the split
    launch's bits), and through step_sampled with its played-action output on.  (That output exists for drawn actions only:
    the lanes there play what they drew, the oracle plays the same, and a THRUST moves a ship off its edge -- so this run is
    held to the oracle, not to the NOOP run's bits.)
  * path differential: the same constructed states and the same ring of actions for 300 ticks, once through the split
    launch and once through the non-split instantiation of the same library (final-observation output on); every output
    array and every lane-state row (sf_save_lanes: every state field) bit for bit after every tick, every field of
    state_dict at the end.  The three atan2-derived feature columns and fort_angle are among them.
  * LDS map: a tick with a FULL missile pool in the batch's last tile (20 missiles in every lane, some of which hit the
    fortress or leave the area on that tick -- the event words -- and lanes with 19 that fire their 20th -- the hand-over);
    the pool's count, check_state() and the observation rows of the last tile (the staging rows) against the oracle: what
    a shifted LDS map that overlapped would break."""
import numpy as np
import pytest

from bearingref import VDIR_BOUND, close_on_circle_f32
from lockstep import (ST_BIG, ST_SHELL, ST_SMALL, check_ticks, every, fresh, fuzz_sparse, make_env, missile_table, n_actions, oracle_trace, play,
                      same_bytes, sfa)
from sfcompare import compare_state, obs_close

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SIZES = [256, 16640, 33024]  # 64, 128 and 256 envs per split workgroup (sf_launch_step)
GAMETYPES = ["youturn", "autoturn"]
# sf_layout.h: SF_BIG_HEX_EDGES / SF_SMALL_HEX_EDGES, (nx, ny, px, py); edge k runs from vertex (px, py)_k to vertex k + 1
BIG = [(174.0, 100.0, 155.0, 315.0), (-0.0, 200.0, 255.0, 141.0), (-174.0, 100.0, 455.0, 141.0),
       (-173.0, -100.0, 555.0, 315.0), (-0.0, -200.0, 455.0, 488.0), (173.0, -100.0, 255.0, 488.0)]
SMALL_HEX = [(35.0, 20.0, 315.0, 315.0), (-0.0, 40.0, 335.0, 280.0), (-35.0, 20.0, 375.0, 280.0),
             (-34.0, -20.0, 395.0, 315.0), (-0.0, -40.0, 375.0, 349.0), (34.0, -20.0, 335.0, 349.0)]


# ---------------------------------------------------------------- 1. edge census

def _census_points(quarters):
    """[(x, y)] where the ship is to stand after its move: per edge the midpoint of the edge (`quarters`: and its quarter
    points; all exactly on its line: the coordinates are multiples of 1/4 and n . (p - p_k) cancels exactly), per vertex the
    vertex; each of them as it is and one ulp to either side in x and in y.  120 points, with the quarter points 240."""
    pts = []
    for hexagon in (BIG, SMALL_HEX):
        for k, (nx, ny, px, py) in enumerate(hexagon):
            qx, qy = hexagon[(k + 1) % 6][2:]
            on = [(px + t * (qx - px), py + t * (qy - py)) for t in ((0.25, 0.5, 0.75) if quarters else (0.5,))]
            for x, y in on:
                assert nx * (x - px) + ny * (y - py) == 0.0  # on the edge's line, exactly
            for x, y in on + [(px, py)]:
                pts += [(x, y), (np.nextafter(x, np.inf), y), (np.nextafter(x, -np.inf), y),
                        (x, np.nextafter(y, np.inf)), (x, np.nextafter(y, -np.inf))]
    return np.array(pts)


def _census_base(O, gametype, n):
    """Lane i takes point i % P; the first P lanes at rest, the next P arriving by one step of velocity (s + v == point,
    exactly), and so on alternating."""
    pts = _census_points(quarters=n >= 480)  # (a batch of 256 envs holds the 120 points twice, the larger ones the 240)
    P = len(pts)
    assert 2 * P <= n and P == 2 * 6 * (4 if n >= 480 else 2) * 5
    base = fresh(O, gametype, n)
    i = np.arange(n)
    tgt = pts[i % P]
    moving = (i // P) % 2 == 1
    vel = np.zeros((n, 2))
    found = ~moving
    for v in ((1.5, -2.25), (-1.5, 2.25), (0.5, 0.75), (-0.5, -0.75)):  # the first step that lands on the point exactly
        s = tgt - np.array(v)
        ok = moving & ~found & ((s + np.array(v)) == tgt).all(1)
        vel[ok] = v
        found |= ok
    assert found.all()
    base["ship_x"], base["ship_y"] = tgt[:, 0] - vel[:, 0], tgt[:, 1] - vel[:, 1]
    base["ship_vx"], base["ship_vy"] = vel[:, 0], vel[:, 1]
    base["ship_angle"] = 90  # (autoturn games turn the ship themselves)
    return base, tgt, P


def _sampled_rule(obs, oo):
    """A drawn THRUST along the fortress's row or column leaves vdir (column 7) within rounding noise of +-180 degrees, one
    angle with two names: the device's derived bearing and the oracle's second atan2 differ by an ulp of pi there
    (sf_lane_dev.h: compute_extras) and land on either side, with the parent's library as with this one.  So the sampled run
    compares every other column to sfcompare's float32 tolerance and column 7 ON THE CIRCLE, by the rule of
    tests/bearingref.py: device and oracle are each within VDIR_BOUND of the true angle, so the float32 the device shows is
    within twice that, and half a float32 ulp, of the oracle's double, mod 360.  The NOOP runs compare all, bit for bit."""
    ok = obs_close(obs, oo, False)
    ok[:, 7] = close_on_circle_f32(obs[:, 7], oo[:, 7], 2 * VDIR_BOUND, 360)
    return ok


def _census_lockstep(O, env, gametype, base, pv, T, sampled):
    """T ticks of NOOP (sampled: of what the lanes draw, which the oracle then plays) against the oracle, the state after
    every tick; returns (Ticks, the oracle's trace)."""
    ticks = play(env, np.zeros((T, len(base)), np.uint8), "sampled" if sampled else "step", every(1), check_state=True,
                 events=True)
    trace = oracle_trace(O, gametype, base, pv, ticks.played)
    for t, (oo, orw, od, oi, snaps, _) in enumerate(trace):
        sd, rew = ticks.states[t], ticks.reward[t]
        # what the issue names, every lane, exactly ...
        assert np.array_equal((sd["flags"] & 1) != 0, snaps["ship_alive"] != 0), t
        for st in (ST_BIG, ST_SMALL, ST_SHELL):
            assert np.array_equal(sd["stats"][st], snaps["stats"][:, st]), (t, st)
        assert np.array_equal(rew, orw), (t, np.flatnonzero(rew != orw)[:5])
        assert np.array_equal(sd["ship_death_timer"], snaps["ship_death_timer"]), t
    # ... and the rest of the tick with it, the event words included
    check_ticks(ticks, trace, _sampled_rule if sampled else "f32_bits")
    return ticks, trace


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("gametype", GAMETYPES)
def test_edge_census(sfa, oracle_mod, gametype, n):
    O = oracle_mod
    base, tgt, P = _census_base(O, gametype, n)
    pv = np.zeros(n, np.int32)
    runs = {}
    for path in ("split", "final_obs", "sampled"):
        env = make_env(sfa, gametype, base, pv)
        if path == "final_obs":
            env.enable_final_obs()  # (the step leaves the split launch: the XTRA / FOBS instantiation, given actions)
        runs[path] = _census_lockstep(O, env, gametype, base, pv, 2, path == "sampled")
        env.close()
    # the census is one: ships ON a line live, the ulp to the outside of the big hexagon / the inside of the small one kills
    s1 = runs["split"][1][0][4]
    d = s1["stats"] - base["stats"]
    assert (d[:, ST_BIG] == 1).any() and (d[:, ST_SMALL] == 1).any() and (s1["ship_alive"] == 1).any()
    assert np.array_equal(s1["ship_x"], tgt[:, 0]) and np.array_equal(s1["ship_y"], tgt[:, 1])  # every ship stood on its point
    rest, mov = slice(0, P), slice(P, 2 * P)
    assert np.array_equal(s1["ship_alive"][rest], s1["ship_alive"][mov])  # at rest or arriving: the same verdict
    # the non-split launch with the same (NOOP) actions: the same bits in every output and every state field
    same_bytes(runs["split"][0], runs["final_obs"][0])


# ---------------------------------------------------------------- 2. path differential

@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("gametype", GAMETYPES)
def test_split_and_non_split_paths_agree_for_300_ticks(sfa, oracle_mod, gametype, n):
    O = oracle_mod
    rng = np.random.default_rng(4100 + n + len(gametype))
    small, pv_s = fuzz_sparse(O, gametype, 512, rng)
    idx = np.arange(n) % 512
    base, pv = small[idx].copy(), pv_s[idx]
    ring = torch.from_numpy(rng.integers(0, n_actions(gametype), (37, n)).astype(np.uint8))
    envs = []
    for non_split in (False, True):
        env = make_env(sfa, gametype, base, pv, seed=7)
        if non_split:
            env.enable_final_obs()
        envs.append(env)
    e1, e2 = envs
    ring = ring.to(e1.device)
    same = torch.ones((), dtype=torch.bool, device=e1.device)
    first_bad = None
    T = 300
    for t in range(T):
        a = ring[t % len(ring)]
        o1, o2 = e1.step_tensors(a), e2.step_tensors(a)
        for x, y in zip(o1, o2):  # obs (the bearings' columns 6 and 7 and fort_angle's 10 among them), reward, done, info
            same &= (x.view(torch.uint8) == y.view(torch.uint8)).all()
        same &= torch.equal(e1.save_lanes().rows, e2.save_lanes().rows)  # every state field, as the lane rows pack them
        if (t + 1) % 50 == 0 and first_bad is None and not bool(same):
            first_bad = t - 49
    assert first_bad is None, "the two paths differ within the 50 ticks from tick %d" % first_bad
    sd1, sd2 = e1.state_dict(), e2.state_dict()
    for k in sd1:
        assert np.array_equal(np.asarray(sd1[k]).view(np.uint8), np.asarray(sd2[k]).view(np.uint8)), k
    # (the run is not idle: ships died on both hexagons and the fortress turned)
    assert (sd1["stats"][ST_BIG] > base["stats"][:, ST_BIG]).any() and (sd1["stats"][ST_SMALL] > base["stats"][:, ST_SMALL]).any()
    assert len(set(sd1["fort_angle"].tolist())) > 10
    for e in envs:
        e.check_actions()
        e.check_state()
        e.close()


# ---------------------------------------------------------------- 3. the LDS map

def _full_pool_base(O, gametype, n):
    """The batch's last tile with a full missile pool: 20 missiles in every lane -- slot 0 about to hit the fortress, slot 1
    about to leave the area, the others in flight at headings that run through the table -- but for every fourth lane, which
    has 19 and fires its 20th this tick."""
    base = fresh(O, gametype, n)
    tab = missile_table()
    last = np.arange(n - 64, n)
    k = 0
    for i in last:
        for s in range(20):
            if s == 19 and i % 4 == 0:
                continue
            a = (k * 7) % 360
            k += 1
            base["missile_alive"][i, s] = 1
            base["missile_angle"][i, s] = a
            base["missile_vx"][i, s], base["missile_vy"][i, s] = tab[a]
            if s == 0:
                base["missile_x"][i, s], base["missile_y"][i, s] = 355 - tab[a, 0] + 3.0, 315 - tab[a, 1] - 2.0
            elif s == 1:  # heading 0 or 180, half a pixel from the border it flies at
                a = 0 if i % 2 else 180
                base["missile_angle"][i, s] = a
                base["missile_vx"][i, s], base["missile_vy"][i, s] = tab[a]
                base["missile_x"][i, s], base["missile_y"][i, s] = (709.5 if a == 0 else 0.5), 300.0
            else:
                base["missile_x"][i, s], base["missile_y"][i, s] = 120.0 + (k % 90), 80.0 + (k % 45)
    return base, last


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("gametype", GAMETYPES)
def test_full_pool_tick_in_the_last_tile(sfa, oracle_mod, gametype, n):
    O = oracle_mod
    base, last = _full_pool_base(O, gametype, n)
    pv = np.zeros(n, np.int32)
    env = make_env(sfa, gametype, base, pv, events=True)
    orc = O.OracleVecEnv(gametype, 64)
    orc.load_snapshots(base[last], pv[last])
    acts = np.zeros((2, n), np.uint8)
    acts[0, last[::4]] = 1   # FIRE in the last tile: the lanes with 19 fill their last slot (the hand-over)
    acts[0, last[1::4]] = 1  # ... and full lanes, whose shot is counted and creates nothing
    dev = torch.from_numpy(acts).to(env.device)
    assert base["missile_alive"][last].sum() == 64 * 20 - 16
    for t in range(2):
        obs, rew, done, info = [x.cpu().numpy() for x in env.step_tensors(dev[t])]
        oo, orw, od, oi = orc.step(acts[t, last].astype(np.int32))
        snaps = orc.snapshots()
        want = oo.astype(np.float32)
        bad = np.argwhere(obs[last].view(np.uint32) != want.view(np.uint32))  # the staging rows of the last tile
        assert bad.size == 0, (t, bad[:5].tolist())
        assert np.array_equal(rew[last], orw) and np.array_equal(done[last].astype(bool), od), t
        assert np.array_equal(info[last].astype(bool), oi), t
        assert np.array_equal(env.events.cpu().numpy().view(np.uint32)[last], orc.events()), t  # the event words of the last tile
        sd = env.state_dict()
        pool = int(sum(bin(int(m)).count("1") for m in sd["missile_mask"][last]))  # the pool's live entries
        assert pool == int((snaps["missile_alive"] != 0).sum()), (t, pool)
        bad = compare_state(sd, snaps, lanes=last)  # the pool's entries, found by owner and slot
        assert not bad, (t, bad)
        env.check_state()  # state_ok: no hand-over poll gave up, no packed field wrapped
        if t == 0:
            # the tick did what it is here for: 64 hits and 64 departures reached their owners, 16 missiles were handed over
            assert (snaps["missile_alive"][:, 0] == 0).all() and (snaps["missile_alive"][:, 1] == 0).all()
            assert (snaps["missile_alive"][::4, 19] == 1).all() and pool == 64 * 18
    # the other tiles saw nothing of it
    assert (env.get_field("missile_mask")[: n - 64] == 0).all()
    env.check_actions()
    env.close()
