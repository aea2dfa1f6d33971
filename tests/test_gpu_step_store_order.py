"""The step kernel's state stores and its pool hand-over, in the ticks in which their ORDER can show.

A launch of one tick with 256 envs per workgroup stores the ship's two chunks behind the shells' walk and the score chunk behind the missile events, long
before the timers, the reward and the rest of the lane; a new game rewrites both, so a tick in which a lane of the tile
finishes stores them a second time.  A split launch's games' wave takes the missile events of its lanes from the tile's
missile wave, through LDS, behind the ship's stores.  None of that changes a result: every case here steps a batch in
lock-step with the CPU oracle and compares, after EVERY tick,

  * the observation rows as bit patterns (the oracle's float64 row, rounded to float32 for float32 batches: the integers are
    exact and the three bearings agree to 1e-13 relative, as in test_gpu_step_reorder),
  * reward / done / info exactly,
  * every state field get_field reads back (sfcompare.compare_state: bit for bit; the shells' positions to 1e-9, the oracle's
    libm against the device's direction arithmetic, as everywhere),
  * the rows of the output arrays BEHIND n_envs, which no lane may write (the outputs live in arenas with a sentinel tail,
    looked at behind the last tick: nothing puts a sentinel back; the state of the padding lanes themselves is not reachable
    through the API).

The same cases run a second time in ONE fresh child process with SFMI_FORCE_SPLIT=1; its per-tick SHA-256 over the raw bytes of
every output and every state field must equal this process's: the two launches agree byte for byte, shells included.

Shapes: 64 envs (one tile, a workgroup of one tile), 256 (four tiles), 320 (a padded tile row); and, in this process only,
32 832 envs (one tile past 32 768: the smallest batch stepped with 256 envs per workgroup, the launches that store early;
four whole tiles of it against the oracle, float32 and float64 rows).  Lane i plays part i % 8:

  0  `time` two ticks short of the game's end: tick 1 is a `done` tick with auto-reset in an eighth of every tile's lanes
  1  a dead ship whose explosion ends: it respawns in tick 0
  2  a ship that flies into the small hexagon in tick 0
  3  a ship that a shell kills in tick 0 (parts 2 and 3: two ways to die in one tick, in different lanes)
  4  fires a missile in tick 0 and in tick 2
  5  three missiles under way, one of which hits the fortress in tick 0
  6  three missiles under way, one of which leaves the area in tick 0
  7  three missiles under way, random keys
  (parts 5-7: 72 missiles a tile, more than a pool row, in the ticks in which part 4 fires: the events come through the
  hand-over.  Tick 1 has no missile event in any lane.)

Each case asserts from the ORACLE's side that these things happened in the compared ticks.  One step_repeat case (repeat 3) and
one rollout case (K = 4) per game type cover the stores of the REPEAT and FUSED instantiations, and a float64-observation
batch the one-tick instantiations that are not split."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from lockstep import (ST_INCS, ST_MISSED, ST_SHELL, ST_SHOTS, ST_SMALL, check_ticks, every, make_env, missile_table, n_actions, oracle_trace,
                      play, sfa)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

GAMETYPES = ["youturn", "autoturn"]
SHAPES = [64, 256, 320]
T = 6
SENTINEL = 0x5A


# ---------------------------------------------------------------- the cases

def _setup(O, gametype, n):
    rng = np.random.default_rng(7000 + n + len(gametype))
    tab = missile_table()
    base = O.OracleVecEnv(gametype, n).snapshots()
    base["ship_x"], base["ship_y"] = 455.0, 315.0  # inside the big hexagon, outside the small one: nothing happens by itself
    base["ship_vx"], base["ship_vy"] = 0.0, 0.0
    base["time"] = 34 * rng.integers(10, 3000, n)
    base["fort_vuln_timer"] = 300
    base["vlner"] = 5
    kind = np.arange(n) % 8
    for i in range(n):
        k = kind[i]
        if k == 0:
            base["time"][i] = 180000 - 34 * 2
        elif k == 1:
            base["ship_alive"][i] = 0
            base["ship_death_timer"][i] = 1000
        elif k == 2:
            base["ship_x"][i], base["ship_y"][i] = 355.0, 352.0
            base["ship_vy"][i] = -4.0
        elif k == 3:
            s = int(rng.integers(0, 6))
            base["shell_alive"][i, s] = 1
            base["shell_vx"][i, s], base["shell_vy"][i, s] = rng.uniform(-6, 6, 2)
            base["shell_x"][i, s] = 455.0 - base["shell_vx"][i, s] + rng.uniform(-3, 3)
            base["shell_y"][i, s] = 315.0 - base["shell_vy"][i, s] + rng.uniform(-3, 3)
        elif k >= 5:
            for j, s in enumerate(rng.choice(20, 3, replace=False)):
                ang = int(rng.integers(0, 360))
                base["missile_alive"][i, s] = 1
                base["missile_angle"][i, s] = ang
                base["missile_vx"][i, s], base["missile_vy"][i, s] = tab[ang]
                if k == 5 and j == 0:    # on the fortress after tick 0's move
                    base["missile_x"][i, s] = 355 - tab[ang, 0] + rng.uniform(-5, 5)
                    base["missile_y"][i, s] = 315 - tab[ang, 1] + rng.uniform(-5, 5)
                elif k == 6 and j == 0:  # outside the area after tick 0's move, whatever the heading
                    base["missile_x"][i, s], base["missile_y"][i, s] = -50.0, 300.0
                else:                    # far from the fortress and from every edge for all T ticks
                    c = np.array([130.0, 315.0]) if rng.random() < 0.5 else np.array([600.0, 315.0])
                    base["missile_x"][i, s], base["missile_y"][i, s] = c - 3 * tab[ang]
    base["tick"] = base["time"] // 34
    acts = np.zeros((T, n), np.uint8)
    acts[0, kind == 4] = 1
    acts[2, kind == 4] = 1
    acts[:, kind == 7] = rng.integers(2, n_actions(gametype), (T, int((kind == 7).sum())))  # any key but FIRE
    return base, base["vlner"].astype(np.int32), acts


def _check_events(base, trace, n):
    """From the oracle's side: the compared ticks hold what the module's docstring says."""
    kind = np.arange(n) % 8
    s0, d0 = trace[0][4], trace[0][4]["stats"] - base["stats"]
    assert trace[1][2][kind == 0].all() and not trace[1][2][kind != 0].any() and not trace[0][2].any()
    assert (s0["ship_alive"][kind == 1] == 1).all()
    assert (d0[kind == 2, ST_SMALL] == 1).all() and (d0[kind == 3, ST_SHELL] == 1).all()
    assert (s0["ship_alive"][np.isin(kind, (2, 3))] == 0).all()
    assert (d0[kind == 4, ST_SHOTS] == 1).all() and (s0["missile_alive"][kind == 4].sum(1) == 1).all()
    assert (d0[kind == 5, ST_INCS] == 1).all() and (d0[kind == 6, ST_MISSED] == 1).all()
    alive = np.array([base["missile_alive"].sum(1)] + [tr[4]["missile_alive"].sum(1) for tr in trace])  # [T + 1, n]
    fired = np.array([tr[4]["stats"][:, ST_SHOTS] for tr in trace]) - np.array(
        [base["stats"][:, ST_SHOTS]] + [tr[4]["stats"][:, ST_SHOTS] for tr in trace[:-1]])
    gone = alive[:-1] + fired - alive[1:]  # missiles that hit or left, per tick and lane (no new game among their owners)
    gone[:, kind == 0] = 0
    full = n // 64 * 64
    tiles = lambda x: x[:full].reshape(-1, 64).sum(1)
    assert (tiles(alive[0]) >= 64).all() and (tiles(gone[0]) >= 16).all()      # a full row, events and a shot in tick 0
    assert (tiles(gone[1]) == 0).all() and (gone[1] == 0).all()                # no lane owns an event in tick 1
    assert (tiles(alive[2]) >= 64).all() and (tiles(fired[2]) == 8).all()      # a full row and a shot again in tick 2


_CASES = {}


def _case(O, gametype, n):
    """(base, prev_vlner, actions, the oracle's trace): computed once, shared, never changed."""
    key = (gametype, n)
    if key not in _CASES:
        base, pv, acts = _setup(O, gametype, n)
        trace = oracle_trace(O, gametype, base, pv, acts)
        _check_events(base, trace, n)
        for x in (base, pv, acts):
            x.setflags(write=False)
        _CASES[key] = (base, pv, acts, trace)
    return _CASES[key]


# ---------------------------------------------------------------- the device's side (this process and the child)

def _arena(torch, env, rows):
    """The four outputs as the first n rows of arenas of `rows` rows filled with the sentinel."""
    n = env.num_envs
    big = (torch.empty((rows,) + tuple(env.obs_shape), dtype=env.obs_dtype, device=env.device),
           torch.empty(rows, dtype=torch.int32, device=env.device), torch.empty(rows, dtype=torch.uint8, device=env.device),
           torch.empty(rows, dtype=torch.uint8, device=env.device))
    for b in big:
        b.view(torch.uint8).fill_(SENTINEL)
    return big, tuple(b[:n] for b in big)


def _play(m, gametype, base, pv, acts, f64=False):
    """Step the batch tick by tick, the outputs in arenas.  Returns (Ticks with the state after every tick, the sha256 per
    tick of all the outputs' and the state's bytes); asserts that nothing behind n_envs was written."""
    import torch

    n = len(base)
    env = make_env(m, gametype, base, pv, f64=f64)
    big, out = _arena(torch, env, (n + 255) // 256 * 256)
    ticks = play(env, acts, "step", every(1), out=out, check_state=True, events=True)
    for b in big:  # (nothing puts the sentinel back: a tail still whole after the last tick was whole after every tick)
        tail = b[n:].contiguous().view(torch.uint8).cpu().numpy()
        assert (tail == SENTINEL).all(), ("written behind n_envs", tuple(b.shape))
    env.close()
    digests = []
    for t in range(len(acts)):
        h = hashlib.sha256()
        for x in (ticks.obs[t], ticks.reward[t], ticks.done[t], ticks.info[t]):
            h.update(x.tobytes())
        sd = ticks.states[t]
        for k in sorted(sd):
            h.update(k.encode() + np.ascontiguousarray(sd[k]).tobytes())
        digests.append(h.hexdigest())
    return ticks, digests


def _child_main(path):
    """The child process: every case of the file `path`, its digests as one JSON line."""
    sys.path.insert(0, ROOT)
    import spacefortress_amd as m

    z = np.load(path, allow_pickle=False)
    out = {}
    for name in json.loads(str(z["names"])):
        gametype, n = name.split(":")
        out[name] = _play(m, gametype, z[name + ":base"], z[name + ":pv"], z[name + ":acts"])[1]
    print("DIGESTS " + json.dumps(out), flush=True)


if __name__ == "__main__":
    _child_main(sys.argv[1])
    sys.exit(0)

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


_PLAYED = {}


def _played(sfa, O, gametype, n):
    if (gametype, n) not in _PLAYED:
        base, pv, acts, _ = _case(O, gametype, n)
        _PLAYED[(gametype, n)] = _play(sfa, gametype, base, pv, acts)
    return _PLAYED[(gametype, n)]


@pytest.fixture(scope="module")
def forced_split_digests(oracle_mod, tmp_path_factory):
    """Every (game type, shape) once more, in ONE fresh child process with SFMI_FORCE_SPLIT=1."""
    path = str(tmp_path_factory.mktemp("store_order") / "cases.npz")
    arrays, names = {}, []
    for gametype in GAMETYPES:
        for n in SHAPES:
            base, pv, acts, _ = _case(oracle_mod, gametype, n)
            name = "%s:%d" % (gametype, n)
            names.append(name)
            arrays[name + ":base"], arrays[name + ":pv"], arrays[name + ":acts"] = base, pv, acts
    np.savez(path, names=np.array(json.dumps(names)), **arrays)
    r = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=dict(os.environ, SFMI_FORCE_SPLIT="1"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("DIGESTS ")]
    assert line, r.stdout[-2000:]
    return json.loads(line[-1][len("DIGESTS "):])


def _against_oracle(ticks, trace, f64=False, lanes=None):
    """Every tick's outputs, state and event words against the oracle's (of `lanes` of the batch, or of all of it): float32
    rows as bit patterns, float64 rows to sfcompare.obs_close's 1e-9, the words bit for bit."""
    check_ticks(ticks, trace, "close_f64" if f64 else "f32_bits", lanes)


@pytest.mark.parametrize("n", SHAPES)
@pytest.mark.parametrize("gametype", GAMETYPES)
def test_every_tick_against_the_oracle(sfa, oracle_mod, gametype, n):
    """The batch as launched by default: outputs and every state field after every tick."""
    _against_oracle(_played(sfa, oracle_mod, gametype, n)[0], _case(oracle_mod, gametype, n)[3])


@pytest.mark.parametrize("n", SHAPES)
@pytest.mark.parametrize("gametype", GAMETYPES)
def test_forced_split_child_agrees_byte_for_byte(sfa, oracle_mod, forced_split_digests, gametype, n):
    """The same ticks in a fresh process with SFMI_FORCE_SPLIT=1: the digest of every output and state byte, tick by tick."""
    mine = _played(sfa, oracle_mod, gametype, n)[1]
    theirs = forced_split_digests["%s:%d" % (gametype, n)]
    assert mine == theirs, [t for t in range(T) if mine[t] != theirs[t]]


@pytest.mark.parametrize("gametype", GAMETYPES)
def test_float64_observations_one_tick_not_split(sfa, oracle_mod, gametype):
    """A float64-observation batch is stepped by the one-tick instantiations without a missile wave."""
    base, pv, acts, trace = _case(oracle_mod, gametype, 256)
    _against_oracle(_play(sfa, gametype, base, pv, acts, f64=True)[0], trace, f64=True)


BIG = 32832                   # one tile past 32 768 envs: workgroups of 256 envs, the launches that store chunks early
BIG_TILES = (0, 1, 300, 512)  # the tiles compared with the oracle; 512 is the last one, in front of a padded tile row


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("gametype", GAMETYPES)
def test_workgroups_of_256_envs(sfa, oracle_mod, gametype, f64):
    """The smallest batch that is stepped with 256 envs per workgroup, where a launch of one tick stores the ship's chunks and
    the score chunk early: float32 rows by the split instantiation, float64 rows by the one without a missile wave.  The
    256-env case repeated over the batch; four whole tiles against the oracle after every tick, the last tile among them."""
    base, pv, acts, _ = _case(oracle_mod, gametype, 256)
    base, pv, acts = np.resize(base, BIG), np.resize(pv, BIG), np.stack([np.resize(a, BIG) for a in acts])
    lanes = np.concatenate([np.arange(64 * k, 64 * k + 64) for k in BIG_TILES])
    trace = oracle_trace(oracle_mod, gametype, base, pv, acts, lanes)
    _check_events(base[lanes], trace, len(lanes))
    _against_oracle(_play(sfa, gametype, base, pv, acts, f64=f64)[0], trace, f64=f64, lanes=lanes)


def _state_bytes(sd):
    return {k: np.ascontiguousarray(v).tobytes() for k, v in sd.items()}


@pytest.mark.parametrize("gametype", GAMETYPES)
def test_rollout_of_four_ticks(sfa, oracle_mod, gametype):
    """The FUSED instantiation keeps its single store behind the tick loop: K = 4 ticks in one launch give the rows and leave
    the state of four single steps (which the tests above hold to the oracle), byte for byte."""
    base, pv, acts, trace = _case(oracle_mod, gametype, 256)
    single = _played(sfa, oracle_mod, gametype, 256)[0]
    env = make_env(sfa, gametype, base, pv)
    obs, rew, done, info = (x.cpu().numpy() for x in env.rollout(torch.from_numpy(np.array(acts[:4])).to(env.device)))
    assert np.array([tr[2] for tr in trace[:4]]).any()  # a new game inside the launch
    for t in range(4):
        assert obs[t].tobytes() == single.obs[t].tobytes() and rew[t].tobytes() == single.reward[t].tobytes(), t
        assert done[t].tobytes() == single.done[t].tobytes() and info[t].tobytes() == single.info[t].tobytes(), t
    assert _state_bytes(env.state_dict()) == _state_bytes(single.states[3])
    env.close()


@pytest.mark.parametrize("gametype", GAMETYPES)
def test_step_repeat_of_three_ticks(sfa, oracle_mod, gametype):
    """The REPEAT instantiation: one action for three ticks in one launch.  The lanes whose game ends inside the window stop
    there (their new game is not played on); every other lane's state, summed reward, info and observation are those of
    three single steps with that action, which the oracle plays here."""
    from sfcompare import compare_state

    n = 256
    base, pv, acts, _ = _case(oracle_mod, gametype, n)
    orc = oracle_mod.OracleVecEnv(gametype, n)
    orc.load_snapshots(base, pv)
    steps = [orc.step(acts[0].astype(np.int32)) for _ in range(3)]
    snaps = orc.snapshots()
    ended = np.array([s[2] for s in steps]).any(0)
    assert ended.any() and not ended.all()
    keep = np.flatnonzero(~ended)
    env = make_env(sfa, gametype, base, pv)
    obs, rew, done, info = (x.cpu().numpy() for x in env.step_repeat(torch.from_numpy(acts[0].copy()).to(env.device), 3))
    assert np.array_equal(done.astype(bool), ended)
    assert (env.last_ticks.cpu().numpy()[keep] == 3).all()
    want = steps[2][0].astype(np.float32)
    assert obs[keep].view(np.uint32).tobytes() == want[keep].view(np.uint32).tobytes()
    assert np.array_equal(rew[keep], sum(s[1] for s in steps)[keep])
    assert np.array_equal(info[keep].astype(bool), np.array([s[3] for s in steps]).any(0)[keep])
    bad = compare_state(env.state_dict(), snaps[keep], lanes=keep)
    assert not bad, bad
    env.close()
