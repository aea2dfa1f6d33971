"""aim, vdir and ndist -- observation columns 6, 7, 8 and monitors' thresholds of them -- of EVERY path that writes an observation,
held to the 70-digit reference of tests/bearingref.py by the bounds derived there (1.88e-13 degrees on aim, 2.18e-13 on vdir, on
the circle; ndist bit for bit; float32 rows as the rounding of a double within the bound; monitors with a band), on the ~3 000
states of its generator (lane i takes state i % P; tests/test_bearing_columns_model.py proves reference, bounds and states
consistent on the host, and that the bounds notice three mutants).  The four restatements of the numerical code and what
selects them (sf_kernels.hip: sf_launch_step's rule -- fast_obs = features & float32 & n % 64 == 0; xtra / fobs = a
final-observation output; split = fast_obs & !xtra & lanes <= 65536 -- and sf_launch_step_repeat):

  float64 features, step_tensors          generic writer, immediates, LDS table; also at n % 64 != 0 (the tail wave)
  float32 features, default               split launch: constants as data (SfKRow, sf_atan2_razor), write_features_f32
  float32 features + enable_final_obs     fast writer, not split (FOBS)
  normalized-features, both dtypes        generic writer, Python's % and the clamps
  monitors                                the thresholds
  rollout of two ticks                    FUSED (both rows)
  step_repeat, K = 3                      REPEAT: the bearings carried to the window's one row
  reset(), reset_lanes(mask), a tick that ends every game
                                          device-libm form at spawn points: the new game's row; the final_obs row of the
                                          finished game, from the tick's own bearings
  save_lanes -> load_lanes(obs=...)       sf_lanes_load_kernel: the global-table form for played states, the reset form
                                          (device libm) for time == 0 rows -- here the whole generator, unplayed

The reference is evaluated on the state the row describes: the CPU oracle's snapshot after the tick, which `compare_state` holds
bit for bit to the device's `state_dict()` in the same test (ship position, velocity and heading are also compared directly).
Every column outside {6, 7, 8} must equal what `state_dict()` implies (values: the only licence is the sign of a zero quotient,
sf_div_const's documented one), kill_ready as the kernels define it.  Ships that die on the tick stay in.

`pytest -s` prints one table: per case, column and family the largest error in units of its bound (float32: 0 inside the allowed
interval of floats).  Measured values: profiles/bearing_columns.md."""

import numpy as np
import pytest

import bearingref as br
from lockstep import load_state, sfa
from sfcompare import compare_state

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GAMETYPES = ["youturn", "autoturn"]
INPUTS = ("ship_x", "ship_y", "ship_vx", "ship_vy", "ship_angle")


class _World:
    """The generator's states as oracle snapshots, the oracle's snapshots after 1, 2 and 3 ticks without keys, and the
    reference on each of them -- computed once per module, never changed."""

    def __init__(self, O):
        self.O = O
        self.st = br.states()
        self.P = len(self.st)
        self.n = -(-self.P // 64) * 64
        self.snaps, self.refs = {}, {}
        for g in GAMETYPES:
            base = self.base(g, self.n)
            orc = O.OracleVecEnv(g, self.n)
            orc.load_snapshots(base, np.zeros(self.n, np.int32))
            self.snaps[g] = [base.copy()]
            for _ in range(3):
                orc.step(np.zeros(self.n, np.int32))
                self.snaps[g].append(orc.snapshots())

    def base(self, g, n):
        st = self.st[np.arange(n) % self.P]
        base = self.O.OracleVecEnv(g, n).snapshots()
        for k, f in (("ship_x", "sx"), ("ship_y", "sy"), ("ship_vx", "vx"), ("ship_vy", "vy"), ("ship_angle", "angle")):
            base[k] = st[f]
        return base

    def tiled(self, g, t, n):
        return self.snaps[g][t][np.arange(n) % self.P] if n != self.n else self.snaps[g][t]

    def ref(self, g, t):
        if (g, t) not in self.refs:
            s = self.snaps[g][t][: self.P]
            self.refs[g, t] = br.reference(s["ship_x"], s["ship_y"], s["ship_vx"], s["ship_vy"], s["ship_angle"].astype(np.int64))
        return self.refs[g, t]

    def fam(self, n):
        i = np.arange(n) % self.P
        return self.st["family"][i], self.st["note"][i]


@pytest.fixture(scope="module")
def world(oracle_mod):
    return _World(oracle_mod)


@pytest.fixture(scope="module")
def table():
    rows = []
    yield rows
    fams = sorted({f for r in rows for f in r[1]}, key=lambda f: (list(br.FAMILIES) + [f]).index(f))
    print("\n\nbearing columns on the device: largest error per case, column and family, in units of the bound")
    print("%-64s" % "case / column" + "".join("%10s" % f for f in fams))
    inside = 0
    for name, row in rows:
        if " f32 " in name and not any(row.values()):
            inside += 1  # (a float32 row's figure is its distance to the allowed interval of floats: 0 inside)
            continue
        print("%-64s" % name + "".join("%10.3g" % row[f] if f in row else "%10s" % "-" for f in fams))
    print("float32: %d rows (case, column), every value inside its interval of at most two floats" % inside)


def _make(sfa, g, base, **kw):
    n = len(base)
    env = sfa.SFVecEnv(n, gametype=g, **kw)
    load_state(env, base, np.zeros(n, np.int32))
    return env


def _same_inputs(sd, snaps, lanes=None):
    """the five inputs of the reference, device against oracle, bit for bit (compare_state holds the whole state)"""
    for k in INPUTS:
        a = np.asarray(sd[k]) if lanes is None else np.asarray(sd[k])[lanes]
        b = snaps[k] if lanes is None else snaps[k][lanes]
        assert np.array_equal(a.astype(np.float64).view(np.uint64), np.asarray(b, np.float64).view(np.uint64)), k


def _hold(table, case, g, ot, obs, sd, ref, ridx, fam, lanes=None):
    """One observation array [m, dim] against the reference (row j: reference entry ridx[j], lane lanes[j] of `sd`) by every
    rule of bearingref; adds the case's rows to the table, then asserts."""
    famv, note = fam
    f32 = obs.dtype == np.float32
    cast = (lambda a: a.astype(np.float32)) if f32 else (lambda a: a)
    R = {k: ([v[j] for j in ridx] if isinstance(v, list) else v[ridx]) for k, v in ref.items()}
    other = br.other_columns(sd, ot, g == "youturn", lanes)
    bad = []
    title = "%s %s %s %s " % (case, g, ot, "f32" if f32 else "f64")

    def note_rows(col, err, ok):
        if col in ("aim", "vdir", "naim", "nvdir"):  # (the exact checks have nothing to tabulate)
            table.append((title + col, {str(f): float(np.max(err[famv == f])) for f in dict.fromkeys(famv.tolist())}))
        for i in np.flatnonzero(~ok)[:4]:
            bad.append((col, str(famv[i]), str(note[i]), int(i), float(err[i])))

    if ot == "monitors":
        assert np.array_equal(obs[:, :4], cast(other)), (title, np.argwhere(obs[:, :4] != cast(other))[:5].tolist())
        want, free = br.monitors_columns(R)
        ok = ((obs[:, 4:10] == want) | free).all(1)
        note_rows("thresholds", (~ok).astype(np.float64), ok)
        assert free.mean(0).max() < br.BAND_SHARE_MAX, free.mean(0)
        assert not bad, bad
        return
    keep = [c for c in range(obs.shape[1]) if c not in (6, 7, 8)]
    ne = np.argwhere(obs[:, keep] != cast(other[:, keep]))
    assert ne.size == 0, (title, "columns outside 6, 7, 8", ne[:5].tolist())
    names = ("aim", "vdir", "ndist") if ot == "features" else ("naim", "nvdir", "nndist")
    for c in (6, 7):
        err, ok = br.check_column(obs[:, c], R[names[c - 6]], *br.RULES[ot][c], f32=f32)
        note_rows(names[c - 6], err, ok)
    ok = obs[:, 8] == cast(R[names[2]])
    note_rows(names[2] + " (bit for bit)", (~ok).astype(np.float64), ok)
    g_ = (lambda k: np.asarray(sd[k])) if lanes is None else (lambda k: np.asarray(sd[k])[lanes])
    rest = g_("ship_vx") * g_("ship_vx") + g_("ship_vy") * g_("ship_vy") == 0.0
    ok = ~rest | (obs[:, 7] == 0.0)
    if rest.any():
        note_rows("vdir at rest is 0.0", (~ok).astype(np.float64), ok)
    assert not bad, (title, bad)


def _noop(env):
    return torch.zeros(env.num_envs, dtype=torch.uint8, device=env.device)


def _finish(env):
    env.check_actions()
    env.check_state()
    env.close()


# ---------------------------------------------------------------- one tick through every stepping path

STEP_CASES = [  # (case, observation type, dtype, final-observation output, batch beyond the generator's size)
    ("generic writer", "features", "f64", False, 0),
    ("generic writer, tail wave", "features", "f64", False, 37),
    ("split launch", "features", "f32", False, 0),
    ("fast writer, not split (FOBS)", "features", "f32", True, 0),
    ("generic writer", "normalized-features", "f32", False, 0),
    ("generic writer", "normalized-features", "f64", False, 0),
    ("thresholds", "monitors", "f32", False, 0),
]


@pytest.mark.parametrize("case,ot,dt,fobs,extra", STEP_CASES, ids=[("%s %s %s" % c[:3]).replace(",", "").replace(" ", "_") for c in STEP_CASES])
@pytest.mark.parametrize("g", GAMETYPES)
def test_one_tick(sfa, world, table, g, case, ot, dt, fobs, extra):
    n = world.n + extra
    env = _make(sfa, g, world.base(g, n), obs_type=ot, obs_dtype=torch.float64 if dt == "f64" else torch.float32)
    if fobs:
        env.enable_final_obs()
    obs = env.step_tensors(_noop(env))[0].cpu().numpy()
    sd, snaps = env.state_dict(), world.tiled(g, 1, n)
    bad = compare_state(sd, snaps)
    assert not bad, bad
    _same_inputs(sd, snaps)
    _hold(table, case, g, ot, obs, sd, world.ref(g, 1), np.arange(n) % world.P, world.fam(n))
    _finish(env)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("g", GAMETYPES)
def test_rollout_of_two_ticks(sfa, world, table, g, dt):
    """FUSED: both rows; the first against the oracle's state after one tick (the device's is not to be had in between), the
    second against state_dict()."""
    n = world.n
    env = _make(sfa, g, world.base(g, n), obs_dtype=torch.float64 if dt == "f64" else torch.float32)
    obs = env.rollout(torch.zeros((2, n), dtype=torch.uint8, device=env.device))[0].cpu().numpy()
    sd = env.state_dict()
    bad = compare_state(sd, world.snaps[g][2])
    assert not bad, bad
    _same_inputs(sd, world.snaps[g][2])
    # the first row's other columns: the twin batch's state after one tick
    twin = _make(sfa, g, world.base(g, n), obs_dtype=torch.float64)
    twin.step_tensors(_noop(twin))
    sd1 = twin.state_dict()
    assert not compare_state(sd1, world.snaps[g][1])
    _same_inputs(sd1, world.snaps[g][1])
    _hold(table, "rollout (FUSED), tick 1", g, "features", obs[0], sd1, world.ref(g, 1), np.arange(n) % world.P, world.fam(n))
    _hold(table, "rollout (FUSED), tick 2", g, "features", obs[1], sd, world.ref(g, 2), np.arange(n) % world.P, world.fam(n))
    _finish(twin)
    _finish(env)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("g", GAMETYPES)
def test_step_repeat_of_three_ticks(sfa, world, table, g, dt):
    """REPEAT: the bearings of the window's last tick, carried behind the loop to the one row."""
    n = world.n
    env = _make(sfa, g, world.base(g, n), obs_dtype=torch.float64 if dt == "f64" else torch.float32)
    obs = env.step_repeat(_noop(env), 3)[0].cpu().numpy()
    assert (env.last_ticks.cpu().numpy() == 3).all()
    sd = env.state_dict()
    bad = compare_state(sd, world.snaps[g][3])
    assert not bad, bad
    _same_inputs(sd, world.snaps[g][3])
    _hold(table, "step_repeat, K = 3 (REPEAT)", g, "features", obs, sd, world.ref(g, 3), np.arange(n) % world.P, world.fam(n))
    _finish(env)


# ---------------------------------------------------------------- new games: the device-libm form

def _spawn_ref(sd, lanes=None):
    f = (lambda k: np.asarray(sd[k])) if lanes is None else (lambda k: np.asarray(sd[k])[lanes])
    return br.reference(f("ship_x"), f("ship_y"), f("ship_vx"), f("ship_vy"), f("ship_angle").astype(np.int64))


def _spawn_fam(n):
    return np.array(["spawn"] * n), np.array([""] * n)


def _is_spawn(O, g, sd, lanes):
    """the reference's inputs of a new game are pinned: integer spawn points inside the area, the preset's start velocity"""
    one = O.OracleVecEnv(g, 1).snapshots()
    x, y = np.asarray(sd["ship_x"])[lanes], np.asarray(sd["ship_y"])[lanes]
    assert ((x == np.rint(x)) & (x >= 170) & (x < 550) & (y == np.rint(y)) & (y >= 150) & (y < 480)).all()
    assert (np.asarray(sd["ship_vx"])[lanes] == one["ship_vx"][0]).all() and (np.asarray(sd["ship_vy"])[lanes] == one["ship_vy"][0]).all()
    assert (np.asarray(sd["time"])[lanes] == 0).all()


@pytest.mark.parametrize("ot,dt", [("features", "f32"), ("features", "f64"), ("normalized-features", "f64"), ("monitors", "f32")])
@pytest.mark.parametrize("g", GAMETYPES)
def test_reset_and_reset_lanes(sfa, oracle_mod, table, g, ot, dt):
    n = 640
    env = sfa.SFVecEnv(n, gametype=g, obs_type=ot, obs_dtype=torch.float64 if dt == "f64" else torch.float32, spawn_stride=3)
    orc = oracle_mod.OracleVecEnv(g, n, spawn_stride=3)
    obs = env.reset().cpu().numpy()
    orc.reset()
    sd = env.state_dict()
    bad = compare_state(sd, orc.snapshots())
    assert not bad, bad
    _same_inputs(sd, orc.snapshots())
    _is_spawn(oracle_mod, g, sd, np.arange(n))
    _hold(table, "reset()", g, ot, obs, sd, _spawn_ref(sd), np.arange(n), _spawn_fam(n))
    # two ticks on, every third lane starts over: only those rows are written
    for _ in range(2):
        env.step_tensors(_noop(env))
    mask = torch.zeros(n, dtype=torch.uint8, device=env.device)
    mask[::3] = 1
    out = torch.full((n, env.obs_dim), 7.0, dtype=env.obs_dtype, device=env.device)
    env.reset_lanes(mask=mask, out=out)
    out = out.cpu().numpy()
    lanes = np.arange(0, n, 3)
    keep = np.ones(n, bool)
    keep[lanes] = False
    assert (out[keep] == 7.0).all()
    sd = env.state_dict()
    _is_spawn(oracle_mod, g, sd, lanes)
    assert (np.asarray(sd["time"])[keep] == 68).all()
    _hold(table, "reset_lanes(mask)", g, ot, out[lanes], sd, _spawn_ref(sd, lanes), np.arange(len(lanes)), _spawn_fam(len(lanes)), lanes=lanes)
    _finish(env)


@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("g", GAMETYPES)
def test_the_tick_that_ends_the_game(sfa, world, table, g, dt):
    """`time` one tick short of the limit: the step returns the new game's row (device libm at the spawn point) and writes the
    finished game's last row to final_obs, from the tick's own bearings.  That row describes the state a twin batch without
    the time limit holds after the same tick (held to the oracle); for youturn ships at rest it is the state in front of the
    tick, so the row is also held to the reference on the generator's own inputs."""
    n = world.n
    kw = {"obs_dtype": torch.float64 if dt == "f64" else torch.float32}
    env = _make(sfa, g, world.base(g, n), spawn_stride=3, **kw)  # (a spawn stream per lane: the new games differ)
    env.set_field("time", np.full(n, 180000 - 34, np.int32))
    fo = env.enable_final_obs()
    obs, rew, done, info = [x.cpu().numpy() for x in env.step_tensors(_noop(env))]
    assert (done == 1).all()
    sd = env.state_dict()
    _is_spawn(world.O, g, sd, np.arange(n))
    _hold(table, "new game's row at done", g, "features", obs, sd, _spawn_ref(sd), np.arange(n), _spawn_fam(n))
    twin = _make(sfa, g, world.base(g, n), **kw)
    twin.step_tensors(_noop(twin))
    sd1 = twin.state_dict()
    assert not compare_state(sd1, world.snaps[g][1])
    _same_inputs(sd1, world.snaps[g][1])
    last = fo.cpu().numpy()
    _hold(table, "final_obs row at done", g, "features", last, sd1, world.ref(g, 1), np.arange(n) % world.P, world.fam(n))
    if g == "youturn":
        st = world.st
        rest = np.flatnonzero((st["vx"] == 0) & (st["vy"] == 0))
        r0 = br.reference(st["sx"][rest], st["sy"][rest], st["vx"][rest], st["vy"][rest], st["angle"][rest])
        for c, k in ((6, "aim"), (7, "vdir")):
            err, ok = br.check_column(last[rest, c], r0[k], *br.RULES["features"][c], f32=dt == "f32")
            assert ok.all(), (k, st["note"][rest][~ok][:5], err[~ok][:5])
        assert np.array_equal(last[rest, 8], r0["ndist"].astype(last.dtype))
    _finish(twin)
    _finish(env)


# ---------------------------------------------------------------- lane states into a second batch

@pytest.mark.parametrize("ot,dt", [("features", "f32"), ("features", "f64"), ("normalized-features", "f32"), ("monitors", "f32")])
@pytest.mark.parametrize("g", GAMETYPES)
def test_load_lanes_observations(sfa, world, table, g, ot, dt):
    """sf_lanes_load_kernel: a played batch's rows (time 34) take the global-table form; the same states unplayed (time 0)
    count as new games and take the device libm -- the whole generator through the form that otherwise only meets spawn
    points."""
    n = world.n
    kw = {"obs_type": ot, "obs_dtype": torch.float64 if dt == "f64" else torch.float32}
    src = _make(sfa, g, world.base(g, n), **kw)
    unplayed = src.save_lanes()
    src.step_tensors(_noop(src))
    played = src.save_lanes()
    dst = sfa.SFVecEnv(n, gametype=g, **kw)
    for t, states, case in ((1, played, "load_lanes, played (global table)"), (0, unplayed, "load_lanes, time == 0 (device libm)")):
        buf = torch.full((n, dst.obs_dim), 7.0, dtype=dst.obs_dtype, device=dst.device)
        dst.load_lanes(states, obs=buf)
        sd = dst.state_dict()
        bad = compare_state(sd, world.snaps[g][t])
        assert not bad, bad
        _same_inputs(sd, world.snaps[g][t])
        assert (np.asarray(sd["time"]) == 34 * t).all()
        _hold(table, case, g, ot, buf.cpu().numpy(), sd, world.ref(g, t), np.arange(n) % world.P, world.fam(n))
    _finish(src)
    _finish(dst)


# ---------------------------------------------------------------- device against oracle next to the wraps

@pytest.mark.parametrize("g", GAMETYPES)
def test_device_and_oracle_name_the_same_angle_on_the_wraps(sfa, world, g):
    """One angle has two names at a wrap: vdir at +-180, the normalised vdir at 0 and 1, aim at -180 and 180.  The device (a
    derived first angle) and the CPU oracle (glibc, a second atan2) are each within the bound of the true angle, so they agree
    within twice the bound ON THE CIRCLE -- and may show opposite ends of the range, which an agent sees as a jump.
    Asserted: the agreement on the circle, every lane.  Printed: how many lanes show opposite ends."""
    n = world.n
    fam, note = world.fam(n)
    for ot in ("features", "normalized-features"):
        env = _make(sfa, g, world.base(g, n), obs_type=ot, obs_dtype=torch.float64)
        obs = env.step_tensors(_noop(env))[0].cpu().numpy()
        orc = world.O.OracleVecEnv(g, n, obs_type=ot)
        orc.load_snapshots(world.base(g, n), np.zeros(n, np.int32))
        want = orc.step(np.zeros(n, np.int32))[0]
        for c in (6, 7):
            bound, period, _ = br.RULES[ot][c]
            d = np.abs(obs[:, c] - want[:, c])
            ends = d > period / 2
            d = np.minimum(d, np.abs(period - d))
            assert (d <= 2 * bound + np.spacing(float(period))).all(), (ot, c, note[np.argmax(d)], float(d.max()))
            print("\n%s %s column %d: %d of %d lanes on opposite ends of the range%s; bit-identical %.1f %%"
                  % (g, ot, c, int(ends.sum()), n, (" (" + ", ".join(sorted(set(note[ends].tolist()))[:4]) + ")") if ends.any() else "",
                     100 * (obs[:, c] == want[:, c]).mean()))
        assert np.array_equal(obs[:, 8], want[:, 8])
        _finish(env)
