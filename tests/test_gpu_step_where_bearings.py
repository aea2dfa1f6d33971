"""The observation rows sf_hold_end_kernel writes for HELD envs (include/sfmi_hold.h: sf_step_where), held to the bounds of
DESIGN 9: aim within 1.88e-13 degrees and vdir within 2.18e-13 of the 70-digit reference of tests/bearingref.py on the circle, ndist
bit for bit, a float32 row the rounding of a double inside the bound, every other column exactly what state_dict() implies --
the rules and the ~3 000 states of tests/test_gpu_bearing_columns.py (its `_hold`, as for sf_load_lanes), here for the rows that
come from the stash through LDS and obs_rows_from_stage, and for both sides of its switch on time == 0:

  call 1 on the generator's states, UNPLAYED (time 0): the held lanes' rows take the reset's form (device libm), the active
         lanes' rows are the step's own, one tick on;
  call 2 with the complementary mask: the lanes that played are now held at time 34 and take the step's table form, the others
         catch up;
  a SF_FLAG_REF_RESET_OBS batch: held new games of which no tick has been played read aim = vdir = ndist = 0 as their reset did,
         byte for byte; the same lanes held after their first tick read the bearings of their state.

The reference is evaluated on the state the row describes: the oracle's snapshot, which compare_state holds to state_dict().
float32 and float64, features, normalized-features and monitors, both game types; tile 0 held whole, tile 1 all active, the
rest mixed lane by lane."""
import numpy as np
import pytest

import bearingref as br
from lockstep import sfa  # noqa: F401  (the fixture)
from sfcompare import compare_state
from test_gpu_bearing_columns import GAMETYPES, _finish, _hold, _make, _noop, _same_inputs, _spawn_fam, _spawn_ref, _World

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def world(oracle_mod):
    return _World(oracle_mod)


@pytest.fixture(scope="module")
def table():
    return []  # (_hold files its figures here; test_gpu_bearing_columns.py prints its own table)


def _mask(n, seed):
    m = np.random.default_rng(seed).random(n) < 0.5
    m[:64] = False  # tile 0 held whole
    m[64:128] = True  # tile 1 all active: the hold kernels leave it alone
    return m


CASES = [("features", "f32"), ("features", "f64"), ("normalized-features", "f32"), ("normalized-features", "f64"), ("monitors", "f32")]


@pytest.mark.parametrize("ot,dt", CASES)
@pytest.mark.parametrize("g", GAMETYPES)
def test_held_rows_of_unplayed_and_of_played_states(sfa, world, table, g, ot, dt):
    n = world.n
    env = _make(sfa, g, world.base(g, n), obs_type=ot, obs_dtype=torch.float64 if dt == "f64" else torch.float32)
    active = _mask(n, 7)
    played = np.zeros(n, np.int64)  # ticks each lane has played: which of the oracle's snapshots it is in
    for call, (m, case) in enumerate(((active, "step_where, held at time 0 (device libm)"),
                                      (~active, "step_where, held at time 34 (global table)"))):
        buf = torch.full((n, env.obs_dim), 7.0, dtype=env.obs_dtype, device=env.device)
        out = (buf,) + tuple(env._alloc()[1:])
        env.step_where(_noop(env), torch.from_numpy(m).to(env.device), out=out)
        played += m
        obs, sd = buf.cpu().numpy(), env.state_dict()
        assert (np.asarray(sd["time"]) == 34 * played).all()
        for t in (0, 1):
            lanes = np.flatnonzero(played == t)
            if len(lanes):
                bad = compare_state(sd, world.snaps[g][t][lanes], lanes=lanes)
                assert not bad, (case, t, bad)
                _same_inputs(sd, world.snaps[g][t], lanes)
        held = np.flatnonzero(~m)
        assert (played[held] == call).all() and len(held) > n // 3
        _hold(table, case, g, ot, obs[held], sd, world.ref(g, call), held % world.P,
              tuple(x[held] for x in world.fam(n)), lanes=held)
        # ... and the active lanes' rows are the step's own, one tick on
        act = np.flatnonzero(m)
        _hold(table, case + ": the active lanes", g, ot, obs[act], sd, world.ref(g, 1), act % world.P,
              tuple(x[act] for x in world.fam(n)), lanes=act)
    assert (played == 1).all()
    _finish(env)


@pytest.mark.parametrize("ot,dt", [("features", "f32"), ("features", "f64"), ("normalized-features", "f64")])
@pytest.mark.parametrize("g", GAMETYPES)
def test_ref_reset_obs_applies_to_a_held_game_that_has_not_been_played(sfa, table, g, ot, dt):
    n = 640
    env = sfa.SFVecEnv(n, gametype=g, obs_type=ot, obs_dtype=torch.float64 if dt == "f64" else torch.float32, spawn_stride=3,
                       ref_reset_obs=True)
    first = env.reset().clone()
    assert not bool(first[:, 6:9].any())  # (the flag: the reference's zeros)
    active = _mask(n, 9)
    held = np.flatnonzero(~active)
    m = torch.from_numpy(active).to(env.device)
    buf = torch.full((n, env.obs_dim), 7.0, dtype=env.obs_dtype, device=env.device)
    env.step_where(_noop(env), m, out=(buf,) + tuple(env._alloc()[1:]))
    assert buf[~m].cpu().numpy().tobytes() == first[~m].cpu().numpy().tobytes()  # time 0: the row reset() wrote, zeros included
    assert bool((buf[m][:, 6:8] != 0).any())
    assert (env.get_field("time") == 34 * active).all()
    # the same lanes, held again after their first tick: the bearings of their state
    env.step_where(_noop(env), ~m)
    env.step_where(_noop(env), m, out=(buf,) + tuple(env._alloc()[1:]))
    sd = env.state_dict()
    assert (np.asarray(sd["time"])[held] == 34).all()
    _hold(table, "step_where, REF_RESET_OBS, held after one tick", g, ot, buf.cpu().numpy()[held], sd, _spawn_ref(sd, held),
          np.arange(len(held)), _spawn_fam(len(held)), lanes=held)
    _finish(env)
