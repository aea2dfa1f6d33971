"""tests/lockstep.py held to account, on the CPU: the harness that holds the step kernel to the oracle must pass a batch that
is right and fail one that is wrong in a single bit -- of an observation, a reward, a flag, any state field, at any tick whose
state it was asked to fetch, in any lane it was asked to look at -- and each play mode must go through the entry point it
names.  The batch is a stand-in for SFVecEnv played by the oracle itself (StubEnv): right by construction; the wrong bits are
put into what play() returned.

Inputs: fuzz_sparse at 64 lanes from default_rng(5), both game types, six ticks of random actions; after them the state has
live missiles and live shells (asserted), so that every one of the 30 fields compare_state reads has an element to change."""
import functools

import numpy as np
import pytest

from lockstep import OBS_RULES, Ticks, check_ticks, every, fuzz_sparse, load_state, n_actions, oracle_trace, play, same_bytes
from sfcompare import EXACT_F_FIELDS, INT_FIELDS, compare_state, snapshots_to_fields

torch = pytest.importorskip("torch")

GAMETYPES = ["youturn", "autoturn"]
N, T = 64, 6
# the fields state_dict has and compare_state reads
FIELDS = sorted([h for h, _ in INT_FIELDS + EXACT_F_FIELDS] + ["flags", "ship_angle", "fort_angle", "fort_last_angle", "stats", "missile_mask",
                                                              "shell_mask", "missile_x", "missile_y", "missile_angle", "shell_x",
                                                              "shell_y", "shell_vx", "shell_vy"])
assert len(FIELDS) == 30


class StubEnv:
    """SFVecEnv's stepping surface with the oracle behind it: CPU tensors, float32-rounded rows (or the float64 ones), int32
    rewards, uint8 flags; state_dict() is the oracle's snapshots as fields.  `calls` records the entry points used."""
    device = torch.device("cpu")

    def __init__(self, O, gametype, base, pv, f64=False):
        self.num_envs = len(base)
        self.orc = O.OracleVecEnv(gametype, self.num_envs)
        self.orc.load_snapshots(base, pv)
        self.obs_dim, self.obs_dtype = self.orc.obs_dim, torch.float64 if f64 else torch.float32
        self.n_actions = n_actions(gametype)
        self.calls, self.fields, self.drawn = [], {}, []
        self.rng = np.random.default_rng(77)
        self.events = self.rollout_events = None

    def set_field(self, name, value):
        self.fields[name] = np.array(value)

    def enable_events(self):
        self.calls.append("enable_events")
        self.events = torch.zeros(self.num_envs, dtype=torch.int32)
        return self.events

    def _tick(self, actions, out):
        obs, rew, done, info = self.orc.step(actions.numpy().astype(np.int32))
        if self.events is not None:  # (written in place, as the launch does: play() has to copy the row before the next tick)
            self.events.copy_(torch.from_numpy(self.orc.events().view(np.int32)))
        res = (torch.from_numpy(obs).to(self.obs_dtype), torch.from_numpy(rew), torch.from_numpy(done.astype(np.uint8)),
               torch.from_numpy(info.astype(np.uint8)))
        if out is None:
            return res
        for dst, src in zip(out, res):
            dst.copy_(src)
        return out

    def step_tensors(self, actions, out=None):
        self.calls.append("step_tensors")
        return self._tick(actions, out)

    def step_sampled(self, out=None, actions_out=None):
        self.calls.append("step_sampled")
        a = torch.from_numpy(self.rng.integers(0, self.n_actions, self.num_envs).astype(np.uint8))
        self.drawn.append(a.numpy().copy())
        actions_out.copy_(a)
        return self._tick(a, out)

    def rollout(self, actions):
        self.calls.append(("rollout", tuple(actions.shape)))
        rows, words = [], []
        for a in actions:
            rows.append(self._tick(a, None))
            words.append(None if self.events is None else self.events.clone())
        self.rollout_events = None if self.events is None else torch.stack(words)  # (a fused launch's own [K, N] buffer)
        return tuple(torch.stack(x) for x in zip(*rows))

    def state_dict(self):
        self.calls.append("state_dict")
        return snapshots_to_fields(self.orc.snapshots())

    def check_actions(self):
        self.calls.append("check_actions")

    def check_state(self):
        self.calls.append("check_state")

    def close(self):
        pass


@functools.lru_cache(maxsize=None)
def _case_cached(O, gametype):
    rng = np.random.default_rng(5)
    base, pv = fuzz_sparse(O, gametype, N, rng)
    acts = rng.integers(0, n_actions(gametype), (T, N)).astype(np.uint8)
    trace = oracle_trace(O, gametype, base, pv, acts)
    ticks = play(StubEnv(O, gametype, base, pv), acts, "step", every(1))
    ticks64 = play(StubEnv(O, gametype, base, pv, f64=True), acts, "step", every(1))
    return base, pv, acts, trace, ticks, ticks64


@pytest.fixture(params=GAMETYPES)
def case(request, oracle_mod):
    """(base, prev_vlner, actions, the oracle's trace, a faithful float32 play, a faithful float64 play): computed once,
    shared, never changed -- the tests change copies."""
    return (request.param,) + _case_cached(oracle_mod, request.param)


def _changed(ticks, name, index, change):
    """A copy of `ticks` with one element of one output array changed."""
    x = getattr(ticks, name).copy()
    x[index] = change(x[index])
    return ticks._replace(**{name: x})


def _with_state(ticks, t, field, index, change):
    """A copy of `ticks` with one element of one field of the state after tick t changed."""
    sd = {k: np.array(v) for k, v in ticks.states[t].items()}
    sd[field][index] = change(sd[field][index])
    return ticks._replace(states={**ticks.states, t: sd})


def _fails(ticks, trace, rule, where, lanes=None):
    with pytest.raises(AssertionError) as e:
        check_ticks(ticks, trace, rule, lanes)
    assert e.value.args[0][:2] == where, e.value.args[0]  # the tick and what differed


# ---------------------------------------------------------------- a faithful batch passes

@pytest.mark.parametrize("mode", ["step", "sampled", "fused"])
def test_a_faithful_batch_passes_under_every_rule_and_reaches_the_modes_entry_point(oracle_mod, case, mode):
    gametype, base, pv, acts, _, _, _ = case
    for f64 in (False, True):
        env = StubEnv(oracle_mod, gametype, base, pv, f64)
        load_state(env, base, pv, extra={"ep_return": np.arange(N)})
        want = dict(snapshots_to_fields(base), prev_vlner=np.asarray(pv, np.int32), ep_return=np.arange(N))
        assert sorted(env.fields) == sorted(want) and all(np.array_equal(env.fields[k], want[k]) for k in want)
        ticks = play(env, acts, mode, every(T) if mode == "fused" else every(2), check_state=True)
        assert sorted(ticks.states) == ([T - 1] if mode == "fused" else [1, 3, 5])
        if mode == "step":
            assert env.calls.count("step_tensors") == T and np.array_equal(ticks.played, acts)
        elif mode == "sampled":  # the oracle is given what the lanes drew, not `acts`
            assert env.calls.count("step_sampled") == T and "step_tensors" not in env.calls
            assert np.array_equal(ticks.played, np.array(env.drawn)) and not np.array_equal(ticks.played, acts)
            with pytest.raises(AssertionError):
                check_ticks(ticks, oracle_trace(oracle_mod, gametype, base, pv, acts), "rounded_f32_bits")
        else:
            assert env.calls.count(("rollout", (T, N))) == 1 and "step_tensors" not in env.calls
        assert env.calls[-2:] == ["check_actions", "check_state"]
        trace = oracle_trace(oracle_mod, gametype, base, pv, ticks.played)
        for rule in OBS_RULES:
            if (rule == "f32_bits" and f64) or (rule == "close_f64" and not f64):
                continue  # (a rule for rows of the other width)
            check_ticks(ticks, trace, rule)
        check_ticks(ticks, trace, lambda a, b: np.ones(a.shape, bool))
        assert ticks.obs.dtype == (np.float64 if f64 else np.float32) and ticks.reward.dtype == np.int32
        assert ticks.done.dtype == np.uint8 and ticks.info.dtype == np.uint8


def test_play_without_check_state_and_into_a_callers_arena(oracle_mod, case):
    gametype, base, pv, acts, trace, ticks, _ = case
    env = StubEnv(oracle_mod, gametype, base, pv)
    arena = (torch.zeros(N + 7, env.obs_dim), torch.zeros(N + 7, dtype=torch.int32), torch.zeros(N + 7, dtype=torch.uint8),
             torch.zeros(N + 7, dtype=torch.uint8))
    got = play(env, acts, "step", every(1), out=tuple(b[:N] for b in arena))
    assert "check_state" not in env.calls and env.calls[-1] == "check_actions"
    same_bytes(got, ticks)
    assert np.array_equal(arena[1][:N].numpy(), ticks.reward[-1]) and not any(b[N:].any() for b in arena)


def test_a_trace_of_another_length_fails(case):
    _, _, _, _, trace, ticks, _ = case
    with pytest.raises(AssertionError):
        check_ticks(ticks, trace[:-1], "f32_bits")


# ---------------------------------------------------------------- every kind of wrong bit fails

def test_one_float32_ulp_in_one_cell_fails_the_bits_rules(case):
    _, _, _, _, trace, ticks, _ = case
    bad = _changed(ticks, "obs", (4, 17, 1), lambda v: np.nextafter(v, np.float32(np.inf)))
    _fails(bad, trace, "f32_bits", (4, "obs"))
    _fails(bad, trace, "rounded_f32_bits", (4, "obs"))
    check_ticks(bad, trace, "close_f32")  # (an ulp is inside the tolerance of the rule that has one)


def test_3e_9_relative_in_one_cell_fails_the_float64_rule(case):
    _, _, _, _, trace, _, ticks64 = case
    t, c = 2, 1  # ship x: hundreds
    i = int(np.flatnonzero(np.abs(ticks64.obs[t, :, c]) > 1)[0])
    _fails(_changed(ticks64, "obs", (t, i, c), lambda v: v * (1 + 3e-9)), trace, "close_f64", (t, "obs"))
    check_ticks(_changed(ticks64, "obs", (t, i, c), lambda v: v * (1 + 3e-10)), trace, "close_f64")


def test_a_callable_rule_is_asked(case):
    _, _, _, _, trace, ticks, _ = case

    def rule(a, b):
        ok = np.ones(a.shape, bool)
        ok[5, 3] = False
        return ok

    with pytest.raises(AssertionError) as e:
        check_ticks(ticks, trace, rule)
    assert e.value.args[0][:3] == (0, "obs", [[5, 3]])


def test_a_reward_off_by_one_fails(case):
    _, _, _, _, trace, ticks, _ = case
    _fails(_changed(ticks, "reward", (3, 63), lambda v: v + 1), trace, "f32_bits", (3, "reward"))


@pytest.mark.parametrize("name", ["done", "info"])
def test_a_flipped_flag_byte_fails(case, name):
    _, _, _, _, trace, ticks, _ = case
    _fails(_changed(ticks, name, (5, 0), lambda v: v ^ 1), trace, "f32_bits", (5, name))


def _element(sd, field, lane=None):
    """(index, change): one element of `field` that compare_state reads -- a live slot of a projectile field -- and the
    smallest change of it that must show: a float one ulp, an integer or a mask one bit, a shell's float 1e-6 (its
    tolerance is 1e-9)."""
    x = np.asarray(sd[field])
    lanes = range(x.shape[-1]) if lane is None else [lane]
    if x.ndim == 1:
        index = (lanes[0],)
    elif field == "stats":
        index = (0, lanes[0])
    else:
        mask = sd["missile_mask" if field.startswith("missile") else "shell_mask"]
        live = [(s, i) for i in lanes for s in range(20) if (int(mask[i]) >> s) & 1]
        assert live, (field, "no live slot")  # (never skipped: the inputs have live missiles and shells)
        index = live[0]
    if field.startswith("shell_") and field != "shell_mask":
        return index, lambda v: v + 1e-6
    if x.dtype.kind == "f":
        return index, lambda v: np.nextafter(v, x.dtype.type(np.inf))
    return index, lambda v: v ^ 1


@pytest.mark.parametrize("field", FIELDS)
def test_one_element_of_each_state_field_fails(case, field):
    _, _, _, _, trace, ticks, _ = case
    sd = ticks.states[T - 1]
    assert sorted(sd) == FIELDS and not compare_state(sd, trace[T - 1][4])
    assert sd["missile_mask"].any() and sd["shell_mask"].any()  # live missiles and shells after the six ticks
    index, change = _element(sd, field)
    _fails(_with_state(ticks, T - 1, field, index, change), trace, "f32_bits", (T - 1, "state"))


def test_a_changed_state_shows_only_at_a_tick_state_at_selects(oracle_mod, case):
    gametype, base, pv, acts, trace, ticks, _ = case
    bad = _with_state(ticks, 3, "vlner", (9,), lambda v: v ^ 1)
    _fails(bad, trace, "f32_bits", (3, "state"))
    for sel, seen in ((every(2), True), (lambda t: t == 2, False), (None, False)):
        got = play(StubEnv(oracle_mod, gametype, base, pv), acts, "step", sel)
        assert (3 in got.states) == seen
        got = got._replace(states={t: bad.states[t] for t in got.states})  # the same wrong batch, fetched at other ticks
        if seen:
            _fails(got, trace, "f32_bits", (3, "state"))
        else:
            check_ticks(got, trace, "f32_bits")
    with pytest.raises(AssertionError):  # a fused launch has no state in between to fetch
        play(StubEnv(oracle_mod, gametype, base, pv), acts, "fused", every(2))


# ---------------------------------------------------------------- the event words

@pytest.mark.parametrize("mode", ["step", "sampled", "fused"])
def test_event_words_are_carried_by_every_mode_and_one_bit_of_one_lane_fails(oracle_mod, case, mode):
    from spacefortress_amd._lib import EVENT_NAMES

    gametype, base, pv, acts, _, plain, _ = case
    env = StubEnv(oracle_mod, gametype, base, pv)
    ticks = play(env, acts, mode, None, events=True)
    assert env.calls[0] == "enable_events" and ticks.events.dtype == np.uint32 and ticks.events.shape == (T, N)
    assert plain.events is None  # (not asked for: not there, and check_ticks does not look)
    trace = oracle_trace(oracle_mod, gametype, base, pv, ticks.played)
    assert all(len(tr) == 6 and tr[5].dtype == np.uint32 and tr[5].shape == (N,) for tr in trace)
    check_ticks(ticks, trace, "f32_bits")  # an untouched copy passes
    check_ticks(ticks._replace(events=ticks.events.copy()), trace, "f32_bits")
    assert len({int(w) for w in ticks.events.reshape(-1)}) > 8 and not (ticks.events >> 22).any()  # (the run has events to get wrong)
    # one bit of one lane of one tick: set where it is clear, cleared where it is set, flipped -- every one of the 22 bits,
    # at a tick and a lane that move with the bit
    for k, bit in enumerate(sorted(EVENT_NAMES)):
        t, lane = k % T, (7 * k + 3) % N
        w = int(ticks.events[t, lane])
        for change in (lambda v: v | np.uint32(bit), lambda v: v & ~np.uint32(bit), lambda v: v ^ np.uint32(bit)):
            if int(change(np.uint32(w))) == w:
                check_ticks(_changed(ticks, "events", (t, lane), change), trace, "f32_bits")
                continue
            with pytest.raises(AssertionError) as e:
                check_ticks(_changed(ticks, "events", (t, lane), change), trace, "f32_bits")
            where = e.value.args[0]
            assert where[:3] == (t, "events", [lane]), where
            got, want = where[3][0]  # the names on both sides: they differ by the changed bit's name
            assert set(got) ^ set(want) == {EVENT_NAMES[bit]}, where
    # a bit the oracle has and the batch has not, found by name: the first set bit of the run
    t, lane = [int(x) for x in np.argwhere(ticks.events != 0)[0]]
    _fails(_changed(ticks, "events", (t, lane), lambda v: v & (v - np.uint32(1))), trace, "f32_bits", (t, "events"))
    # a trace without words cannot vouch for a batch that has them
    with pytest.raises(AssertionError):
        check_ticks(ticks, [tr[:5] for tr in trace], "f32_bits")
    # lanes outside a selection are not looked at
    lanes = np.array([3, 4, 20, 41, 63])
    sub = oracle_trace(oracle_mod, gametype, base, pv, ticks.played, lanes)
    check_ticks(_changed(ticks, "events", (2, 5), lambda v: v ^ np.uint32(1)), sub, "f32_bits", lanes)
    _fails(_changed(ticks, "events", (2, 41), lambda v: v ^ np.uint32(1)), sub, "f32_bits", (2, "events"), lanes)
    # and same_bytes reads them where both sides have them
    same_bytes(ticks, ticks)
    with pytest.raises(AssertionError):
        same_bytes(ticks, _changed(ticks, "events", (T - 1, N - 1), lambda v: v ^ np.uint32(0x200000)))


# ---------------------------------------------------------------- selection

def test_lanes_outside_the_selection_are_not_looked_at(oracle_mod, case):
    gametype, base, pv, acts, _, ticks, _ = case
    lanes = np.array([3, 4, 20, 41, 63])
    trace = oracle_trace(oracle_mod, gametype, base, pv, acts, lanes)
    check_ticks(ticks, trace, "f32_bits", lanes)
    ulp = lambda v: np.nextafter(v, np.float32(np.inf))
    for lane, seen in ((5, False), (41, True)):
        sd = ticks.states[2]
        cases = [(_changed(ticks, "obs", (2, lane, 1), ulp), "obs"), (_changed(ticks, "reward", (2, lane), lambda v: v + 1), "reward"),
                 (_changed(ticks, "done", (2, lane), lambda v: v ^ 1), "done"), (_changed(ticks, "info", (2, lane), lambda v: v ^ 1), "info"),
                 (_with_state(ticks, 2, "fort_timer", (lane,), lambda v: v ^ 1), "state"),
                 (_with_state(ticks, 2, "stats", (4, lane), lambda v: v ^ 1), "state")]
        assert sd["time"].shape == (N,)
        for bad, what in cases:
            if seen:
                _fails(bad, trace, "f32_bits", (2, what), lanes)
            else:
                check_ticks(bad, trace, "f32_bits", lanes)


# ---------------------------------------------------------------- same_bytes

def test_same_bytes_fails_on_one_output_byte_and_on_one_state_byte(case):
    _, _, _, _, _, ticks, ticks64 = case
    same_bytes(ticks, ticks)
    same_bytes(ticks, ticks._replace(played=ticks.played + 1))  # (what was played is an input, not an output)
    for name in ("obs", "reward", "done", "info"):
        x = getattr(ticks, name).copy()
        x.view(np.uint8).reshape(-1)[-1] ^= 1
        with pytest.raises(AssertionError) as e:
            same_bytes(ticks, ticks._replace(**{name: x}))
        assert e.value.args[0][:2] == (T - 1, name)
    for field in ("shell_vy", "flags"):  # a slot that is not live counts too: the bytes, not the game
        sd = {k: np.array(v) for k, v in ticks.states[1].items()}
        sd[field].view(np.uint8).reshape(-1)[0] ^= 1
        with pytest.raises(AssertionError) as e:
            same_bytes(ticks, ticks._replace(states={**ticks.states, 1: sd}))
        assert e.value.args[0][:2] == (1, field)
    with pytest.raises(AssertionError):
        same_bytes(ticks, ticks._replace(states={t: sd for t, sd in ticks.states.items() if t}))
    with pytest.raises(AssertionError):
        same_bytes(ticks, ticks64)
    assert isinstance(ticks, Ticks)
