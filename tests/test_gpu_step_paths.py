"""Every stepping path shows the hooks what a plain step of a twin batch shows them.

The paths: SFVecEnv.step_tensors / step_repeat, FrameStack.step, DeviceRollout.step (features, behind SFVecNormalize, stacked
images), FrameRollout.step, SFVecNormalize.step_tensors -- with frame_skip 1 and 3.  Each steps its batch 12 agent steps on the
same action rows as a TWIN: a bare batch of the same kind stepped by step_tensors (frame_skip 1) or step_repeat(a, 3).  Compared
bit for bit: the actions and the engine's int reward, done and info handed to SFVecEnv._stepped, env.last_ticks, env.events, the
episode log's records and histogram, the recording's actions and sums, the duration log's vectors.

The hooks: the episode log and events always.  `ends`: the clocks are set so that games end inside the run (frame_skip 3: also
inside a window); with frame_skip 1 a duration log follows.  `recording` (frame_skip 1): a recording needs a batch nothing has
edited, so nobody finishes in its 12 ticks.  130 envs for features (two tiles and a partial one), 65 for images.

Then the refusals (a duration log or a recording with frame_skip > 1, through every wrapper) and bad actions through every path.
"""
import numpy as np
import pytest

from lockstep import sfa

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

T, S = 12, 4
N_FEATURES, N_IMAGE = 130, 65
PATHS = ("step_tensors", "step_repeat", "FrameStack", "DeviceRollout", "DeviceRollout+VecNormalize", "DeviceRollout(num_stack)",
         "FrameRollout", "SFVecNormalize")
IMAGE_PATHS = ("FrameStack", "DeviceRollout(num_stack)", "FrameRollout")
CASES = [(1, "ends"), (1, "recording"), (3, "ends")]


def _n(path):
    return N_IMAGE if path in IMAGE_PATHS else N_FEATURES


def _actions(n, device):
    return torch.from_numpy(np.random.default_rng(n).integers(0, 5, (T, n)).astype(np.uint8)).to(device)


def _make_env(sfa, image, fs, hook, env_fs):
    """A new batch with every hook the case allows; `ends`: the lanes finish 1 .. 41 ticks from now, every 7th nowhere near it."""
    n = N_IMAGE if image else N_FEATURES
    env = sfa.SFVecEnv(n, gametype="youturn", obs_type="image" if image else "features", spawn_stride=1, frame_skip=env_fs)
    if hook == "ends":
        clock = (180000 - 34 * (1 + np.arange(n) % 41)).astype(np.int32)
        clock[::7] = 34 * 100
        env.set_field("time", clock)
        if fs == 1:
            env.enable_durations()
    else:
        env.start_recording()
    env.enable_events()
    env.enable_episode_log(capacity=512, hist=(-60, 100))
    return env


def _stepper(sfa, path, env, fs):
    """(callable taking (t, actions), the objects to keep alive) for one path"""
    if path == "step_tensors":
        return (lambda t, a: env.step_tensors(a)), None
    if path == "step_repeat":
        return (lambda t, a: env.step_repeat(a, fs)), None
    if path == "FrameStack":
        w = sfa.FrameStack(env, S)
        return (lambda t, a: w.step(a)), w
    if path == "DeviceRollout":
        w = sfa.DeviceRollout(env, T)
    elif path == "DeviceRollout+VecNormalize":
        w = sfa.DeviceRollout(sfa.SFVecNormalize(env), T)
    elif path == "DeviceRollout(num_stack)":
        w = sfa.DeviceRollout(env, T, num_stack=S)
    elif path == "FrameRollout":
        w = sfa.FrameRollout(env, T, num_stack=S)
    else:
        w = sfa.SFVecNormalize(env)
        return (lambda t, a: w.step_tensors(a)), w
    return (lambda t, a: w.step(t, a)), w


def _run(sfa, path, fs, hook, twin=False):
    """Everything the hooks of a batch stepped through `path` saw, as host data"""
    image = path in IMAGE_PATHS
    env = _make_env(sfa, image, fs, hook, 1 if (twin or path == "step_repeat") else fs)
    acts = _actions(env.num_envs, env.device)
    seen = []
    inner = env._stepped

    def spy(actions, rew, done, info):
        seen.append([x.reshape(-1).to(torch.int64).cpu().numpy().copy() for x in (actions, rew, done, info)])
        inner(actions, rew, done, info)

    env._stepped = spy
    if twin:
        step, keep = ((lambda t, a: env.step_tensors(a)) if fs == 1 else (lambda t, a: env.step_repeat(a, fs))), None
    else:
        step, keep = _stepper(sfa, path, env, fs)
    ticks, events = [], []
    for t in range(T):
        step(t, acts[t])
        ticks.append(None if env.last_ticks is None else env.last_ticks.cpu().numpy().copy())
        events.append(env.events.cpu().numpy().copy())
    torch.cuda.synchronize()
    assert len(seen) == T
    out = {"seen": seen, "ticks": ticks, "events": events, "records": env._episodes.drain(), "hist": env._episodes.histogram(),
           "rows_seen": env._episodes.rows_seen}
    if env._rec is not None:
        rp = env._rec.replay(env)
        out["recording"] = (rp.actions, rp.returns, rp.kills, rp.dones, rp.digest)
    if env._durations is not None:
        out["durations"] = {}
        for k in ("thrust_durations", "shot_durations", "shot_intervals_invul", "shot_intervals_vul"):
            v, c = (x.cpu().numpy() for x in env._durations.get(k))
            out["durations"][k] = (c, np.where(np.arange(v.shape[1])[None, :] < c[:, None], v, 0))
    del keep
    env.close()
    return out


_twins = {}


def _twin(sfa, image, fs, hook):
    """the plain run every path of one kind is held against: made once, never changed"""
    key = (image, fs, hook)
    if key not in _twins:
        _twins[key] = _run(sfa, IMAGE_PATHS[0] if image else "step_tensors", fs, hook, twin=True)
    return _twins[key]


@pytest.mark.parametrize("fs,hook", CASES)
@pytest.mark.parametrize("path", PATHS)
def test_every_path_shows_the_hooks_what_the_plain_step_shows(sfa, path, fs, hook):
    got = _run(sfa, path, fs, hook)
    want = _twin(sfa, path in IMAGE_PATHS, fs, hook)
    done = np.array([s[2] for s in want["seen"]])
    if hook == "ends":
        assert done.any(), "no env finished inside the run"
        if fs > 1:
            last = np.array(want["ticks"])
            assert (last == fs).any() and ((last < fs) & (done != 0)).any(), "no env finished inside a window"
    for t in range(T):
        for k, name in enumerate(("actions", "reward", "done", "info")):
            assert np.array_equal(got["seen"][t][k], want["seen"][t][k]), (t, name)
        assert np.array_equal(got["events"][t], want["events"][t]), t
        if fs > 1:
            assert np.array_equal(got["ticks"][t], want["ticks"][t]), t
        else:  # (step_repeat(a, 1) says one tick each; the plain step says nothing)
            assert got["ticks"][t] is None or (got["ticks"][t] == 1).all(), t
    assert any(e.any() for e in want["events"])
    assert got["rows_seen"] == want["rows_seen"] == T
    for k, v in want["records"].items():
        assert np.array_equal(got["records"][k], v), k
    assert len(want["records"]["env"]) == int(done.sum())
    assert np.array_equal(got["hist"], want["hist"])
    assert ("recording" in want) == (hook == "recording") and ("durations" in want) == (hook == "ends" and fs == 1)
    if "recording" in want:
        for g, w in zip(got["recording"][:4], want["recording"][:4]):
            assert np.array_equal(g, w)
        assert got["recording"][4] == want["recording"][4] and want["recording"][0].shape == (T, _n(path))
    if "durations" in want:
        pushed = 0
        for k, (c, v) in want["durations"].items():
            assert np.array_equal(got["durations"][k][0], c) and np.array_equal(got["durations"][k][1], v), k
            pushed += int(c.sum())
        assert pushed > 0


# ---------------------------------------------------------------------------------------------------------------
# refusals
WRAPPERS = PATHS[2:]


@pytest.mark.parametrize("path", PATHS)
def test_a_duration_log_refuses_an_action_repeat(sfa, path):
    n = _n(path)
    env = sfa.SFVecEnv(n, obs_type="image" if path in IMAGE_PATHS else "features", frame_skip=1 if path == "step_repeat" else 3)
    step, keep = _stepper(sfa, path, env, 3)
    a = torch.ones(n, dtype=torch.uint8, device=env.device)
    env.enable_durations()
    with pytest.raises(RuntimeError, match="duration log"):
        step(0, a)
    env._durations = None
    step(0, a)  # (and goes on without it)
    del keep
    env.close()


@pytest.mark.parametrize("path", PATHS)
def test_a_recording_refuses_an_action_repeat(sfa, path):
    n = _n(path)
    a = torch.ones(n, dtype=torch.uint8, device="cuda")
    if path == "step_repeat":
        env = sfa.SFVecEnv(n)
        env.start_recording()
        with pytest.raises(RuntimeError, match="recording"):
            env.step_repeat(a, 3)
        env.step_repeat(a, 1)  # (sf_step: a replay file can hold it)
        assert env._rec.replay(env).actions.shape == (1, n)
        env.close()
        return
    # a batch made with frame_skip > 1 starts no recording, whatever wraps it
    env = sfa.SFVecEnv(n, obs_type="image" if path in IMAGE_PATHS else "features", frame_skip=3)
    step, keep = _stepper(sfa, path, env, 3)
    inner = getattr(keep, "venv", None) or getattr(keep, "env", None) or env
    inner = getattr(inner, "venv", inner)
    assert inner is env
    with pytest.raises(RuntimeError, match="frame_skip"):
        inner.start_recording()
    assert env._rec is None
    step(0, a)
    assert env._rec is None and bool((env.last_ticks == 3).all())
    del keep
    env.close()


# ---------------------------------------------------------------------------------------------------------------
# bad actions
@pytest.mark.parametrize("fs", [1, 3])
@pytest.mark.parametrize("path", PATHS)
def test_bad_actions_are_refused_in_front_of_the_launch(sfa, path, fs):
    n = _n(path)
    env = sfa.SFVecEnv(n, obs_type="image" if path in IMAGE_PATHS else "features", frame_skip=1 if path == "step_repeat" else fs)
    step, keep = _stepper(sfa, path, env, fs)
    seen = []
    inner = env._stepped
    env._stepped = lambda *a: (seen.append(1), inner(*a))
    good = torch.ones(n, dtype=torch.uint8, device=env.device)
    if path.startswith("DeviceRollout") or path == "FrameRollout":
        step(0, good.float())  # (the rollout takes what the policy gives: .long())
        assert len(seen) == 1
    else:
        with pytest.raises(TypeError, match="uint8, int32 or int64"):
            step(0, good.float())
    for a in (good.cpu(), torch.ones(n + 1, dtype=torch.uint8, device=env.device), good[:-1]):
        with pytest.raises(ValueError, match="%d elements" % n):
            step(0, a)
    assert len(seen) <= 1
    step(0, good)
    del keep
    env.close()
