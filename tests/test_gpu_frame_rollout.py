"""FrameRollout / sf_gather_stacks on the device: the image rollout storage that keeps every frame once, held byte for byte to
the stacked storage (DeviceRollout(env, T, num_stack=4)) and to the numpy statement of the stack rule (tests/framestore_np.py).
Every comparison is torch.equal: the feature has no arithmetic."""
import numpy as np
import pytest

from framestore_np import gather
from lockstep import sfa

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
FRAME = 84 * 84


def _dev_store(frames_np, layout):
    """[rows, n, 7056] on the host -> (device tensor in `layout`, env_stride, row_stride)"""
    rows, n = frames_np.shape[:2]
    t = torch.from_numpy(frames_np).cuda()
    if layout == "time":
        return t, FRAME, n * FRAME
    return t.permute(1, 0, 2).contiguous(), rows * FRAME, FRAME


def _as(model_u8, dtype, dev):
    t = torch.from_numpy(model_u8).to(dev)
    return t if dtype == torch.uint8 else t.to(dtype)


# 1 ------------------------------------------------------------------ the kernel against the model
@pytest.mark.parametrize("layout", ["time", "env"])
@pytest.mark.parametrize("S", [1, 2, 4])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 96, 4097])
def test_gather_kernel_equals_the_model(sfa, n, S, layout):
    from spacefortress_amd import frame_rollout as fr

    dev = torch.device("cuda")
    T = 3 if n > 1000 else 6
    rows = T + S
    rng = np.random.default_rng(1000 * n + 10 * S + (layout == "env"))
    frames_np = rng.integers(1, 256, (rows, n, FRAME), dtype=np.uint8)  # (no zero pixels: a zeroed slot cannot pass for a frame)
    starts_np = (rng.random((rows, n)) < 0.3).astype(np.uint8)
    frames, es, rs = _dev_store(frames_np, layout)
    starts = torch.from_numpy(starts_np).to(dev)
    stream = torch.cuda.current_stream().cuda_stream

    def run(index, m, step, dtype):
        out = torch.full((m, S, 84, 84), 7, dtype=dtype, device=dev)
        fr.gather_stacks(frames.data_ptr(), starts.data_ptr(), n, rows, S, es, rs, index, m, step, out, stream)
        return out

    assert fr.gather_errors(dev, clear=True) >= 0
    # NULL index: the n stacks of one step, every step, the three output types
    for t, dtype in zip(range(T + 1), [torch.uint8, torch.float16, torch.float32] * 3):
        want = gather(frames_np, starts_np, S, None, t)[0].reshape(n, S, 84, 84)
        assert torch.equal(run(None, n, t, dtype), _as(want, dtype, dev)), (t, dtype)
    # index lists: random with repeats, reversed, single, empty; int32 and int64
    m = min(T * n, 300)
    rand = rng.integers(0, T * n, m)
    rand[m // 2:] = rand[:m - m // 2]  # every index of the first half twice
    lists = [(rand, torch.int64, torch.uint8), (rand, torch.int32, torch.float32),
             (np.arange(min(T * n, 200))[::-1].copy(), torch.int32, torch.uint8),
             (np.arange(T * n - 1, max(T * n - 150, -1), -1), torch.int64, torch.float16),
             (np.array([T * n - 1]), torch.int64, torch.uint8), (np.array([0]), torch.int32, torch.float16),
             (np.zeros(0, np.int64), torch.int64, torch.uint8), (np.zeros(0, np.int64), torch.int32, torch.float32)]
    for idx_np, itype, dtype in lists:
        idx = torch.from_numpy(np.ascontiguousarray(idx_np)).to(dev).to(itype)
        want, bad = gather(frames_np, starts_np, S, idx_np)
        assert bad == 0
        got = run(idx, len(idx_np), 0, dtype)
        assert got.shape == (len(idx_np), S, 84, 84)
        assert torch.equal(got, _as(want.reshape(-1, S, 84, 84), dtype, dev)), (len(idx_np), itype, dtype)
    assert fr.gather_errors(dev) == 0
    # out of range: a zero stack each, counted on the device, sticky until cleared
    for itype, extra in ((torch.int64, [-1, T * n, T * n + 5, -(1 << 40), 1 << 40, (1 << 32) + 1]),
                         (torch.int32, [-1, T * n, T * n + 5, -(1 << 31), (1 << 31) - 1])):
        idx_np = np.concatenate([rand[:20], np.array(extra, np.int64), rand[20:40]])
        order = rng.permutation(len(idx_np))
        idx_np = idx_np[order]
        want, bad = gather(frames_np, starts_np, S, idx_np)
        assert bad == len(extra)
        for dtype in (torch.uint8, torch.float16, torch.float32):
            got = run(torch.from_numpy(idx_np).to(dev).to(itype), len(idx_np), 0, dtype)
            assert torch.equal(got, _as(want.reshape(-1, S, 84, 84), dtype, dev)), (itype, dtype)
        assert fr.gather_errors(dev) == 3 * bad
        assert fr.gather_errors(dev) == 3 * bad  # sticky
        with pytest.raises(IndexError):
            from spacefortress_amd import _lib
            _lib.check(_lib.lib().sf_gather_errors(None, 1, None))
        assert fr.gather_errors(dev) == 0


def test_gather_refuses_bad_arguments(sfa):
    from spacefortress_amd import _lib, frame_rollout as fr

    dev = torch.device("cuda")
    n, S, T = 8, 4, 2
    frames = torch.zeros((T + S, n, FRAME), dtype=torch.uint8, device=dev)
    starts = torch.zeros((T + S, n), dtype=torch.uint8, device=dev)
    out = torch.zeros((n, S, 84, 84), dtype=torch.uint8, device=dev)
    L = _lib.lib()
    args = lambda **kw: [kw.get(k, v) for k, v in (("f", frames.data_ptr()), ("s", starts.data_ptr()), ("n", n), ("rows", T + S), ("S", S),
                                                  ("es", FRAME), ("rs", n * FRAME), ("idx", None), ("it", 0), ("m", n), ("step", 0),
                                                  ("out", out.data_ptr()), ("ot", _lib.STACK_U8), ("stream", None))]
    assert L.sf_gather_stacks(*args()) == 0
    for bad in (dict(step=T + 1), dict(step=-1), dict(m=n - 1), dict(S=0), dict(S=17), dict(rows=S - 1), dict(es=FRAME - 16),
                dict(es=FRAME + 8), dict(rs=FRAME), dict(ot=3), dict(out=out.data_ptr() + 4), dict(f=frames.data_ptr() + 8),
                dict(idx=starts.data_ptr(), it=1), dict(f=None), dict(s=None)):
        assert L.sf_gather_stacks(*args(**bad)) == _lib.SF_ERR_ARG, bad
    torch.cuda.synchronize()
    with pytest.raises(TypeError):
        fr.gather_stacks(frames.data_ptr(), starts.data_ptr(), n, T + S, S, FRAME, n * FRAME, None, n, 0, out.double(), None)


# 2 ------------------------------------------------------------------ the twin against the stacked storage
def _twin_run(sfa, layout, forced, before_update=None):
    """Three rollouts of a stacked and a deduplicated storage on twin batches.  forced: {(rollout, step): lanes whose game is
    made to end ON that step (their clock is set one tick before the end on both twins)}.  before_update(k, env, ro, fro) runs
    where the trainer samples its minibatches: after compute_returns, before after_update.  -> masks [3, T + 1, N] as numpy."""
    N, T, S = 96, 14, 4
    env = sfa.SFVecEnv(N, gametype="autoturn", obs_type="image", spawn_stride=1)
    twin = sfa.SFVecEnv(N, gametype="autoturn", obs_type="image", spawn_stride=1)
    ro = sfa.DeviceRollout(env, T, num_stack=S)
    fro = sfa.FrameRollout(twin, T, num_stack=S, layout=layout)
    with pytest.raises(AttributeError, match="stack_at"):
        fro.observations
    assert torch.equal(ro.reset(), fro.reset())
    if not forced:
        for e in (env, twin):
            e.set_field("time", np.full(N, 34 * 5287, np.int32))
    g = torch.Generator(device=env.device).manual_seed(2)
    all_masks = []
    for k in range(3):
        for t in range(T):
            lanes = forced.get((k, t)) if forced else None
            if lanes is not None:
                for e in (env, twin):
                    tm = e.get_field("time").copy()
                    tm[lanes] = 34 * 5294  # one tick before Game::isGameOver
                    e.set_field("time", tm)
            a = torch.randint(0, 3, (N,), device=env.device, generator=g, dtype=torch.uint8)
            vp = torch.rand(N, 1, device=env.device, generator=g)
            o1, r1, m1 = ro.step(t, a, value_pred=vp, action_log_prob=vp * 2, state=vp * 3)
            o2, r2, m2 = fro.step(t, a, value_pred=vp, action_log_prob=vp * 2, state=vp * 3)
            assert o2.shape == (N, S, 84, 84) and o2.dtype == torch.uint8
            assert torch.equal(o1, o2), (k, t)
            assert torch.equal(r1, r2) and torch.equal(m1, m2), (k, t)
        for t in range(T + 1):
            assert torch.equal(fro.stack_at(t), ro.observations[t]), (k, t)
        for name in ("rewards", "masks", "actions", "value_preds", "action_log_probs", "states", "episode_rewards", "final_rewards"):
            assert torch.equal(getattr(ro, name), getattr(fro, name)), (k, name)
        assert ro.num_destruction == fro.num_destruction
        nv = torch.rand(N, 1, device=env.device, generator=g)
        ro.compute_returns(nv, True, 0.99, 0.95)
        fro.compute_returns(nv, True, 0.99, 0.95)
        assert torch.equal(ro.returns, fro.returns)
        all_masks.append(ro.masks[:, :, 0].cpu().numpy().copy())
        if before_update is not None:
            before_update(k, env, ro, fro)
        ro.after_update()
        fro.after_update()
        assert torch.equal(fro.stack_at(0), ro.observations[0]), k
        assert torch.equal(ro.masks[0], fro.masks[0]) and torch.equal(ro.states[0], fro.states[0])
    out = (env, twin, ro, fro, np.stack(all_masks))
    return out


@pytest.mark.parametrize("layout", ["time", "env"])
def test_twin_of_the_stacked_storage_by_play(sfa, layout):
    env, twin, ro, fro, masks = _twin_run(sfa, layout, None)
    assert (masks[:, 1:] == 0).any(), "no episode ended inside the window"
    env.close()
    twin.close()


@pytest.mark.parametrize("layout", ["time", "env"])
def test_twin_with_games_ended_on_consecutive_steps(sfa, layout):
    """A game cannot end twice within S steps by play alone: the clocks of chosen lanes are set so that they end on consecutive
    steps (A), two steps apart (B), and on the last step of a rollout and the first of the next (C)."""
    A, B, Cc = np.arange(0, 10), np.arange(10, 20), np.arange(20, 30)
    forced = {(0, 3): np.concatenate([A, B]), (0, 4): A, (0, 5): B, (0, 13): Cc, (1, 0): Cc, (1, 1): Cc,
              (2, 0): A, (2, 7): B, (2, 8): B, (2, 9): B}
    env, twin, ro, fro, masks = _twin_run(sfa, layout, forced)
    m = masks  # [rollout, step 0 .. T, env]; masks[k, t + 1] == 0: the game ended on step t
    assert (m[0, 4, A] == 0).all() and (m[0, 5, A] == 0).all() and (m[0, 6, A] == 1).all()
    assert (m[0, 4, B] == 0).all() and (m[0, 5, B] == 1).all() and (m[0, 6, B] == 0).all()
    assert (m[0, 14, Cc] == 0).all() and (m[1, 0, Cc] == 0).all() and (m[1, 1, Cc] == 0).all() and (m[1, 2, Cc] == 0).all()
    assert (m[2, 8:11][:, B] == 0).all()
    env.close()
    twin.close()


# 3 ------------------------------------------------------------------ the generators
def test_generators_equal_the_stacked_storage(sfa):
    ran = []
    env, twin, ro, fro, masks = _twin_run(sfa, "time", {(1, 3): np.arange(5), (1, 4): np.arange(5), (2, 0): np.arange(5, 9)},
                                          lambda k, env, ro, fro: ran.append(k) or _check_generators(env, ro, fro))
    assert ran == [0, 1, 2]
    env.close()
    twin.close()


def _check_generators(env, ro, fro):
    T, N = ro.rewards.shape[:2]
    for s in (ro, fro):
        s.returns[:-1] = torch.arange(T * N, device=env.device, dtype=torch.float32).view(T, N, 1)  # a unique tag per transition
    adv = ro.returns[:-1] * 2
    for k, nmb in ((11, 4), (12, 7)):  # (7: a last, shorter minibatch is not dropped -- 1344 = 7 * 192 divides; 4 * 336 too)
        torch.manual_seed(k)
        a = list(ro.feed_forward_generator(adv, nmb))
        torch.manual_seed(k)
        b = list(fro.feed_forward_generator(adv, nmb))
        assert len(a) == len(b) >= nmb
        seen = []
        for x, y in zip(a, b):
            assert len(x) == len(y) == 7
            for u, v in zip(x, y):
                assert u.shape == v.shape and u.dtype == v.dtype and torch.equal(u, v)
            seen.append(y[3][:, 0].long())
        assert torch.equal(torch.sort(torch.cat(seen)).values, torch.arange(T * N, device=env.device))
    perm = torch.randperm(T * N, device=env.device)
    u8 = [mb[0] for mb in fro.feed_forward_generator(adv, 4, perm=perm)]
    for dtype in (torch.float32, torch.float16):
        fl = [mb[0] for mb in fro.feed_forward_generator(adv, 4, obs_dtype=dtype, perm=perm)]
        for x, y in zip(u8, fl):
            assert y.dtype == dtype and torch.equal(y, x.to(dtype))
    obs_flat = ro.observations[:-1].reshape(T * N, 4, 84, 84)
    for x, p in zip(u8, perm.split(T * N // 4)):
        assert torch.equal(x, obs_flat[p])
    # recurrent: whole trajectories env by env
    for k, nmb in ((21, 3), (22, 5)):
        torch.manual_seed(k)
        a = list(ro.recurrent_generator(adv, nmb))
        torch.manual_seed(k)
        b = list(fro.recurrent_generator(adv, nmb))
        assert len(a) == len(b)
        seen = []
        for x, y in zip(a, b):
            for u, v in zip(x, y):
                assert u.shape == v.shape and u.dtype == v.dtype and torch.equal(u, v)
            seen.append(y[3][:, 0].long())
        if N % nmb == 0:
            assert torch.equal(torch.sort(torch.cat(seen)).values, torch.arange(T * N, device=env.device))
    eperm = torch.randperm(N, device=env.device)
    u8 = [mb[0] for mb in fro.recurrent_generator(adv, 3, perm=eperm)]
    f32 = [mb[0] for mb in fro.recurrent_generator(adv, 3, obs_dtype=torch.float32, perm=eperm)]
    f16 = [mb[0] for mb in fro.recurrent_generator(adv, 3, obs_dtype=torch.float16, perm=eperm)]
    for x, y, z in zip(u8, f32, f16):
        assert torch.equal(y, x.float()) and torch.equal(z, x.half())
    from spacefortress_amd import frame_rollout as fr
    assert fr.gather_errors(env.device) == 0


# 4 ------------------------------------------------------------------ graph capture
def test_captured_rollout_equals_eager_stepping(sfa):
    N, T, S = 96, 10, 4
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(5)
    acts = torch.randint(0, 3, (T, N), device=dev, generator=g, dtype=torch.uint8)
    rows = [acts[t] for t in range(T)]
    stores = []
    for captured in (False, True):
        env = sfa.SFVecEnv(N, gametype="autoturn", obs_type="image", spawn_stride=1)
        fro = sfa.FrameRollout(env, T, num_stack=S)
        fro.reset()
        env.set_field("time", np.full(N, 34 * 5290, np.int32))
        cur = []
        if captured:
            torch.cuda.synchronize()
            side = torch.cuda.Stream(device=dev)
            side.wait_stream(torch.cuda.current_stream(dev))
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.stream(side):
                with torch.cuda.graph(graph, stream=side):  # one stream, no parallel branches
                    for t in range(T):
                        fro.step(t, rows[t])
            torch.cuda.current_stream(dev).wait_stream(side)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
        else:
            for t in range(T):
                fro.step(t, rows[t])
        torch.cuda.synchronize()
        stores.append([fro.frames.clone(), fro.starts.clone(), fro.rewards.clone(), fro.masks.clone(), fro.actions.clone(),
                       fro.episode_rewards.clone(), fro.final_rewards.clone(), fro.stack_at(T).clone(), fro._cur.clone()])
        env.close()
    assert bool((stores[0][3] == 0).any()), "no episode ended inside the window"
    for x, y in zip(*stores):
        assert torch.equal(x, y)


# 5 ------------------------------------------------------------------ footprint
def test_footprint(sfa):
    N, T, S = 256, 128, 4
    env = sfa.SFVecEnv(N, gametype="autoturn", obs_type="image")
    fro = sfa.FrameRollout(env, T, num_stack=S)
    dedup = fro.nbytes()
    assert dedup == (T + S) * N * 7056 + (T + S) * N
    del fro
    ro = sfa.DeviceRollout(env, T, num_stack=S)
    assert ro.nbytes() == (T + 1) * N * S * 7056
    assert dedup * 3.9 < ro.nbytes()
    env.close()


# 6 ------------------------------------------------------------------ refusals
def test_refusals(sfa):
    sym = sfa.SFVecEnv(4)
    with pytest.raises(ValueError):
        sfa.FrameRollout(sym, 4, num_stack=4)
    with pytest.raises(ValueError):
        sfa.FrameRollout(sfa.SFVecNormalize(sym), 4, num_stack=4)
    raw = sfa.SFVecEnv(4, obs_type="image-raw")
    with pytest.raises(ValueError):
        sfa.FrameRollout(raw, 4, num_stack=4)
    geo = sfa.SFVecEnv(4, obs_type="image", image_geometry=(.25, (130, 80, 450, 460), 3))
    assert not geo.default_geometry
    with pytest.raises(ValueError):
        sfa.FrameRollout(geo, 4, num_stack=4)
    img = sfa.SFVecEnv(4, obs_type="image")
    for bad in (dict(num_stack=0), dict(num_stack=17), dict(layout="rows")):
        with pytest.raises(ValueError):
            sfa.FrameRollout(img, 4, **bad)
    fro = sfa.FrameRollout(img, 4, num_stack=2)
    fro.reset()
    with pytest.raises(IndexError):
        fro.stack_at(5)
    for e in (sym, raw, geo, img):
        e.close()
