"""sf_compute_returns, sf_record_step, sf_record_step_f32 and the step kernel's bookkeeping epilogue (sf_step_record)
through the raw C ABI, at every launch shape and on every kind of float the arrays can hold, against the reference of
tests/trainerref.py bit for bit (assert_bits_equal: NaN where the reference has NaN, the same 32 bits everywhere else).
Every buffer lies in a larger allocation with 64 sentinel elements in front and behind, outputs start out as sentinels:
a lane that writes past its row, or does not write, shows.  test_trainer_ref_model.py shows on the CPU that the reference
equals torch's own evaluation of the trainer's expressions and that these inputs catch a wrong rounding of gamma * tau, a
contracted multiply-add and a sign-extended uint8 action.

Launch shapes (both kernels: one lane per env, 256-thread blocks):

      n       blocks
      1       one lane
     63 / 64 / 65      one wave, ragged / full / one lane into the second
    255 / 256 / 257    one block ragged / full / one lane into the second
    511 / 513          two blocks ragged / three (returns only)
   4097       17 blocks, the last of one lane
  65537       257 blocks: row t + 1 starts 256 KiB behind row t, and a block index past 255
"""
import ctypes as C
import functools

import numpy as np
import pytest

import trainerref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

DEV = "cuda"
TDT = {np.uint8: torch.uint8, np.int32: torch.int32, np.int64: torch.int64, np.float32: torch.float32}


@pytest.fixture(scope="module")
def L():
    import spacefortress_amd  # noqa: F401  (the package loads and checks libsfmi.so)
    from spacefortress_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return _lib.lib()


def _p(t, byte_offset=0):
    return None if t is None else C.c_void_p(t.data_ptr() + byte_offset)


def _dev(x, dtype=None):
    """numpy -> a guarded device tensor holding it"""
    x = np.ascontiguousarray(x)
    return R.guarded(x.shape, dtype or TDT[x.dtype.type], DEV, x)


def _out(shape, dtype=torch.float32):
    return R.guarded(shape, dtype, DEV)


def _bytes(t):
    return t.cpu().numpy().tobytes()


# ---------------------------------------------------------------------------------------------------------------
# a. sf_compute_returns
@functools.lru_cache(maxsize=2)
def _returns_inputs(kind, T, n):
    return R.gen_returns_case(kind, T, n)


def _run_returns(L, kind, n, T, gae, gamma, tau):
    rewards, vp, masks, nv = _returns_inputs(kind, T, n)
    want, want_vp = R.compute_returns(rewards, vp, masks, nv, gae, gamma, tau)
    tag = "%s n=%d T=%d %s (%r, %r)" % (kind, n, T, "gae" if gae else "plain", gamma, tau)
    d_rew, d_vp, d_masks, d_nv, d_ret = _dev(rewards), _dev(vp), _dev(masks), _dev(nv), _out((T + 1, n))
    assert L.sf_compute_returns(T, n, _p(d_rew), _p(d_vp), _p(d_masks), _p(d_nv), _p(d_ret), int(gae), gamma, tau, None) == 0, tag
    torch.cuda.synchronize()
    if gae:
        R.assert_bits_equal(d_ret[:T], want[:T], tag + " returns")
        assert R.untouched(d_ret[T]), tag + ": returns[T] is not the GAE path's to write"
        R.assert_bits_equal(d_vp[T], nv, tag + " value_preds[T] = next_value")
        R.assert_bits_equal(d_vp, want_vp, tag + " value_preds")
    else:
        R.assert_bits_equal(d_ret, want, tag + " returns")
        R.assert_bits_equal(d_ret[T], nv, tag + " returns[T] = next_value")
    assert _bytes(d_vp[:T]) == vp[:T].tobytes() and (gae or _bytes(d_vp[T]) == vp[T].tobytes()), tag + ": value_preds changed"
    assert _bytes(d_rew) == rewards.tobytes() and _bytes(d_masks) == masks.tobytes() and _bytes(d_nv) == nv.tobytes(), tag + ": an input changed"
    R.margins_intact(d_rew, d_vp, d_masks, d_nv, d_ret)
    # the same inputs again: the same bytes (plain returns without value_preds at all: sfmi.h)
    d_ret2 = _out((T + 1, n))
    assert L.sf_compute_returns(T, n, _p(d_rew), _p(d_vp) if gae else None, _p(d_masks), _p(d_nv), _p(d_ret2), int(gae), gamma, tau, None) == 0, tag
    torch.cuda.synchronize()
    assert _bytes(d_ret2) == _bytes(d_ret), tag + ": a second run differs"
    R.margins_intact(d_rew, d_vp, d_masks, d_nv, d_ret2)


@pytest.mark.parametrize("T", R.RETURNS_TS)
@pytest.mark.parametrize("n", R.RETURNS_NS)
def test_returns_at_every_launch_shape(L, n, T):
    kind, (gamma, tau) = R.RETURNS_FULL
    for gae in (True, False):
        _run_returns(L, kind, n, T, gae, gamma, tau)


@pytest.mark.parametrize("pair", range(len(R.GAMMA_TAU)), ids=["%.4g-%.4g" % p for p in R.GAMMA_TAU])
@pytest.mark.parametrize("kind", R.KINDS)
def test_returns_of_every_kind_and_pair(L, kind, pair):
    gamma, tau = R.GAMMA_TAU[pair]
    if (kind, (gamma, tau)) == R.RETURNS_FULL:
        return  # test_returns_at_every_launch_shape has these shapes
    for n, T in R.RETURNS_OTHER_SHAPES:
        for gae in (True, False):
            _run_returns(L, kind, n, T, gae, gamma, tau)


def test_returns_refusals(L):
    n, T = 257, 3
    rewards, vp, masks, nv = R.gen_returns_case("normal", T, n)
    d_rew, d_vp, d_masks, d_nv, d_ret = _dev(rewards), _dev(vp), _dev(masks), _dev(nv), _out((T + 1, n))
    a = [T, n, _p(d_rew), _p(d_vp), _p(d_masks), _p(d_nv), _p(d_ret), 1, 0.99, 0.95, None]
    for i, v in ((0, 0), (0, -1), (1, 0), (1, -5), (2, None), (3, None), (4, None), (5, None), (6, None)):
        b = list(a)
        b[i] = v
        assert L.sf_compute_returns(*b) < 0, (i, v)
    torch.cuda.synchronize()
    assert R.untouched(d_ret) and _bytes(d_vp) == vp.tobytes()
    R.margins_intact(d_rew, d_vp, d_masks, d_nv, d_ret)


# ---------------------------------------------------------------------------------------------------------------
# b. sf_record_step / sf_record_step_f32
def _record_fn(L, rkind):
    return L.sf_record_step_f32 if rkind.startswith("f32-") else L.sf_record_step


@pytest.mark.parametrize("rkind", R.REWARD_KINDS)
@pytest.mark.parametrize("n", R.RECORD_NS)
def test_record_step_at_every_launch_shape(L, n, rkind):
    """12 chained steps from accumulators that are no integers; `done` bytes from {0, 1, 2, 255}; the action type changes
    with the step, the values are whatever the type holds."""
    fn = _record_fn(L, rkind)
    ep, fin = R.gen_accumulators(rkind, n)
    d_ep, d_fin = _dev(ep), _dev(fin)
    d_r, d_m, d_act = _out(n), _out(n), _out(n, torch.int64)
    for step in range(R.RECORD_STEPS):
        r, d, a = R.gen_step_rewards(rkind, n, step), R.gen_done(n, step), R.gen_actions(R.ACT_DTYPES[step % 3], n, step)
        w_r, w_m, ep, fin, w_a = R.record_step(r, d, ep, fin, a)
        d_rew, d_done, d_a = _dev(r), _dev(d), _dev(a)
        R.refill(d_r, d_m, d_act)
        tag = "%s n=%d step %d" % (rkind, n, step)
        assert fn(n, _p(d_rew), _p(d_done), _p(d_r), _p(d_m), _p(d_ep), _p(d_fin), _p(d_a), a.itemsize, _p(d_act), None) == 0, tag
        torch.cuda.synchronize()
        R.assert_bits_equal(d_r, w_r, tag + " reward_out")
        R.assert_bits_equal(d_m, w_m, tag + " mask_out")
        R.assert_bits_equal(d_ep, ep, tag + " episode_rewards")
        R.assert_bits_equal(d_fin, fin, tag + " final_rewards")
        got = d_act.cpu().numpy()
        assert np.array_equal(got, w_a), (tag, a.dtype, got[got != w_a][:4], w_a[got != w_a][:4])
        assert _bytes(d_rew) == r.tobytes() and _bytes(d_done) == d.tobytes() and _bytes(d_a) == a.tobytes(), tag + ": an input changed"
        R.margins_intact(d_rew, d_done, d_a, d_r, d_m, d_ep, d_fin, d_act)


@pytest.mark.parametrize("rkind", ["i32-full", "f32-normal"])
def test_record_step_with_every_set_of_outputs(L, rkind):
    """All 32 NULL / non-NULL combinations of reward_out, mask_out, episode_rewards, final_rewards, actions_out: what is
    passed equals the reference, and final_rewards without episode_rewards is left alone (sfmi.h)."""
    fn, n = _record_fn(L, rkind), R.NULL_N
    for combo in range(32):
        has_r, has_m, has_ep, has_fin, has_a = (bool(combo >> k & 1) for k in range(5))
        r, d, a = R.gen_step_rewards(rkind, n, combo), R.gen_done(n, combo), R.gen_actions(R.ACT_DTYPES[combo % 3], n, combo)
        ep0, fin0 = R.gen_accumulators(rkind, n, seed=combo)
        w_r, w_m, w_ep, w_fin, w_a = R.record_step_optional(r, d, ep0 if has_ep else None, fin0 if has_fin else None, a)
        d_rew, d_done, d_a = _dev(r), _dev(d), _dev(a)
        d_r, d_m, d_act = (_out(n) if has_r else None), (_out(n) if has_m else None), (_out(n, torch.int64) if has_a else None)
        d_ep, d_fin = (_dev(ep0) if has_ep else None), (_dev(fin0) if has_fin else None)
        tag = "%s combo %d" % (rkind, combo)
        # (without actions_out the actions are not read: NULL on the odd combinations)
        acts = _p(d_a) if has_a or combo % 2 == 0 else None
        assert fn(n, _p(d_rew), _p(d_done), _p(d_r), _p(d_m), _p(d_ep), _p(d_fin), acts, a.itemsize, _p(d_act), None) == 0, tag
        torch.cuda.synchronize()
        for got, want, what in ((d_r, w_r, "reward_out"), (d_m, w_m, "mask_out"), (d_ep, w_ep, "episode_rewards"), (d_fin, w_fin, "final_rewards")):
            if got is not None:
                R.assert_bits_equal(got, want, tag + " " + what)
        if has_fin and not has_ep:
            assert _bytes(d_fin) == fin0.tobytes(), tag + ": final_rewards without episode_rewards must stay as it is"
        if has_a:
            assert np.array_equal(d_act.cpu().numpy(), w_a), tag
        R.margins_intact(*[t for t in (d_rew, d_done, d_a, d_r, d_m, d_ep, d_fin, d_act) if t is not None])


@pytest.mark.parametrize("rkind", ["i32-engine", "f32-normal"])
def test_record_step_refusals(L, rkind):
    fn, n = _record_fn(L, rkind), R.NULL_N
    d_rew, d_done, d_a = _dev(R.gen_step_rewards(rkind, n, 0)), _dev(R.gen_done(n, 0)), _dev(R.gen_actions(np.int32, n, 0))
    outs = [_out(n), _out(n), _out(n), _out(n), _out(n, torch.int64)]  # reward_out, mask_out, episode_rewards, final_rewards, actions_out
    a = [n, _p(d_rew), _p(d_done), _p(outs[0]), _p(outs[1]), _p(outs[2]), _p(outs[3]), _p(d_a), 4, _p(outs[4]), None]
    for change in ({0: 0}, {0: -1}, {1: None}, {2: None}, {7: None}, {8: 2}, {8: 0}):
        b = list(a)
        for i, v in change.items():
            b[i] = v
        assert fn(*b) < 0, change
    torch.cuda.synchronize()
    assert R.untouched(*outs), "a refused call wrote something"
    R.margins_intact(d_rew, d_done, d_a, *outs)


# ---------------------------------------------------------------------------------------------------------------
# c. sf_step_record: the step kernel's epilogue
def _env_pair(n, gametype, obs_type, f64, first_done=3, spread=17):
    """Two equal batches whose env e ends its game `first_done + e % spread` steps from here."""
    import spacefortress_amd as sfa
    mk = lambda: sfa.SFVecEnv(n, gametype=gametype, obs_type=obs_type, spawn_stride=1, obs_dtype=torch.float64 if f64 else torch.float32)
    env, twin = mk(), mk()
    d = first_done + np.arange(n) % spread
    for e in (env, twin):
        e.set_field("time", (34 * (5295 - d)).astype(np.int32))
    return env, twin


def _engine_outputs(env):
    n = env.num_envs
    return (_out((n,) + tuple(env.obs_shape), env.obs_dtype), _out(n, torch.int32), _out(n, torch.uint8), _out(n, torch.uint8))


@pytest.mark.parametrize("n,gametype,obs_type,f64,adt", R.epilogue_cases(),
                         ids=["%d-%s-%s-%s-%s" % (c[0], c[1], c[2], "f64" if c[3] else "f32", np.dtype(c[4]).name) for c in R.epilogue_cases()])
def test_epilogue_against_the_reference(L, n, gametype, obs_type, f64, adt):
    """40 steps of sf_step_record.  The bookkeeping equals the reference applied to what the SAME launch wrote to reward_dev
    and done_dev; the game (obs, reward, done, info) equals a twin batch stepped with sf_step.  Everything is kept on the
    device and compared after the last step."""
    steps = R.EPILOGUE_STEPS
    env, twin = _env_pair(n, gametype, obs_type, f64)
    rng = np.random.default_rng([n, len(gametype), len(obs_type), int(f64)])
    acts = torch.from_numpy(rng.integers(0, env.n_actions, (steps, n)).astype(adt)).cuda()
    ep, fin = R.gen_accumulators("f32-normal", n)
    d_ep, d_fin = _dev(ep), _dev(fin)
    obs, rew, done, info = _engine_outputs(env)
    o2, r2, dn2, i2 = twin._alloc()
    d_r, d_m, d_act = _out(n), _out(n), _out(n, torch.int64)
    kept, game_differs = [], torch.zeros((), dtype=torch.bool, device=DEV)
    for t in range(steps):
        R.refill(obs, rew, done, info, d_r, d_m, d_act)
        assert L.sf_step_record(env._h, _p(acts[t]), acts.element_size(), _p(obs), _p(rew), _p(done), _p(info), _p(d_r), _p(d_m), _p(d_ep),
                                _p(d_fin), _p(d_act), None) == 0, t
        assert L.sf_step(twin._h, _p(acts[t]), acts.element_size(), _p(o2), _p(r2), _p(dn2), _p(i2), None) == 0, t
        game_differs |= (obs != o2).any() | (rew != r2).any() | (done != dn2).any() | (info != i2).any()
        kept.append(tuple(x.clone() for x in (rew, done, d_r, d_m, d_ep, d_fin, d_act)))
    torch.cuda.synchronize()
    assert not bool(game_differs), "the epilogue changed the game"
    R.margins_intact(obs, rew, done, info, d_r, d_m, d_ep, d_fin, d_act)
    saw_done = False
    for t, (k_rew, k_done, k_r, k_m, k_ep, k_fin, k_act) in enumerate(kept):
        r_np, d_np = k_rew.cpu().numpy(), k_done.cpu().numpy()
        assert set(np.unique(d_np).tolist()) <= {0, 1}
        saw_done = saw_done or bool(d_np.any())
        w_r, w_m, ep, fin, w_a = R.record_step(r_np, d_np, ep, fin, acts[t].cpu().numpy())
        tag = "step %d" % t
        R.assert_bits_equal(k_r, w_r, tag + " reward_f32")
        R.assert_bits_equal(k_m, w_m, tag + " mask_f32")
        R.assert_bits_equal(k_ep, ep, tag + " episode_rewards")
        R.assert_bits_equal(k_fin, fin, tag + " final_rewards")
        assert np.array_equal(k_act.cpu().numpy(), w_a), tag
    assert saw_done, "no game ended inside the run"
    assert L.sf_check_actions(env._h, None) == 0
    env.close()
    twin.close()


def test_epilogue_with_every_set_of_outputs(L):
    """All 16 NULL / non-NULL combinations of mask_f32, episode_rewards, final_rewards, actions_out (reward_f32 is
    required), three steps each on one pair of batches in which some game ends at every step."""
    n = R.NULL_N
    env, twin = _env_pair(n, "youturn", "features", False, first_done=1, spread=48)
    rng = np.random.default_rng(16)
    obs, rew, done, info = _engine_outputs(env)
    o2, r2, dn2, i2 = twin._alloc()
    ends = 0
    for combo in range(16):
        has_m, has_ep, has_fin, has_a = (bool(combo >> k & 1) for k in range(4))
        ep, fin = R.gen_accumulators("f32-normal", n, seed=combo)
        fin0 = fin
        d_r, d_m, d_act = _out(n), (_out(n) if has_m else None), (_out(n, torch.int64) if has_a else None)
        d_ep, d_fin = (_dev(ep) if has_ep else None), (_dev(fin) if has_fin else None)
        for t in range(3):
            a_np = rng.integers(0, env.n_actions, n).astype(R.ACT_DTYPES[(combo + t) % 3])
            a = torch.from_numpy(a_np).cuda()
            R.refill(*[x for x in (obs, rew, done, info, d_r, d_m, d_act) if x is not None])
            tag = "combo %d step %d" % (combo, t)
            assert L.sf_step_record(env._h, _p(a), a.element_size(), _p(obs), _p(rew), _p(done), _p(info), _p(d_r), _p(d_m), _p(d_ep),
                                    _p(d_fin), _p(d_act), None) == 0, tag
            assert L.sf_step(twin._h, _p(a), a.element_size(), _p(o2), _p(r2), _p(dn2), _p(i2), None) == 0, tag
            torch.cuda.synchronize()
            assert torch.equal(obs, o2) and torch.equal(rew, r2) and torch.equal(done, dn2) and torch.equal(info, i2), tag
            d_np = done.cpu().numpy()
            ends += int(d_np.any())
            w_r, w_m, ep, fin, w_a = R.record_step_optional(rew.cpu().numpy(), d_np, ep if has_ep else None, fin if has_fin else None, a_np)
            R.assert_bits_equal(d_r, w_r, tag + " reward_f32")
            for got, want, what in ((d_m, w_m, "mask_f32"), (d_ep, ep, "episode_rewards"), (d_fin, fin, "final_rewards")):
                if got is not None:
                    R.assert_bits_equal(got, want, tag + " " + what)
            if has_a:
                assert np.array_equal(d_act.cpu().numpy(), w_a), tag
        if has_fin and not has_ep:
            assert _bytes(d_fin) == fin0.tobytes(), "combo %d: final_rewards without episode_rewards must stay as it is" % combo
        R.margins_intact(*[x for x in (obs, rew, done, info, d_r, d_m, d_ep, d_fin, d_act) if x is not None])
    assert ends >= 40, "games must end all through the run (%d of 48 steps)" % ends
    env.close()
    twin.close()


def test_epilogue_refuses_misaligned_outputs(L):
    """reward_f32 (and the other float outputs) off a 4-byte boundary, actions_out off an 8-byte one: SF_ERR_ARG, nothing is
    launched -- every output keeps its sentinel and the batch has not moved (its next step is the twin's first)."""
    from spacefortress_amd import _lib
    n = R.NULL_N
    env, twin = _env_pair(n, "autoturn", "features", False)
    a = torch.from_numpy(np.random.default_rng(5).integers(0, env.n_actions, n).astype(np.uint8)).cuda()
    obs, rew, done, info = _engine_outputs(env)
    d_r, d_m, d_ep, d_fin, d_act = _out(n), _out(n), _out(n), _out(n), _out(n, torch.int64)
    good = [env._h, _p(a), 1, _p(obs), _p(rew), _p(done), _p(info), _p(d_r), _p(d_m), _p(d_ep), _p(d_fin), _p(d_act), None]
    for i, t, off in ((7, d_r, 2), (7, d_r, 1), (8, d_m, 2), (9, d_ep, 3), (10, d_fin, 2), (11, d_act, 4), (11, d_act, 2)):
        b = list(good)
        b[i] = _p(t, off)
        assert L.sf_step_record(*b) == _lib.SF_ERR_ARG, (i, off)
    for change in ({7: None}, {1: None}, {2: 2}, {0: None}):  # reward_f32 is required; actions; act_type; the batch
        b = list(good)
        for i, v in change.items():
            b[i] = v
        assert L.sf_step_record(*b) < 0, change
    torch.cuda.synchronize()
    assert R.untouched(obs, rew, done, info, d_r, d_m, d_ep, d_fin, d_act), "a refused call wrote something"
    R.margins_intact(obs, rew, done, info, d_r, d_m, d_ep, d_fin, d_act)
    ep, fin = R.gen_accumulators("f32-normal", n)
    d_ep.copy_(torch.from_numpy(ep))
    d_fin.copy_(torch.from_numpy(fin))
    assert L.sf_step_record(*good) == 0
    o2, r2, dn2, i2 = twin.step_tensors(a)
    torch.cuda.synchronize()
    assert torch.equal(obs, o2) and torch.equal(rew, r2) and torch.equal(done, dn2) and torch.equal(info, i2)
    w_r, w_m, ep, fin, w_a = R.record_step(rew.cpu().numpy(), done.cpu().numpy(), ep, fin, a.cpu().numpy())
    R.assert_bits_equal(d_r, w_r)
    R.assert_bits_equal(d_m, w_m)
    R.assert_bits_equal(d_ep, ep)
    R.assert_bits_equal(d_fin, fin)
    assert np.array_equal(d_act.cpu().numpy(), w_a)
    env.close()
    twin.close()


# ---------------------------------------------------------------------------------------------------------------
# d. the `stream` argument, in a captured graph
def test_rollout_bookkeeping_and_returns_replay_from_a_graph(L):
    """Four sf_record_step_f32, each on its own rows of one reward / done buffer, then sf_compute_returns, captured on a side
    stream into one linear graph; replayed twice on different contents."""
    n, T = 1000, 4
    gamma, tau = R.RETURNS_FULL[1]
    d_src, d_done, d_a = _out((T, n)), _out((T, n), torch.uint8), _out((T, n), torch.int32)
    d_rew, d_masks, d_vp, d_ret, d_nv = _out((T, n)), _out((T + 1, n)), _out((T + 1, n)), _out((T + 1, n)), _out(n)
    d_ep, d_fin, d_act = _out(n), _out(n), _out((T, n), torch.int64)
    side = torch.cuda.Stream()
    sp = C.c_void_p(side.cuda_stream)

    def launch():
        for t in range(T):
            assert L.sf_record_step_f32(n, _p(d_src[t]), _p(d_done[t]), _p(d_rew[t]), _p(d_masks[t + 1]), _p(d_ep), _p(d_fin), _p(d_a[t]), 4,
                                        _p(d_act[t]), sp) == 0
        assert L.sf_compute_returns(T, n, _p(d_rew), _p(d_vp), _p(d_masks), _p(d_nv), _p(d_ret), 1, gamma, tau, sp) == 0

    def load(kind, seed):
        rewards, vp, masks, nv = R.gen_returns_case(kind, T, n, seed)
        done = np.stack([R.gen_done(n, t, seed) for t in range(T)])
        acts = np.stack([R.gen_actions(np.int32, n, t, seed) for t in range(T)])
        ep, fin = R.gen_accumulators("f32-" + kind, n, seed)
        for dst, x in ((d_src, rewards), (d_done, done), (d_a, acts), (d_vp, vp), (d_nv, nv), (d_ep, ep), (d_fin, fin)):
            dst.copy_(torch.from_numpy(x))
        R.refill(d_rew, d_masks, d_ret, d_act)
        d_masks[0].copy_(torch.from_numpy(masks[0]))
        torch.cuda.synchronize()
        return rewards, vp, masks[0], nv, done, acts, ep, fin

    load("normal", 0)
    with torch.cuda.stream(side):  # (the kernels' code objects are loaded before the capture)
        launch()
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        launch()
    torch.cuda.synchronize()
    for kind, seed in (("special", 1), ("normal", 2)):
        rewards, vp, m0, nv, done, acts, ep, fin = load(kind, seed)
        g.replay()
        torch.cuda.synchronize()
        masks = [m0]
        for t in range(T):
            w_r, w_m, ep, fin, w_a = R.record_step(rewards[t], done[t], ep, fin, acts[t])
            masks.append(w_m)
            R.assert_bits_equal(d_rew[t], w_r, "%s rewards[%d]" % (kind, t))
            R.assert_bits_equal(d_masks[t + 1], w_m, "%s masks[%d]" % (kind, t + 1))
            assert np.array_equal(d_act[t].cpu().numpy(), w_a)
        R.assert_bits_equal(d_ep, ep, kind + " episode_rewards")
        R.assert_bits_equal(d_fin, fin, kind + " final_rewards")
        want, want_vp = R.compute_returns(rewards, vp, np.stack(masks), nv, True, gamma, tau)
        R.assert_bits_equal(d_ret[:T], want[:T], kind + " returns")
        R.assert_bits_equal(d_vp, want_vp, kind + " value_preds")
        assert R.untouched(d_ret[T])
        R.margins_intact(d_src, d_done, d_a, d_rew, d_masks, d_vp, d_ret, d_nv, d_ep, d_fin, d_act)
    del g
