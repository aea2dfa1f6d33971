"""The numpy model of the time limit's bootstrap (tests/timelimit_np.py), on the CPU: hand-made cases whose answers can be
read off, and the properties sf_compute_returns_tl's definition promises -- a select on the mask, so nothing of a never-finished
env's final_value shows; a finished env with final_value 0 is the plain recursion; the numpy and the torch evaluation agree
bit for bit."""
import numpy as np
import pytest

import timelimit_np as TL
import trainerref as TR

f32 = np.float32


def _case(T, n, finish_at, seed=0):
    """engine-like rewards, masks all 1 but masks[t + 1][i] = 0 where finish_at[i] == t (None / -1: the env never finishes)"""
    rng = np.random.default_rng([seed, T, n])
    rewards = rng.integers(-1, 4, (T, n)).astype(f32)
    vp = rng.standard_normal((T + 1, n)).astype(f32)
    masks = np.ones((T + 1, n), f32)
    for i, t in enumerate(finish_at):
        if t is not None and t >= 0:
            masks[t + 1, i] = 0
    nv = rng.standard_normal(n).astype(f32)
    fv = rng.standard_normal(n).astype(f32)
    return rewards, vp, masks, nv, fv


def test_one_step_by_hand():
    """T = 1, plain returns: finished -> r + gamma * fv (next_value masked away); not finished -> r + gamma * next_value."""
    g = 0.5
    rewards = np.array([[1.0, 2.0]], f32)
    masks = np.array([[1, 1], [0, 1]], f32)
    nv, fv = np.array([10.0, 20.0], f32), np.array([4.0, 100.0], f32)
    vp = np.zeros((2, 2), f32)
    ret, _ = TL.compute_returns_tl(rewards, vp, masks, nv, fv, False, g, 0.95)
    assert ret[0].tolist() == [1.0 + 0.5 * 4.0, 2.0 + 0.5 * 20.0]
    assert ret[1].tolist() == [10.0, 20.0]
    # GAE, tau = 1, values 0: the same numbers
    ret, _ = TL.compute_returns_tl(rewards, vp, masks, nv, fv, True, g, 1.0)
    assert ret[0].tolist() == [3.0, 12.0]


def test_two_steps_by_hand():
    """T = 2, env 0 finishes at the first step, env 1 at the last, env 2 never (gamma 0.5: every product is exact)."""
    g = 0.5
    rewards = np.array([[1, 1, 1], [2, 2, 2]], f32)
    masks = np.array([[1, 1, 1], [0, 1, 1], [1, 0, 1]], f32)
    nv, fv = np.array([8, 8, 8], f32), np.array([4, 4, 4], f32)
    ret, _ = TL.compute_returns_tl(rewards, np.zeros((3, 3), f32), masks, nv, fv, False, g, 0.0)
    # env 0: ret[1] = 2 + .5 * 8 = 6 (a new game's step); ret[0] = 1 + .5 * 4 (the bootstrap; ret[1] masked) = 3
    # env 1: ret[1] = 2 + .5 * 4 = 4 (next_value masked); ret[0] = 1 + .5 * 4 = 3
    # env 2: ret[1] = 2 + .5 * 8 = 6; ret[0] = 1 + .5 * 6 = 4
    assert ret[1].tolist() == [6.0, 4.0, 6.0]
    assert ret[0].tolist() == [3.0, 3.0, 4.0]


@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("use_gae", [False, True])
def test_never_finished_lanes_ignore_final_value(T, use_gae):
    """A finish at the first step, at the last step, at none: NaN / inf in the final_value of the envs that never finish
    leaves their returns the plain recursion's, bit for bit; the finished envs' differ from it."""
    n = 6
    finish = [0, T - 1, None, None, 0, None]
    rewards, vp, masks, nv, fv = _case(T, n, finish)
    never = ~TL.finished(masks)
    assert never.tolist() == [False, False, True, True, False, True]
    fv[2], fv[3], fv[5] = np.nan, np.inf, -np.inf
    for g, tau in ((0.99, 0.95), (1 / 3, 2 / 3)):
        got, gvp = TL.compute_returns_tl(rewards, vp.copy(), masks, nv, fv, use_gae, g, tau)
        plain, pvp = TR.compute_returns(rewards, vp.copy(), masks, nv, use_gae, g, tau)
        rows = slice(0, T) if use_gae else slice(0, T + 1)
        TR.assert_bits_equal(got[rows][:, never], plain[rows][:, never], "never finished")
        TR.assert_bits_equal(gvp, pvp, "value_preds")
        assert np.isfinite(got[rows][:, ~never]).all()
        fin_t = [0, T - 1, 0]
        for i, t in zip(np.flatnonzero(~never), fin_t):
            assert got[t, i] != plain[t, i], (i, t)


@pytest.mark.parametrize("T", [1, 2, 5])
@pytest.mark.parametrize("use_gae", [False, True])
def test_final_value_zero_is_the_plain_recursion(T, use_gae):
    """r + gamma * 0 = r (engine rewards are never -0.0): every lane, finished or not, equals the plain recursion."""
    rewards, vp, masks, nv, fv = _case(T, 5, [0, T - 1, None, T // 2, None], seed=1)
    fv[:] = 0
    got, _ = TL.compute_returns_tl(rewards, vp.copy(), masks, nv, fv, use_gae, 0.99, 0.95)
    plain, _ = TR.compute_returns(rewards, vp.copy(), masks, nv, use_gae, 0.99, 0.95)
    rows = slice(0, T) if use_gae else slice(0, T + 1)
    TR.assert_bits_equal(got[rows], plain[rows])


def test_rewards2_is_a_select_and_reads_only():
    rewards, vp, masks, nv, fv = _case(5, 4, [0, 4, None, 2])
    fv[2] = np.nan
    keep = rewards.copy()
    r2 = TL.rewards2(rewards, masks, fv, 0.99)
    assert np.array_equal(rewards, keep)
    changed = r2 != rewards
    assert changed.sum() == 3 and changed[0, 0] and changed[4, 1] and changed[2, 3]
    assert r2[0, 0] == rewards[0, 0] + f32(0.99) * fv[0]
    assert not np.isnan(r2).any()


@pytest.mark.parametrize("kind", TR.KINDS)
@pytest.mark.parametrize("use_gae", [False, True])
def test_numpy_and_torch_agree(kind, use_gae):
    """The two evaluations, every kind of value and every (gamma, tau) pair of the table, T = 7, n = 65."""
    T, n = 7, 65
    rewards, vp, masks, nv = TR.gen_returns_case(kind, T, n, seed=5)
    fv = TL.gen_final_value(kind, n, seed=5)
    if kind not in ("masks-as-data", "masks-uniform"):
        assert TL.finished(masks).any() and not TL.finished(masks).all()
    for g, tau in TR.GAMMA_TAU:
        a, avp = TL.compute_returns_tl(rewards, vp.copy(), masks, nv, fv, use_gae, g, tau)
        b, bvp = TL.torch_compute_returns_tl(rewards, vp.copy(), masks, nv, fv, use_gae, g, tau)
        rows = slice(0, T) if use_gae else slice(0, T + 1)
        TR.assert_bits_equal(a[rows], b[rows], "%s %r" % (kind, (g, tau)))
        TR.assert_bits_equal(avp, bvp)
