"""The frame-stack model (tests/framestack_np.py: clear, render_stack, render_shift -- what tests/test_gpu_frame_stack.py
holds the kernels to) without a GPU, against a literal transcription of the trainer's update of its current observation
(rl/train.py:51-56,92-97), on float tensors as the trainer keeps them:

    current_obs *= masks
    current_obs[:, :-1] = current_obs[:, 1:]
    current_obs[:, -1:] = obs

The ring form (one slot written per step, the slot rotating, read back with roll: FrameStack) and the shift form (a new
stack from the previous one: DeviceRollout) both reproduce current_obs at every one of 30 steps, at every depth, with
done bytes other than 1, from numpy arrays and from torch tensors alike."""
import numpy as np
import pytest

import framestack_np as M

torch = pytest.importorskip("torch")

DEPTHS = [1, 2, 3, 4, 5, 16]
SHAPE = (3, 5)  # (the model never looks inside a frame)


def _trainer_step(current_obs, masks, obs):
    """rl/train.py:92-97 + 51-56 for one image channel (shape_dim0 = 1); num_stack > 1 guards the shift there."""
    current_obs *= masks.unsqueeze(2).unsqueeze(2)
    if current_obs.shape[1] > 1:
        current_obs[:, :-1] = current_obs[:, 1:]
    current_obs[:, -1:] = obs
    return current_obs


def _done_bytes(rng, n, rate, values):
    return np.where(rng.random(n) < rate, rng.choice(np.asarray(values, np.uint8), n), 0).astype(np.uint8)


@pytest.mark.parametrize("as_torch", [False, True], ids=["numpy", "torch"])
@pytest.mark.parametrize("values", [(1,), (2, 255), (1, 2, 128, 255)], ids=["ones", "2-255", "mixed"])
@pytest.mark.parametrize("S", DEPTHS)
def test_ring_and_shift_reproduce_the_trainers_current_obs(S, values, as_torch):
    n, T = 37, 30
    rng = np.random.default_rng(100 * S + len(values))
    conv = (lambda a: torch.from_numpy(np.ascontiguousarray(a))) if as_torch else (lambda a: a)
    back = (lambda a: a.numpy()) if as_torch else (lambda a: a)
    first = rng.integers(1, 256, (n,) + SHAPE).astype(np.uint8)  # (no zero pixels: a zeroed slot cannot pass for a frame)
    current_obs = torch.zeros(n, S, *SHAPE)
    _trainer_step(current_obs, torch.ones(n, 1), torch.from_numpy(first).float().unsqueeze(1))
    ring = np.zeros((n, S) + SHAPE, np.uint8)
    head = S - 1
    ring[:, head] = first
    ring = conv(ring)
    shifted = conv(back(ring).copy())
    seen = set()
    for t in range(T):
        obs = rng.integers(1, 256, (n,) + SHAPE).astype(np.uint8)
        done = _done_bytes(rng, n, 0.3 if t % 7 else (0.0, 1.0)[(t // 7) % 2], values)  # random, and none / all now and then
        seen.update(int(v) for v in done)
        masks = torch.FloatTensor([[0.0] if i else [1.0] for i in done])  # rl/train.py:87
        _trainer_step(current_obs, masks, torch.from_numpy(obs).float().unsqueeze(1))
        want = current_obs.numpy()
        # the ring: FrameStack.step
        head = (head + 1) % S
        before = back(ring).copy()
        ring = M.render_stack(ring, conv(obs), head, conv(done))
        assert np.array_equal(np.roll(back(ring), -(head + 1), axis=1).astype(np.float32), want), t
        # ... which touches nothing but slot `head` and the finished envs
        live = done == 0
        others = [s for s in range(S) if s != head]
        assert np.array_equal(back(ring)[live][:, others], before[live][:, others])
        # the shift: DeviceRollout.step
        prev, keep = shifted, back(shifted).copy()
        shifted = M.render_shift(prev, conv(obs), conv(done))
        assert np.array_equal(back(prev), keep)  # (prev is only read)
        assert np.array_equal(back(shifted).astype(np.float32), want), t
    assert seen == set(values) | {0}


@pytest.mark.parametrize("S", DEPTHS)
def test_without_done_flags_nothing_is_zeroed(S):
    rng = np.random.default_rng(S)
    n = 9
    stack = rng.integers(1, 256, (n, S) + SHAPE).astype(np.uint8)
    frame = rng.integers(1, 256, (n,) + SHAPE).astype(np.uint8)
    zeros = np.zeros(n, np.uint8)
    for slot in range(S):
        got = M.render_stack(stack, frame, slot, None)
        assert np.array_equal(got, M.render_stack(stack, frame, slot, zeros))
        assert np.array_equal(got[:, slot], frame) and np.array_equal(np.delete(got, slot, 1), np.delete(stack, slot, 1))
    got = M.render_shift(stack, frame, None)
    assert np.array_equal(got, M.render_shift(stack, frame, zeros))
    assert np.array_equal(got[:, :-1], stack[:, 1:]) and np.array_equal(got[:, -1], frame) and (got != 0).all()


def test_clear_zeroes_rows_with_any_non_zero_byte_and_only_those():
    rng = np.random.default_rng(5)
    stack = rng.integers(1, 256, (11, 48)).astype(np.uint8)
    done = np.array([0, 1, 0, 2, 0, 128, 0, 255, 0, 0, 7], np.uint8)
    keep = stack.copy()
    for conv, back in ((lambda a: a, lambda a: a), (torch.from_numpy, lambda a: a.numpy())):
        got = back(M.clear(conv(stack), conv(done)))
        assert np.array_equal(stack, keep)  # (the input is not modified)
        assert np.array_equal(got[done == 0], keep[done == 0]) and not got[done != 0].any()
    # the same statement as the trainer's: a product with the 0 / 1 mask
    masks = torch.FloatTensor([[0.0] if i else [1.0] for i in done])
    assert np.array_equal(M.clear(stack, done).astype(np.float32), (torch.from_numpy(stack).float() * masks).numpy())
