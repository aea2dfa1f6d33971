"""The three frame-stack operations of the C API (include/sfmi.h: sf_frame_stack_clear, sf_render_stack,
sf_render_shift) as plain array statements.  Test-only.  The operations have no arithmetic: every result is a copy of
an input byte or zero, so comparisons against them are exact.

Written with indexing that numpy arrays and torch tensors share (boolean-row assignment, slices), so the same three
functions that tests/test_frame_stack_model.py holds to the trainer's own update (rl/train.py:51-56,92-97) on the host
also make the expected bytes of stacks of hundreds of megabytes where they lie, on the device.  A done flag is any
non-zero byte.  No input is modified."""

FRAME = 84 * 84  # bytes of one 84x84 frame


def _copy(a):
    return a.copy() if hasattr(a, "copy") else a.clone()


def clear(stack, done):
    """stack [n, B], done [n] -> rows with done != 0 zeroed, the other rows as they were."""
    out = _copy(stack)
    out[done != 0] = 0
    return out


def render_stack(stack, frame, slot, done=None):
    """stack [n, S, ...], frame [n, ...]: slot `slot` becomes the frame; an env with done != 0 has every other slot
    zeroed; everything else as it was."""
    out = _copy(stack)
    if done is not None:
        out[done != 0] = 0
    out[:, slot] = frame
    return out


def render_shift(prev, frame, done=None):
    """prev [n, S, ...], frame [n, ...] -> slots 0 .. S-2 = prev's slots 1 .. S-1 (zero where done != 0), slot S-1 = frame."""
    out = _copy(prev)
    out[:, :-1] = prev[:, 1:]
    if done is not None:
        out[done != 0] = 0
    out[:, -1] = frame
    return out

