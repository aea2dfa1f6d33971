"""The frame-stack kernels -- sf_frame_stack_clear, sf_render_stack, sf_render_shift (include/sfmi.h; sf_render.hip:
sf_stack_clear_kernel and the stack parts of sf_render_kernel) -- and their wrappers, FrameStack and
DeviceRollout(num_stack > 1), against tests/framestack_np.py, which tests/test_frame_stack_model.py holds to the trainer's
own update (rl/train.py:51-56,92-97).

The operation has no arithmetic: every comparison is torch.equal.  Every output buffer starts out filled with non-zero
bytes that differ per env and per slot, so "zeroed", "left alone" and "written" are three outcomes that cannot pass for
one another, and it is a view at a 16-byte (and no better) aligned offset into a larger allocation whose 4 KiB in front
and behind hold a fixed pattern that is checked after every launch.  The new frame a launch must write comes from a twin
batch that plays the same game and has only ever been rendered plainly."""
import ctypes as C

import numpy as np
import pytest

import framestack_np as M
from lockstep import sfa

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FRAME = M.FRAME
GUARD = 4096
DONE_BYTES = (1, 2, 128, 255)  # a done flag is any non-zero byte
GEOM = (.25, (130, 80, 450, 460), 3)  # another geometry than the default: the general renderer
BATCHES = [1, 63, 64, 65, 1000, 4097, 6209]  # a ragged last tile; more than 64 hint words; above SF_PREPASS_MAX_ENVS
DEPTHS = [1, 2, 3, 4, 5, 16]
CASES = [(n, s) for n in BATCHES for s in DEPTHS if s < 16 or n <= 1000]


@pytest.fixture(scope="module")
def L():
    from spacefortress_amd import _lib
    return _lib.lib()


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _dev():
    return torch.device("cuda", torch.cuda.current_device())


class Guarded:
    """`nbytes` of device memory between two guard bands; `shift` moves the view off its 16-byte alignment."""

    def __init__(self, nbytes, shift=0):
        dev = _dev()
        self.front, self.n = GUARD + 16 + shift, int(nbytes)
        self.base = torch.empty(self.front + self.n + GUARD, dtype=torch.uint8, device=dev)
        assert self.base.data_ptr() % 256 == 0
        pat = lambda k: ((torch.arange(k, device=dev) * 37 + 11) % 251 + 1).to(torch.uint8)
        self.pat = (pat(self.front), pat(GUARD).flip(0))
        self.base[:self.front] = self.pat[0]
        self.base[self.front + self.n:] = self.pat[1]
        self.view = self.base[self.front:self.front + self.n]
        assert self.view.data_ptr() % 16 == shift % 16 and (shift or self.view.data_ptr() % 32 != 0)

    def intact(self):
        return torch.equal(self.base[:self.front], self.pat[0]) and torch.equal(self.base[self.front + self.n:], self.pat[1])


def sentinel(n, s):
    """[n, s, FRAME] of 1 + (env * 31 + slot * 7) % 255: never zero, different in neighbouring envs and in every slot."""
    e = torch.arange(n, device=_dev())[:, None] * 31 + torch.arange(s, device=_dev())[None, :] * 7
    return (1 + e % 255).to(torch.uint8)[:, :, None].expand(n, s, FRAME).contiguous()


def random_bytes(shape, seed):
    g = torch.Generator(device=_dev()).manual_seed(seed)
    return torch.randint(1, 256, shape, dtype=torch.uint8, device=_dev(), generator=g)


def done_patterns(n, rng, with_null=False):
    z = np.zeros(n, np.uint8)
    first, last = z.copy(), z.copy()
    first[0], last[-1] = 1, 1
    rnd = np.where(rng.random(n) < 0.3, rng.choice(np.asarray(DONE_BYTES, np.uint8), n), 0).astype(np.uint8)
    pats = [("none", z), ("all", np.ones(n, np.uint8)), ("first", first), ("last", last),
            ("alternating", (np.arange(n) % 2).astype(np.uint8)), ("random", rnd)]
    return ([("null", None)] if with_null else []) + [(k, torch.from_numpy(v).to(_dev())) for k, v in pats]


# ---------------------------------------------------------------------------------------------- (a) sf_frame_stack_clear
CLEAR_N = [1, 63, 64, 65, 257, 4097]
# 48 and 4080 leave some of the 256 threads idle; 4096 is exactly one trip of the loop, 4112 one trip and one piece
CLEAR_B = [16, 48, 4080, 4096, 4112, FRAME, 4 * FRAME, 16 * FRAME]
CLEAR_CASES = [(n, b) for n in CLEAR_N for b in CLEAR_B if n * b <= 256 << 20]  # (leaves out 4097 x 16 frames only)


@pytest.mark.parametrize("n,B", CLEAR_CASES)
def test_frame_stack_clear(L, n, B):
    rng = np.random.default_rng(n * 131 + B)
    fill = random_bytes((n, B), n + B)
    buf = Guarded(n * B)
    for name, done in done_patterns(n, rng):
        buf.view.copy_(fill.view(-1))
        assert L.sf_frame_stack_clear(_p(buf.view), B, _p(done), n, None) == 0
        assert torch.equal(buf.view.view(n, B), M.clear(fill, done)), name
        assert buf.intact(), name
        assert done.any() or torch.equal(buf.view.view(n, B), fill)


def test_frame_stack_clear_refusals(L):
    from spacefortress_amd import _lib
    n, B = 65, 4112
    fill = random_bytes((n * B,), 3)
    done = torch.ones(n, dtype=torch.uint8, device=_dev())
    buf, off = Guarded(n * B), Guarded(n * B, shift=8)
    for b in (buf, off):
        b.view.copy_(fill)
    for args in ((_p(off.view), B, _p(done), n),      # an unaligned stack
                 (_p(buf.view), B - 8, _p(done), n),  # bytes_per_env not a multiple of 16
                 (_p(buf.view), B, _p(done), 0), (_p(buf.view), B, _p(done), -3),
                 (None, B, _p(done), n), (_p(buf.view), B, None, n)):
        assert L.sf_frame_stack_clear(*args, None) == _lib.SF_ERR_ARG
        torch.cuda.synchronize()
        for b in (buf, off):
            assert torch.equal(b.view, fill) and b.intact()


# ------------------------------------------------------------------------------------ batches that have played a while
class Played:
    """A batch and its twin after T steps of the same random actions.  The twin is only ever rendered plainly."""

    def __init__(self, sfa, n, geometry=None, T=140):
        kw = dict(gametype="youturn", obs_type="image", spawn_stride=5, image_geometry=geometry)
        self.n = n
        self.env, self.twin = sfa.SFVecEnv(n, **kw), sfa.SFVecEnv(n, **kw)
        self.rng = np.random.default_rng(1000 + n)
        self.deaths = 0
        for t in range(T):
            o1, o2 = self._step()
            self.deaths += int((torch.from_numpy(self.twin.get_field("flags")) & 1 == 0).sum())
        assert torch.equal(o1, o2)

    def _step(self):
        a = torch.from_numpy(self.rng.integers(0, 5, self.n).astype(np.uint8)).to(self.env.device)
        return self.env.step_tensors(a)[0], self.twin.step_tensors(a)[0]

    def want(self):
        return self.twin.render("image").view(self.n, FRAME)

    def after_step(self):
        """the draw records and the hint words are those the step kernel left"""
        self._step()
        return self.want()

    def from_state(self):
        """the state was written from outside: the next frame launch rebuilds the records from it"""
        for e in (self.env, self.twin):
            e.set_field("time", e.get_field("time"))
        return self.want()

    def record_states(self):
        yield "step", self.after_step()
        yield "state", self.from_state()

    def close(self):
        self.env.close()
        self.twin.close()


_PLAYED = {}


@pytest.fixture(scope="module")
def played(sfa):
    def get(n, geometry=None):
        key = (n, geometry is not None)
        if key not in _PLAYED:
            _PLAYED[key] = Played(sfa, n, geometry, T=140 if geometry is None else 40)
            if geometry is None and n >= 1000:
                assert _PLAYED[key].deaths > 0  # ships have died: explosions, respawns, hint words
        return _PLAYED[key]
    yield get
    for p in _PLAYED.values():
        p.close()
    _PLAYED.clear()


def _slots(S):
    return range(S) if S <= 5 else (0, 7, 15)


# ---------------------------------------------------------------------------- (b) sf_render_stack, the default geometry
@pytest.mark.parametrize("N,S", CASES)
def test_render_stack(L, played, N, S):
    P = played(N)
    env = P.env
    fill = sentinel(N, S)
    buf = Guarded(N * S * FRAME)
    stack = buf.view.view(N, S, FRAME)
    for state, want in P.record_states():
        for slot in _slots(S):
            for name, done in done_patterns(N, P.rng, with_null=True):
                stack.copy_(fill)
                assert L.sf_render_stack(env._h, _p(stack), S, slot, _p(done), env._stream()) == 0
                assert torch.equal(stack, M.render_stack(fill, want, slot, done)), (state, slot, name)
                assert buf.intact(), (state, slot, name)


# ------------------------------------------------------------------------------------------------- (c) sf_render_shift
@pytest.mark.parametrize("N,S", CASES)
def test_render_shift(L, played, N, S):
    P = played(N)
    env = P.env
    fill, prev_fill = sentinel(N, S), random_bytes((N, S, FRAME), N + S)
    buf, pbuf = Guarded(N * S * FRAME), Guarded(N * S * FRAME)
    stack, prev = buf.view.view(N, S, FRAME), pbuf.view.view(N, S, FRAME)
    prev.copy_(prev_fill)
    for state, want in P.record_states():
        for name, done in done_patterns(N, P.rng, with_null=True):
            stack.copy_(fill)
            assert L.sf_render_shift(env._h, _p(prev), _p(stack), S, _p(done), env._stream()) == 0
            assert torch.equal(stack, M.render_shift(prev_fill, want, done)), (state, name)
            assert torch.equal(prev, prev_fill), (state, name)  # the previous stack is only read
            assert buf.intact() and pbuf.intact(), (state, name)
            if S == 1:
                assert torch.equal(stack[:, 0], want)


# ------------------------------------------------------------------------------------------- (d) launch order x stack
def _hint_words(bits):
    words = len(bits) // 64
    return np.packbits(bits.reshape(words, 64), axis=1, bitorder="little").view(np.uint64).reshape(words)


@pytest.mark.parametrize("S", [2, 4])
@pytest.mark.parametrize("N", [65, 1000, 4097])
def test_launch_order_hint_with_a_stack(L, played, N, S):
    """A hinted env's own workgroup leaves after it has loaded the done byte and a workgroup in front of the grid does
    its slots (sf_render.hip: pick_env): whatever the words say, every env's frame AND older slots are handled exactly
    once -- an env that nobody handled keeps its sentinel bytes."""
    from spacefortress_amd import _lib
    P = played(N)
    env, rng = P.env, P.rng
    want = P.after_step()
    words = (N + 63) // 64
    valid = np.zeros(words * 64, bool)
    valid[:N] = True  # (the step kernel never marks a lane behind the batch)
    only_last = np.zeros(words * 64, bool)
    only_last[N - 1] = True  # in the ragged last tile
    fill, prev_fill = sentinel(N, S), random_bytes((N, S, FRAME), 7 * N + S)
    buf, pbuf = Guarded(N * S * FRAME), Guarded(N * S * FRAME)
    stack, prev = buf.view.view(N, S, FRAME), pbuf.view.view(N, S, FRAME)
    prev.copy_(prev_fill)
    all_four = False
    for name, bits in (("none", ~valid & valid), ("all", valid), ("5 %", (rng.random(words * 64) < 0.05) & valid),
                       ("30 %", (rng.random(words * 64) < 0.3) & valid),  # more than the front of the grid holds
                       ("last", only_last)):
        w = _hint_words(bits)
        assert int(bits.sum()) == sum(bin(int(x)).count("1") for x in w)
        _lib.check(L.sf_set_render_order_hint(env._h, w.ctypes.data_as(C.c_void_p), words))
        for call in ("stack", "shift"):
            d = np.where(rng.random(N) < 0.3, rng.choice(np.asarray(DONE_BYTES, np.uint8), N), 0).astype(np.uint8)
            all_four = all_four or len({(bool(h), bool(f)) for h, f in zip(bits[:N], d)}) == 4
            done = torch.from_numpy(d).to(env.device)
            stack.copy_(fill)
            if call == "stack":
                assert L.sf_render_stack(env._h, _p(stack), S, 1, _p(done), env._stream()) == 0
                assert torch.equal(stack, M.render_stack(fill, want, 1, done)), (name, call)
            else:
                assert L.sf_render_shift(env._h, _p(prev), _p(stack), S, _p(done), env._stream()) == 0
                assert torch.equal(stack, M.render_shift(prev_fill, want, done)), (name, call)
                assert torch.equal(prev, prev_fill)
            assert buf.intact() and pbuf.intact(), (name, call)
    assert all_four  # hinted and finished, hinted only, finished only, neither: all among the envs of one launch


# ------------------------------------------------------------------------------ (e) sf_render_stack, another geometry
@pytest.mark.parametrize("S", [1, 3, 4])
@pytest.mark.parametrize("N", [1, 65, 1000])
def test_render_stack_in_another_geometry(L, played, N, S):
    """The general renderer draws into one slot; the finished envs' stacks are zeroed by sf_stack_clear_kernel in a launch
    of its own in front of it."""
    from spacefortress_amd import _lib
    P = played(N, GEOM)
    env = P.env
    assert not env.default_geometry
    want = P.after_step()
    fill = sentinel(N, S)
    buf = Guarded(N * S * FRAME)
    stack = buf.view.view(N, S, FRAME)
    for slot in range(S):
        for name, done in done_patterns(N, P.rng, with_null=True):
            stack.copy_(fill)
            assert L.sf_render_stack(env._h, _p(stack), S, slot, _p(done), env._stream()) == 0
            assert torch.equal(stack, M.render_stack(fill, want, slot, done)), (slot, name)
            assert buf.intact(), (slot, name)
    # sf_render_shift is the default geometry's
    pbuf = Guarded(N * S * FRAME)
    pbuf.view.copy_(fill.view(-1))
    stack.copy_(fill)
    done = torch.ones(N, dtype=torch.uint8, device=env.device)
    assert L.sf_render_shift(env._h, _p(pbuf.view), _p(stack), S, _p(done), env._stream()) == _lib.SF_ERR_ARG
    # the clear stores 16 bytes at a time: a stack that is only 4-byte aligned is refused when there are done flags ...
    off = Guarded(N * S * FRAME, shift=4)
    ostack = off.view.view(N, S, FRAME)
    ostack.copy_(fill)
    assert L.sf_render_stack(env._h, _p(ostack), S, S - 1, _p(done), env._stream()) == _lib.SF_ERR_ARG
    torch.cuda.synchronize()
    for b in (buf, pbuf, off):
        assert torch.equal(b.view, fill.view(-1)) and b.intact()
    # ... and taken without them (the renderer writes 32-bit words)
    assert L.sf_render_stack(env._h, _p(ostack), S, S - 1, None, env._stream()) == 0
    assert torch.equal(ostack, M.render_stack(fill, want, S - 1, None)) and off.intact()


# --------------------------------------------------------------------------------------------------------- (f) refusals
def test_refusals_leave_the_stack_alone(L, played):
    from spacefortress_amd import _lib
    N, S = 65, 4
    P = played(N)
    env = P.env
    want = P.after_step()
    fill = sentinel(N, S)
    nb = N * S * FRAME
    buf, off = Guarded(2 * nb + 2 * FRAME), Guarded(nb, shift=8)
    a, b = buf.view[:nb], buf.view[nb:2 * nb]  # two adjacent stacks: they touch, they do not intersect
    done = torch.ones(N, dtype=torch.uint8, device=env.device)
    pa, pb, st = a.data_ptr(), b.data_ptr(), env._stream()
    vp = C.c_void_p

    def untouched():
        torch.cuda.synchronize()
        return all(bool((x.view(N, S, FRAME) == fill).all()) for x in (a, b, off.view)) and buf.intact() and off.intact()

    for x in (a, b, off.view):
        x.copy_(fill.view(-1))
    buf.view[2 * nb:].copy_(fill.view(-1)[:2 * FRAME])
    for args in ((env._h, vp(pa), S, -1), (env._h, vp(pa), S, S), (env._h, vp(pa), 0, 0), (env._h, vp(pa), -2, 0),
                 (None, vp(pa), S, 0), (env._h, None, S, 0),
                 (env._h, vp(off.view.data_ptr()), S, 1)):  # the default geometry's stack is 16-byte aligned
        assert L.sf_render_stack(*args, _p(done), st) == _lib.SF_ERR_ARG, args[2:]
        assert untouched(), args[2:]
    for prev, stack in ((pa, pa),                          # one buffer
                        (off.view.data_ptr(), pa),         # a previous stack that is not 16-byte aligned
                        (pa, off.view.data_ptr()),         # a new one that is not
                        (pa + FRAME, pa), (pa, pa + FRAME),  # shifted by a frame either way: env e writes what env e + 1 reads
                        (pa + nb - 16, pa), (pa, pa + nb - 16),  # the last 16 bytes of one on the first of the other
                        (None, pa), (pa, None)):
        rc = L.sf_render_shift(env._h, vp(prev) if prev else None, vp(stack) if stack else None, S, _p(done), st)
        assert rc == _lib.SF_ERR_ARG, (prev and prev - pa, stack and stack - pa)
        assert untouched(), (prev and prev - pa, stack and stack - pa)
    assert L.sf_render_shift(None, vp(pa), vp(pb), S, _p(done), st) == _lib.SF_ERR_ARG and untouched()
    assert L.sf_render_shift(env._h, vp(pa), vp(pb), 0, _p(done), st) == _lib.SF_ERR_ARG and untouched()
    # adjacent stacks -- consecutive steps of DeviceRollout's storage -- are taken, in either order
    prev_fill = random_bytes((N, S, FRAME), 99)
    rnd = done_patterns(N, P.rng)[-1][1]
    for prev, stack in ((a, b), (b, a)):
        prev.copy_(prev_fill.view(-1))
        stack.copy_(fill.view(-1))
        assert L.sf_render_shift(env._h, _p(prev), _p(stack), S, _p(rnd), st) == 0
        assert torch.equal(stack.view(N, S, FRAME), M.render_shift(prev_fill, want, rnd))
        assert torch.equal(prev.view(N, S, FRAME), prev_fill) and buf.intact()
        assert torch.equal(buf.view[2 * nb:], fill.view(-1)[:2 * FRAME])  # (what lies behind the two)


# ------------------------------------------------------------------- the wrappers at other depths, staggered endings
def _staggered(sfa, N, S, geometry):
    """Two batches whose lane i ends its game i % (S + 3) steps from now: neighbouring lanes finish on consecutive steps,
    every tile mixes finished and unfinished envs, some lane ends while another lane's stack is still partly empty."""
    kw = dict(gametype="autoturn", obs_type="image", spawn_stride=2, image_geometry=geometry)
    env, twin = sfa.SFVecEnv(N, **kw), sfa.SFVecEnv(N, **kw)
    return env, twin, (34 * (5294 - (np.arange(N) % (S + 3)))).astype(np.int32)


def _trainer_update(current_obs, done, obs):
    """rl/train.py:87,92-93,51-56 on the trainer's float tensor (the shift through a copy: the tensors overlap)"""
    masks = 1.0 - (done != 0).float().view(-1, 1)
    current_obs *= masks.unsqueeze(2).unsqueeze(2)
    if current_obs.shape[1] > 1:
        current_obs[:, :-1] = current_obs[:, 1:].clone()
    current_obs[:, -1:] = obs.float()


def _mixed_within_a_tile(done):
    d = (done != 0).view(-1)
    tiles = [d[i:i + 64] for i in range(0, d.numel(), 64)]
    return any(bool(t.any()) and not bool(t.all()) for t in tiles)


GEOMETRIES = pytest.mark.parametrize("geometry", [None, GEOM], ids=["default", "quarter-scale"])


@GEOMETRIES
@pytest.mark.parametrize("S", [1, 2, 3, 5])
def test_frame_stack_wrapper_at_every_depth_with_staggered_endings(sfa, S, geometry):
    N = 130  # two tiles and a bit
    env, twin, clocks = _staggered(sfa, N, S, geometry)
    for e in (env, twin):
        e.set_field("time", clocks)
    fs = sfa.FrameStack(env, S)
    env.render("image", out=fs.ring[:, fs.head:fs.head + 1])  # no reset(): both start from the state just set
    cur = torch.zeros((N, S, 84, 84), device=env.device)
    cur[:, -1:] = twin.render("image").float()
    assert torch.equal(fs.stacked().float(), cur)
    rng = np.random.default_rng(40 + S)
    done_steps, mixed = [], 0
    for t in range(3 * (S + 3)):
        a = torch.from_numpy(rng.integers(0, 3, N).astype(np.uint8)).to(env.device)
        rew, done, info = fs.step(a)
        obs, r2, d2, i2 = twin.step_tensors(a)
        assert torch.equal(rew, r2) and torch.equal(done, d2.bool()) and torch.equal(info, i2.bool())
        _trainer_update(cur, d2, obs)
        assert torch.equal(fs.stacked().float(), cur), t
        if bool(d2.any()):
            done_steps.append(t)
            mixed += _mixed_within_a_tile(d2)
    assert len(done_steps) >= S + 3 and mixed >= S + 3, (done_steps, mixed)
    assert S == 1 or done_steps[0] + 1 < S  # a lane ended while the stacks held fewer than S frames
    env.close()
    twin.close()


@GEOMETRIES
@pytest.mark.parametrize("S", [2, 3, 5])
def test_device_rollout_at_other_depths_with_staggered_endings(sfa, S, geometry):
    """Two rollouts of 9 steps with after_update() between them.  On another geometry than the default this is the copy +
    sf_render_stack branch of DeviceRollout._step_record."""
    N, T = 130, 9
    env, twin, clocks = _staggered(sfa, N, S, geometry)
    ro = sfa.DeviceRollout(env, T, num_stack=S)
    assert ro.observations.shape == (T + 1, N, S, 84, 84)
    first = ro.reset()
    twin.reset()
    cur = torch.zeros((N, S, 84, 84), device=env.device)
    cur[:, -1:] = twin.render("image").float()
    assert torch.equal(first.float(), cur)
    for e in (env, twin):
        e.set_field("time", clocks)
    g = torch.Generator(device=env.device).manual_seed(50 + S)
    done_steps, mixed = [], 0
    for k in range(2):
        for t in range(T):
            a = torch.randint(0, 3, (N,), device=env.device, generator=g, dtype=torch.uint8)
            before = cur.clone()
            obs, rew, mask = ro.step(t, a)
            o2, r2, d2, i2 = twin.step_tensors(a)
            _trainer_update(cur, d2, o2)
            assert torch.equal(obs.float(), cur), (k, t)
            assert torch.equal(ro.observations[t].float(), before), (k, t)  # the step it came from is as it was
            assert torch.equal(rew[:, 0], r2.float()) and torch.equal(mask[:, 0] == 0, d2.bool())
            if bool(d2.any()):
                done_steps.append(T * k + t)
                mixed += _mixed_within_a_tile(d2)
        ro.after_update()
        assert torch.equal(ro.observations[0].float(), cur), k
    assert len(done_steps) >= S + 3 and mixed >= S + 3, (done_steps, mixed)
    assert done_steps[0] + 1 < S
    env.close()
    twin.close()
