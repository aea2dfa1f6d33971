"""include/sfmi_minibatch.h on the device: sf_advantages held to the header's arithmetic bit for bit and to exactly rounded
statistics within a derived bound; sf_minibatch_gather byte for byte against tests/minibatchref.py and against
feed_forward_generator / recurrent_generator; the device cursor under a captured graph; the example's new flags.

Every buffer a call writes lies between sentinel-filled guards (tests/trainerref.py)."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import minibatchref as MR
import trainerref as TR
from lockstep import sfa  # noqa: F401  (the fixture)

F = torch.float32
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def vp(p):
    return C.c_void_p(p) if p else None


def dev():
    return torch.device("cuda", torch.cuda.current_device())


# ------------------------------------------------------------------------------------------------------------ advantages
class Adv:
    """The buffers of one sf_advantages case, all guarded.  ret / val: float32 [M] (the call reads a prefix of longer tensors
    in the trainer; here the guards stand behind the M-th element)."""

    def __init__(self, ret, val):
        from spacefortress_amd import _lib
        self.lib, self.L, self.dev = _lib, _lib.lib(), dev()
        self.M = M = ret.size
        self.ret, self.val = TR.guarded(M, F, self.dev, ret), TR.guarded(M, F, self.dev, val)
        self.out, self.raw = TR.guarded(M, F, self.dev), TR.guarded(M, F, self.dev)
        self.stats = TR.guarded(2, torch.float64, self.dev)
        ws = int(self.L.sf_advantages_workspace_bytes(M))
        assert ws == 16 * ((M + 255) // 256)
        self.ws = TR.guarded(ws // 8, torch.float64, self.dev)
        self.outputs = (self.out, self.raw, self.stats, self.ws)
        self.all = self.outputs + (self.ret, self.val)

    def call(self, eps=1e-5, **over):
        a = dict(ret=self.ret.data_ptr(), val=self.val.data_ptr(), M=self.M, out=self.out.data_ptr(), raw=self.raw.data_ptr(),
                 stats=self.stats.data_ptr(), ws=self.ws.data_ptr())
        a.update(over)
        return self.L.sf_advantages(vp(a["ret"]), vp(a["val"]), a["M"], eps, vp(a["out"]), vp(a["raw"]), vp(a["stats"]), vp(a["ws"]),
                                    self.lib.raw_stream(self.dev))

    def host(self):
        torch.cuda.synchronize()
        TR.margins_intact(*self.all)
        return self.out.cpu().numpy(), self.raw.cpu().numpy(), self.stats.cpu().numpy()


def _adv_case(M, seed, scale=1.0):
    r = np.random.default_rng([M, seed, 77])
    return (r.standard_normal(M) * scale).astype(f32), r.standard_normal(M).astype(f32)


def _hold_advantages(ret, val, what, eps=1e-5):
    a = Adv(ret, val)
    assert a.call(eps) == 0, a.lib.last_error()
    out, raw, stats = a.host()
    torch_raw = (a.ret - a.val).cpu().numpy()  # torch's own subtraction on the device
    TR.assert_bits_equal(raw, torch_raw, (what, "raw"))
    m_raw, mean, std, _ = MR.advantages_ref(ret, val, eps)
    TR.assert_bits_equal(raw, m_raw, (what, "raw against the model"))
    # the header's float32 line, from the kernel's OWN statistics
    TR.assert_bits_equal(out, MR.advantages_apply(raw, stats[0], stats[1], eps), (what, "adv_out"))
    if a.M > 1 and np.isfinite(raw).all():
        bm, bs = MR.stats_bounds(raw)
        em, es = abs(stats[0] - mean), abs(stats[1] - std)
        print("%s: mean error %.3g (bound %.3g), std error %.3g (bound %.3g)" % (what, em, bm, es, bs))
        assert em <= bm and es <= bs, (what, em, bm, es, bs)
    # two calls give equal bits
    TR.refill(*a.outputs)
    assert a.call(eps) == 0
    out2, raw2, stats2 = a.host()
    assert out2.tobytes() == out.tobytes() and raw2.tobytes() == raw.tobytes() and stats2.tobytes() == stats.tobytes(), what
    return out, raw, stats


@pytest.mark.gpu
@pytest.mark.parametrize("M", MR.ADV_MS)
def test_advantages_equal_the_header_bit_for_bit_and_the_exact_statistics_within_the_bound(sfa, M):
    ret, val = _adv_case(M, 1)
    out, raw, stats = _hold_advantages(ret, val, "normal M=%d" % M)
    if M == 1:
        assert stats[0] == float(raw[0]) and math.isnan(stats[1]) and np.isnan(out).all()
    else:
        assert np.isfinite(out).all()
    if M >= 255:  # another scale, another eps, NULL raw_out and stats_out
        ret, val = _adv_case(M, 2, 1e3)
        want, _, _ = _hold_advantages(ret, val, "scaled M=%d" % M, eps=1e-3)
        a = Adv(ret, val)
        assert a.call(1e-3, raw=0, stats=0) == 0
        got, _, _ = a.host()
        assert got.tobytes() == want.tobytes() and TR.untouched(a.raw, a.stats)


@pytest.mark.gpu
@pytest.mark.parametrize("M", (2, 257, 65537))
def test_constant_input_gives_std_zero_and_exact_zeros(sfa, M):
    out, raw, stats = _hold_advantages(np.full(M, 1.7, f32), np.full(M, 0.2, f32), "constant M=%d" % M)
    assert stats[1] == 0.0 and stats[0] == float(f32(1.7) - f32(0.2))
    assert (out == 0).all() and not np.signbit(out).any()


@pytest.mark.gpu
def test_values_near_1e6_that_differ_by_a_tenth_show_why_the_second_pass_exists(sfa):
    M = 4097
    r = np.random.default_rng(5)
    ret, val = (1e6 + 0.1 * r.integers(0, 2, M)).astype(f32), np.zeros(M, f32)
    out, raw, stats = _hold_advantages(ret, val, "near 1e6")  # (inside the bound: asserted there)
    x = raw.astype(np.float64)
    one_pass = math.sqrt(max(0.0, float((x * x).sum()) - float(x.sum()) ** 2 / M) / (M - 1))
    _, _, std, _ = MR.advantages_ref(ret, val)
    assert abs(one_pass - std) > 100 * MR.stats_bounds(raw)[1]  # what sum x^2 - (sum x)^2 / M would have given
    assert 0.04 < stats[1] < 0.08  # (float32 near 1e6 steps by 0.0625: the values are 1e6 and 1e6 + 0.125)


@pytest.mark.gpu
@pytest.mark.parametrize("special", (np.nan, np.inf, -np.inf))
def test_one_nan_or_inf_gives_all_nan(sfa, special):
    for M, at in ((300, 17), (4097, 4096), (2, 0)):
        ret, val = _adv_case(M, 3)
        ret[at] = special
        out, raw, stats = _hold_advantages(ret, val, "special M=%d" % M)
        assert np.isnan(out).all() and math.isnan(stats[1])
        a = torch.from_numpy(ret).cuda() - torch.from_numpy(val).cuda()
        assert bool(torch.isnan((a - a.mean()) / (a.std() + 1e-5)).all())  # as in torch


@pytest.mark.gpu
def test_advantages_refusals_launch_nothing(sfa):
    from spacefortress_amd import _lib
    ret, val = _adv_case(300, 4)
    a = Adv(ret, val)
    for over in (dict(ret=0), dict(val=0), dict(out=0), dict(ws=0), dict(M=0), dict(M=-3), dict(ret=a.ret.data_ptr() + 2),
                 dict(val=a.val.data_ptr() + 1), dict(out=a.out.data_ptr() + 2), dict(raw=a.raw.data_ptr() + 2),
                 dict(stats=a.stats.data_ptr() + 4), dict(ws=a.ws.data_ptr() + 4)):
        assert a.call(**over) == _lib.SF_ERR_ARG, over
        assert _lib.last_error().startswith("sf_advantages:"), (over, _lib.last_error())
    torch.cuda.synchronize()
    assert TR.untouched(*a.outputs)
    TR.margins_intact(*a.all)
    assert int(a.L.sf_advantages_workspace_bytes(0)) == 0
    with pytest.raises(ValueError, match="sf_advantages"):
        _lib.check(a.call(ws=0))


@pytest.mark.gpu
def test_advantages_against_torchs_own_expression_a_record_not_a_gate(sfa):
    """torch's reduction order is not ours to fix: the largest difference in float32 ulps is printed (profiles/minibatch.md)
    and held only to the float32 roundings torch's own sums may make."""
    for M in (4097, 327680):
        ret, val = _adv_case(M, 6)
        a = Adv(ret, val)
        assert a.call() == 0
        out, raw, stats = a.host()
        t = a.ret - a.val
        want = ((t - t.mean()) / (t.std() + 1e-5)).cpu().numpy()
        ulp = np.spacing(np.abs(want).astype(f32)).astype(np.float64)
        diff = np.abs(out.astype(np.float64) - want.astype(np.float64))
        print("MINIBATCHREC advantages vs torch M=%d: largest difference %.2f ulp, %.3g absolute" % (M, float((diff / ulp).max()), diff.max()))
        # a float32 mean and std rounded a handful of times (2^-24 each) move every output by that much of |out| + |mean| / std
        assert (diff <= 64 * 2.0 ** -24 * (np.abs(want) + 1.0)).all()


# ---------------------------------------------------------------------------------------------------------------- gather
class Gather:
    """One sf_minibatch_gather case on raw buffers: columns of `row_bytes` bytes per row over n_rows_src rows of random words,
    guarded destinations (a destination of `off4` set lies 4 bytes off a 16-byte boundary), index, cursor, idx_out, errors."""

    def __init__(self, n_rows_src, row_bytes, mb, index, off4=(), seed=0):
        from spacefortress_amd import _lib
        self.lib, self.L, self.dev = _lib, _lib.lib(), dev()
        self.n_rows_src, self.mb, self.rb = n_rows_src, mb, list(row_bytes)
        r = np.random.default_rng([n_rows_src, mb, seed] + self.rb)
        self.src_np = [r.integers(1, 2 ** 31 - 1, (n_rows_src, b // 4), dtype=np.int32) for b in self.rb]  # (never a zero word)
        self.src = [torch.from_numpy(s).to(self.dev) for s in self.src_np]
        self.dst, self.dst_ptr = [], []
        for k, b in enumerate(self.rb):
            words = mb * b // 4
            t = TR.guarded(words + 8, torch.int32, self.dev)  # room to slide the destination by up to 7 words
            base = t.data_ptr()
            want = 4 if k in off4 else 0
            shift = ((want - base) % 16) // 4
            self.dst.append((t, shift, words))
            self.dst_ptr.append(base + 4 * shift)
            assert self.dst_ptr[-1] % 16 == want
        self.index = torch.from_numpy(np.ascontiguousarray(index)).to(self.dev)
        self.idx_type = 8 if self.index.dtype == torch.int64 else 4
        self.cursor = TR.guarded(1, torch.int32, self.dev, np.zeros(1, np.int32))
        self.idx_out = TR.guarded(mb, torch.int64, self.dev)
        self.errors = TR.guarded(1, torch.int64, self.dev, np.zeros(1, np.int64))
        self.tab = (_lib.MbColumn * len(self.rb))(*[_lib.MbColumn(s.data_ptr(), b, p) for s, b, p in zip(self.src, self.rb, self.dst_ptr)])

    def call(self, n_batches=1, traj=(0, 0), cursor=True, first=0, stream=None, **over):
        a = dict(tab=self.tab, n_cols=len(self.rb), n_rows_src=self.n_rows_src, index=self.index.data_ptr(), idx_type=self.idx_type,
                 n_index=self.index.numel(), mb=self.mb, cursor=self.cursor.data_ptr() if cursor else 0, first=first,
                 n_batches=n_batches, traj_T=traj[0], traj_n=traj[1], idx_out=self.idx_out.data_ptr(), errors=self.errors.data_ptr())
        if "cursor_ptr" in over:
            over["cursor"] = over.pop("cursor_ptr")
        a.update(over)
        return self.L.sf_minibatch_gather(a["tab"], a["n_cols"], a["n_rows_src"], vp(a["index"]), a["idx_type"], a["n_index"], a["mb"],
                                          vp(a["cursor"]), a["first"], a["n_batches"], a["traj_T"], a["traj_n"], vp(a["idx_out"]),
                                          vp(a["errors"]), stream or self.lib.raw_stream(self.dev))

    def host(self):
        """-> (the destinations as int32 [mb, words per row], idx_out, errors, cursor), guards and slack words checked."""
        torch.cuda.synchronize()
        TR.margins_intact(*[t for t, _, _ in self.dst], self.cursor, self.idx_out, self.errors)
        outs = []
        for (t, shift, words), b in zip(self.dst, self.rb):
            assert TR.untouched(t[:shift], t[shift + words:]), "a destination's neighbouring words were written"
            outs.append(t[shift:shift + words].cpu().numpy().reshape(self.mb, b // 4))
        return outs, self.idx_out.cpu().numpy(), int(self.errors.item()), int(self.cursor.item())

    def refill(self):
        TR.refill(*[t for t, _, _ in self.dst], self.idx_out)

    def hold(self, c, n_batches=1, traj=(0, 0), n_index=None, what=""):
        """The buffers as they stand against the model's minibatch c."""
        outs, idx_out, _, _ = self.host()
        n_index = self.index.numel() if n_index is None else n_index
        want, g, bad = MR.gather_ref(self.src_np, self.index.cpu().numpy(), n_index, self.mb, c, n_batches, traj[0], traj[1])
        assert np.array_equal(idx_out, g), (what, "idx_out")
        for k, (o, w) in enumerate(zip(outs, want)):
            assert o.tobytes() == w.tobytes(), (what, "column", k, self.rb[k])
        return bad


@pytest.mark.gpu
@pytest.mark.parametrize("mb", MR.GATHER_MBS)
@pytest.mark.parametrize("idx_dtype", (np.int32, np.int64))
def test_gather_every_row_width_eight_columns_at_once_and_one_alone(sfa, mb, idx_dtype):
    n_src = 300
    r = np.random.default_rng([mb, 9])
    index = r.integers(0, n_src, 2 * mb).astype(idx_dtype)  # duplicates from mb = 63 on at the latest (2 mb draws of 300)
    eight = Gather(n_src, MR.ROW_BYTES[:8], mb, index, off4=(1, 3, 5, 7))  # 4 .. 1024 bytes; 8, 16, 60, 1024 slid off alignment
    for c in (0, 1):
        eight.cursor.fill_(c)
        assert eight.call(n_batches=2) == 0, eight.lib.last_error()
        assert eight.hold(c, 2, what=("eight", mb, c)) == 0
        assert eight.host()[3] == (c + 1) % 2 and eight.host()[2] == 0
        eight.refill()
    aligned = Gather(n_src, (16, 96, 1024, 1028), mb, index)  # every 16-byte path (and 1028 beside it)
    assert aligned.call(cursor=False, first=1, n_batches=2) == 0
    assert aligned.hold(1, 2, what=("aligned", mb)) == 0
    for b, off in ((1028, ()), (4, ()), (1024, (0,))):  # one column alone
        one = Gather(n_src, (b,), mb, index, off4=off)
        assert one.call(cursor=False, first=0, n_batches=2) == 0
        assert one.hold(0, 2, what=("alone", b, mb)) == 0


@pytest.mark.gpu
@pytest.mark.parametrize("total,n_batches", [(64, 4), (65, 5), (20 * 257, 4)])
def test_a_permutation_of_every_transition_through_the_cursor(sfa, total, n_batches):
    perm = np.random.default_rng(total).permutation(total).astype(np.int64)
    mb = total // n_batches
    g = Gather(total, (96, 4, 8, 4, 4, 4, 4), mb, perm)  # the columns of a PPO minibatch
    seen = []
    for k in range(n_batches + 1):
        assert g.call(n_batches=n_batches) == 0
        assert g.hold(k % n_batches, n_batches, what=(total, k)) == 0
        outs, idx_out, errors, cursor = g.host()
        assert cursor == (k + 1) % n_batches and errors == 0
        seen.append(idx_out.copy())
        g.refill()
    assert np.array_equal(np.sort(np.concatenate(seen[:n_batches])), np.arange(total)) and np.array_equal(seen[0], seen[n_batches])


@pytest.mark.gpu
@pytest.mark.parametrize("T,n,n_batches", [(5, 64, 4), (7, 65, 5), (20, 257, 1)])
def test_trajectory_mode_env_by_env_step_by_step(sfa, T, n, n_batches):
    perm = np.random.default_rng([T, n]).permutation(n).astype(np.int32)
    per = n // n_batches
    g = Gather(T * n, (76, 4, 8, 1024), per * T, perm)
    for k in range(n_batches + 1):
        assert g.call(n_batches=n_batches, traj=(T, n)) == 0, g.lib.last_error()
        assert g.hold(k % n_batches, n_batches, traj=(T, n), what=("traj", T, n, k)) == 0
        _, idx_out, errors, cursor = g.host()
        e = perm[(k % n_batches) * per:(k % n_batches + 1) * per].astype(np.int64)
        assert np.array_equal(idx_out, (e[:, None] + (np.arange(T) * n)[None, :]).reshape(-1))  # recurrent_generator's cat
        assert cursor == (k + 1) % n_batches and errors == 0
        g.refill()
    # a short last minibatch: the envs that are left, a launch with fewer rows on the index from there on
    left = n - n_batches * per
    if left:
        short = Gather(T * n, (76, 4), left * T, perm[n_batches * per:])
        assert short.call(cursor=False, traj=(T, n)) == 0
        assert short.hold(0, 1, traj=(T, n), what="short trajectory minibatch") == 0


@pytest.mark.gpu
@pytest.mark.parametrize("idx_dtype", (np.int32, np.int64))
def test_out_of_range_rows_are_zero_minus_one_counted_and_alone(sfa, idx_dtype):
    total, mb = 65 * 3, 65
    index = np.random.default_rng(8).integers(0, total, 2 * mb).astype(idx_dtype)
    bad_at = {0: -1, 7: total, 63: -total, 64: total + 5, 66: np.iinfo(idx_dtype).max, 100: np.iinfo(idx_dtype).min}
    for k, v in bad_at.items():
        index[k] = v
    g = Gather(total, (4, 20, 96, 1024), mb, index, off4=(2,))
    # minibatch 0 (4 bad rows), minibatch 1 (2), then an index 30 short of minibatch 1: 30 more
    assert g.call(n_batches=2) == 0 and g.hold(0, 2, what="bad rows, minibatch 0") == 4
    outs, idx_out, errors, _ = g.host()
    assert errors == 4 and (idx_out[[0, 7, 63, 64]] == -1).all() and (idx_out >= 0).sum() == mb - 4
    for o in outs:
        assert not o[[0, 7, 63, 64]].any() and (o[[1, 6, 8, 62]] != 0).all()  # zero rows; their neighbours are whole rows
    g.refill()
    assert g.call(n_batches=2) == 0 and g.hold(1, 2, what="bad rows, minibatch 1") == 2
    assert g.host()[2] == 6
    g.refill()
    g.cursor.fill_(1)
    assert g.call(n_batches=2, n_index=2 * mb - 30) == 0
    assert g.hold(1, 2, n_index=2 * mb - 30, what="beyond n_index") == 1 + 30  # (index 66, and the rows from j = 100 on)
    outs, idx_out, errors, _ = g.host()
    assert errors == 6 + 31 and (idx_out[mb - 30:] == -1).all()
    # a cursor at or beyond n_batches: zero rows, all counted, the cursor stays
    g.refill()
    g.errors.zero_()
    for beyond in (2, 2 ** 31 - 1, -1):  # (-1: 0xFFFFFFFF, the cursor is unsigned)
        g.cursor.fill_(beyond)
        assert g.call(n_batches=2) == 0
        outs, idx_out, errors, cursor = g.host()
        assert (idx_out == -1).all() and not any(o.any() for o in outs) and cursor == beyond
    assert g.host()[2] == 3 * mb
    assert g.call(cursor=False, first=2, n_batches=2) == 0 and g.host()[2] == 4 * mb


@pytest.mark.gpu
def test_gather_refusals_launch_nothing(sfa):
    from spacefortress_amd import _lib
    index = np.arange(130, dtype=np.int64)
    g = Gather(130, (4, 96), 65, index)
    col = lambda **kw: (_lib.MbColumn * 1)(_lib.MbColumn(kw.get("src", g.src[0].data_ptr()), kw.get("rb", 4), kw.get("dst", g.dst_ptr[0])))
    nine = (_lib.MbColumn * 9)(*[_lib.MbColumn(g.src[0].data_ptr(), 4, g.dst_ptr[0])] * 9)
    cases = [dict(tab=None), dict(index=0), dict(n_cols=0), dict(tab=nine, n_cols=9), dict(n_rows_src=0), dict(n_index=-1), dict(mb=0),
             dict(mb=-4), dict(n_batches=0), dict(idx_type=2), dict(idx_type=0), dict(traj_T=-1), dict(traj_T=4, traj_n=130),
             dict(traj_T=5, traj_n=0), dict(traj_T=5, traj_n=25), dict(traj_T=13, traj_n=10, mb=64), dict(index=g.index.data_ptr() + 4),
             dict(cursor_ptr=g.cursor.data_ptr() + 2), dict(idx_out=g.idx_out.data_ptr() + 4), dict(errors=g.errors.data_ptr() + 4)]
    cases += [dict(tab=col(**kw), n_cols=1) for kw in (dict(src=0), dict(dst=0), dict(rb=0), dict(rb=6), dict(rb=65540), dict(rb=2),
                                                       dict(src=g.src[0].data_ptr() + 2), dict(dst=g.dst_ptr[0] + 1))]
    for over in cases:
        assert g.call(**over) == _lib.SF_ERR_ARG, over
        assert _lib.last_error().startswith("sf_minibatch_gather:"), (over, _lib.last_error())
    outs, idx_out, errors, cursor = g.host()
    assert TR.untouched(*[t for t, _, _ in g.dst], g.idx_out) and errors == 0 and cursor == 0
    with pytest.raises(ValueError, match="sf_minibatch_gather"):
        _lib.check(g.call(mb=0))


@pytest.mark.gpu
def test_gather_on_a_side_stream(sfa):
    index = np.random.default_rng(4).permutation(4 * 257).astype(np.int64)
    g = Gather(4 * 257, (96, 4, 8, 1028), 257, index, off4=(0,))
    side = torch.cuda.Stream(device=g.dev)
    side.wait_stream(torch.cuda.current_stream(g.dev))
    with torch.cuda.stream(side):
        for k in range(3):
            assert g.call(n_batches=4) == 0
            side.synchronize()
            assert g.hold(k, 4, what=("side stream", k)) == 0
            g.refill()
    assert g.host()[3] == 3


# ------------------------------------------------------------------------------------------------------------ the rollouts
def _fill(ro, seed):
    """Random contents for every tensor a minibatch reads (no env step needed: the gather copies bytes)."""
    gen = torch.Generator(device=ro.env.device).manual_seed(seed)
    rnd = lambda t: t.copy_(torch.randn(t.shape, generator=gen, device=t.device))
    for t in (ro.states, ro.returns, ro.value_preds, ro.action_log_probs):
        rnd(t)
    ro.masks.copy_((torch.rand(ro.masks.shape, generator=gen, device=ro.env.device) > 0.1).float())
    ro.actions.copy_(torch.randint(-2 ** 40, 2 ** 40, ro.actions.shape, generator=gen, device=ro.env.device))
    if hasattr(ro, "frames"):
        ro.frames.copy_(torch.randint(0, 256, ro.frames.shape, generator=gen, device=ro.env.device, dtype=torch.uint8))
        ro.starts.copy_((torch.rand(ro.starts.shape, generator=gen, device=ro.env.device) < 0.1).to(torch.uint8))
    else:
        rnd(ro.observations)


def _same(a, b, what):
    assert len(a) == len(b) == 7, what
    for k, (u, v) in enumerate(zip(a, b)):
        assert u.shape == v.shape and u.dtype == v.dtype, (what, k, u.shape, v.shape, u.dtype, v.dtype)
        assert u.contiguous().view(torch.uint8).cpu().numpy().tobytes() == v.contiguous().view(torch.uint8).cpu().numpy().tobytes(), (what, k)


def _eager(ro, adv, nmb, recurrent, seed, **kw):
    torch.manual_seed(seed)
    gen = ro.recurrent_generator if recurrent else ro.feed_forward_generator
    return [tuple(t.clone() for t in mb) for mb in gen(adv, nmb, **kw)]


def _perm_of(ro, recurrent, seed):
    """The permutation the generators draw after torch.manual_seed(seed)."""
    T, n = ro.rewards.shape[0:2]
    torch.manual_seed(seed)
    return torch.randperm(n if recurrent else T * n, device=ro.env.device)


@pytest.mark.gpu
@pytest.mark.parametrize("n,T,state_size", [(64, 5, 1), (257, 20, 256), (65, 3, 5)])
def test_device_rollout_minibatches_equal_the_generators_bit_for_bit(sfa, n, T, state_size):
    env = sfa.SFVecEnv(n, gametype="youturn", spawn_stride=1)
    ro = sfa.DeviceRollout(env, T, state_size=state_size)
    _fill(ro, n)
    adv = ro.advantages()
    # advantages(): the raw call's bits, the statistics on the device
    a = Adv(ro.returns[:-1].reshape(-1).cpu().numpy(), ro.value_preds[:-1].reshape(-1).cpu().numpy())
    assert a.call() == 0
    want, _, stats = a.host()
    assert adv.shape == (T, n, 1) and adv.dtype == F and adv.cpu().numpy().tobytes() == want.tobytes()
    assert ro.advantage_stats.cpu().numpy().tobytes() == stats.tobytes()
    keep = adv.clone()
    assert ro.advantages(out=adv).data_ptr() == adv.data_ptr() and torch.equal(adv, keep)
    for recurrent in (False, True):
        for nmb in (4, 7, 1):  # (7 leaves a short last minibatch wherever 7 does not divide)
            if recurrent and nmb > n:
                continue
            ref = _eager(ro, adv, nmb, recurrent, 11 * nmb)
            perm = _perm_of(ro, recurrent, 11 * nmb)
            got = [tuple(t.clone() for t in mb) for mb in ro.minibatches(adv, nmb, recurrent=recurrent, perm=perm)]
            assert len(got) == len(ref)
            for k, (x, y) in enumerate(zip(got, ref)):
                _same(x, y, ("fresh", recurrent, nmb, k))
            for k, mb in enumerate(ro.minibatches(adv, nmb, recurrent=recurrent, perm=perm.int(), reuse=True)):  # int32 indices
                _same(mb, ref[k], ("reuse", recurrent, nmb, k))
            torch.manual_seed(11 * nmb)  # without a perm: torch's own draw, as the generators make it
            for k, mb in enumerate(ro.minibatches(adv, nmb, recurrent=recurrent)):
                _same(mb, ref[k], ("own draw", recurrent, nmb, k))
    with pytest.raises(ValueError):
        ro.batcher(adv, 7 if (T * n) % 7 else 11)
    with pytest.raises(ValueError):
        ro.batcher(adv, 7 if n % 7 else 11, recurrent=True)
    with pytest.raises(ValueError):
        ro.batcher(adv.double(), 1)
    with pytest.raises(ValueError):
        list(ro.minibatches(adv, 4, perm=torch.arange(3, device=env.device)))
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("obs_dtype", (torch.uint8, torch.float16, torch.float32))
def test_frame_rollout_minibatches_equal_the_generators_bit_for_bit(sfa, obs_dtype):
    from spacefortress_amd import frame_rollout as fr
    n, T, S = 64, 5, 4
    env = sfa.SFVecEnv(n, gametype="youturn", obs_type="image", spawn_stride=1)
    ro = sfa.FrameRollout(env, T, num_stack=S)
    _fill(ro, 3)
    adv = ro.advantages()
    for recurrent in (False, True):
        for nmb in (4, 3):  # (3: a short last minibatch)
            perm = _perm_of(ro, recurrent, nmb)
            ref = _eager(ro, adv, nmb, recurrent, nmb, obs_dtype=obs_dtype, perm=perm)
            got = list(ro.minibatches(adv, nmb, recurrent=recurrent, perm=perm, obs_dtype=obs_dtype))
            assert len(got) == len(ref)
            for k, (x, y) in enumerate(zip(got, ref)):
                assert x[0].dtype == obs_dtype and x[0].shape[1:] == (S, 84, 84)
                _same(x, y, ("frames", recurrent, nmb, k))
        b = ro.batcher(adv, 4, recurrent=recurrent, obs_dtype=obs_dtype)
        perm = _perm_of(ro, recurrent, 9)
        ref = _eager(ro, adv, 4, recurrent, 9, obs_dtype=obs_dtype, perm=perm)
        b.shuffle(perm)
        for k in range(5):
            _same(b.next(), ref[k % 4], ("frame batcher", recurrent, k))
        assert b.cursor() == 1 and b.errors() == 0
    assert fr.gather_errors(env.device) == 0
    env.close()


@pytest.mark.gpu
@pytest.mark.parametrize("recurrent", (False, True))
def test_one_captured_next_yields_minibatch_after_minibatch(sfa, recurrent):
    """A graph that captured ONE batcher.next() is replayed 2 n_batches + 1 times: replay k leaves minibatch k % n_batches of
    the eager generator in the fixed buffers.  On the runtime's default queues: nothing about them is set here."""
    n, T, nmb = 64, 5, 4
    env = sfa.SFVecEnv(n, gametype="youturn", spawn_stride=1)
    ro = sfa.DeviceRollout(env, T, state_size=3)
    _fill(ro, 21)
    adv = ro.advantages()
    b = ro.batcher(adv, nmb, recurrent=recurrent)
    assert b.n_batches == nmb and b.tuple == (b.obs, b.states, b.actions, b.returns, b.masks, b.old_log_probs, b.adv_targ)
    ptrs = [t.data_ptr() for t in b.tuple]
    torch.manual_seed(5)
    b.shuffle()  # torch's own draw, in place
    assert torch.equal(b.index, _perm_of(ro, recurrent, 5)) and b.cursor() == 0
    ref = _eager(ro, adv, nmb, recurrent, 5)
    side = torch.cuda.Stream(device=env.device)
    side.wait_stream(torch.cuda.current_stream(env.device))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        b.next()  # warm-up
        side.synchronize()
        _same(b.tuple, ref[0], "eager next")
        b.shuffle(b.index.clone())  # (the same order, the cursor back at 0)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            b.next()
    torch.cuda.current_stream(env.device).wait_stream(side)
    torch.cuda.synchronize()
    assert b.cursor() == 0  # (capturing launches nothing)
    for k in range(2 * nmb + 1):
        g.replay()
        torch.cuda.synchronize()
        _same(b.tuple, ref[k % nmb], ("replay", k))
        assert b.cursor() == (k + 1) % nmb
    assert [t.data_ptr() for t in b.tuple] == ptrs
    # shuffle() between replays takes effect and zeroes the cursor
    perm2 = _perm_of(ro, recurrent, 6)
    ref2 = _eager(ro, adv, nmb, recurrent, 6)
    b.shuffle(perm2)
    assert b.cursor() == 0
    for k in range(nmb + 1):
        g.replay()
        torch.cuda.synchronize()
        _same(b.tuple, ref2[k % nmb], ("replay after shuffle", k))
    # new advantages in place reach the next replay
    adv.mul_(2.0)
    b.shuffle(perm2)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(b.adv_targ, ref2[0][6] * 2.0)
    # a cursor beyond n_batches: zero rows, counted
    assert b.errors() == 0
    b.set_cursor(nmb)
    g.replay()
    torch.cuda.synchronize()
    assert all(not bool(t.view(torch.uint8).any()) for t in b.tuple) and bool((b.idx_out == -1).all())
    assert b.errors(clear=True) == b.rows and b.errors() == 0 and b.cursor() == nmb
    env.close()


# ------------------------------------------------------------------------------------------------------------- the example
def _example(*flags):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "ppo_loop.py"), "--envs", "256", "--steps", "16", "--iters", "2",
                          *flags], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


def _finite_losses(text):
    m = re.findall(r"last minibatch: loss (\S+), policy loss (\S+), value loss (\S+), entropy (\S+), bad rows (\d+)", text)
    assert m, text
    for *vals, bad in m:
        assert all(math.isfinite(float(v.rstrip(","))) for v in vals) and int(bad) == 0, text


@pytest.mark.gpu
@pytest.mark.parametrize("flags", (("--obs", "features"), ("--obs", "image"), ("--obs", "features", "--device-policy-head")))
def test_the_example_trains_on_device_minibatches(sfa, flags):
    text = _example(*flags, "--device-minibatches")
    assert "iter   2" in text
    if "--device-policy-head" in flags:
        _finite_losses(text)
    else:  # torch.distributions on the gathered minibatches: the loss of the last one
        m = re.findall(r"last minibatch: loss (\S+)", text)
        assert m and all(math.isfinite(float(v)) for v in m), text


@pytest.mark.gpu
def test_the_example_replays_one_captured_update(sfa):
    text = _example("--graph-update")
    assert "iter   2" in text and "graph" in text
    _finite_losses(text)
