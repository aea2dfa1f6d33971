"""The numpy model of include/sfmi_minibatch.h (tests/minibatchref.py) held to torch-on-CPU evaluation of the trainer's own
expressions: rl/train.py:107-108 for the advantages, rl/storage.py:65-122 for the minibatches (`flat[idx]`,
`t[:, idx].transpose(0, 1).reshape(...)`, BatchSampler's slices).  No GPU."""
import math

import numpy as np
import pytest
import torch
from torch.utils.data.sampler import BatchSampler, SubsetRandomSampler

import minibatchref as MR

f32 = np.float32


def _case(M, seed, scale=1.0, offset=0.0):
    r = np.random.default_rng([M, seed])
    return (r.standard_normal(M) * scale + offset).astype(f32), r.standard_normal(M).astype(f32)


@pytest.mark.parametrize("M", (2, 63, 257, 4097, 65537))
def test_advantages_model_against_the_trainers_expression(M):
    ret, val = _case(M, 1)
    raw, mean, std, out = MR.advantages_ref(ret, val)
    a = torch.from_numpy(ret) - torch.from_numpy(val)  # rl/train.py:107
    assert np.array_equal(raw.view(np.uint32), a.numpy().view(np.uint32))
    d = a.double()
    slack = M * MR.U64 * float(d.abs().sum()) / M  # torch's float64 reductions, in whatever order: M roundings at the worst
    assert abs(mean - float(d.mean())) <= slack + MR.stats_bounds(raw)[0]
    assert abs(std - float(d.std())) <= std * (M + 8) * MR.U64 + MR.stats_bounds(raw)[1]
    # rl/train.py:108 evaluated in float64: the header's float32 line rounds the mean (2^-24 |mean| in the numerator), the
    # difference, the std, eps, their sum and the quotient -- five roundings of the value itself, 2^-24 each
    t = ((d - d.mean()) / (d.std() + 1e-5)).numpy()
    u32 = 2.0 ** -24
    tol = 5 * u32 * np.abs(t) + u32 * abs(mean) / (std + 1e-5)
    assert (np.abs(out.astype(np.float64) - t) <= tol * 1.01).all()
    assert np.array_equal(MR.advantages_apply(raw, mean, std).view(np.uint32), out.view(np.uint32))


def test_advantages_model_edges():
    one = MR.advantages_ref(np.array([3.0], f32), np.array([1.0], f32))
    assert one[0][0] == 2.0 and one[1] == 2.0 and math.isnan(one[2]) and np.isnan(one[3]).all()  # torch.std of one element
    assert math.isnan(float(torch.tensor([2.0]).std()))
    c = MR.advantages_ref(np.full(1000, 1.7, f32), np.full(1000, 0.2, f32))
    assert c[2] == 0.0 and (c[3] == 0).all() and not np.signbit(c[3]).any()
    for special in (np.nan, np.inf, -np.inf):
        ret, val = _case(300, 2)
        ret[17] = special
        raw, mean, std, out = MR.advantages_ref(ret, val)
        assert np.isnan(out).all() and math.isnan(mean) and math.isnan(std)
        a = torch.from_numpy(ret) - torch.from_numpy(val)
        assert bool(torch.isnan((a - a.mean()) / (a.std() + 1e-5)).all())


def test_why_the_second_pass_exists():
    """Values near 1e6 that differ by 1e-1: sum x^2 - (sum x)^2 / M cancels fifteen digits away in float64 and is left with
    one or two, the second pass over (x - mean)^2 keeps all of them -- and stays inside the derived bound."""
    M = 4097
    r = np.random.default_rng(5)
    ret = (1e6 + 0.1 * r.integers(0, 2, M)).astype(f32)
    val = np.zeros(M, f32)
    raw, mean, std, _ = MR.advantages_ref(ret, val)
    x = raw.astype(np.float64)
    two_pass = math.sqrt(float(((x - x.sum() / M) ** 2).sum()) / (M - 1))  # plain float64, numpy's order
    one_pass = math.sqrt(max(0.0, float((x * x).sum()) - float(x.sum()) ** 2 / M) / (M - 1))
    bound = MR.stats_bounds(raw)[1]
    assert abs(two_pass - std) <= bound
    assert abs(one_pass - std) > 100 * bound
    assert 0.04 < std < 0.08


def test_stats_bounds_scale_with_the_operation_count():
    assert MR.sum_depth(1) == 10 and MR.sum_depth(256) == 10 and MR.sum_depth(257) == 11 and MR.sum_depth(327680) == 1289
    raw = np.random.default_rng(3).standard_normal(4097).astype(f32)
    bm, bs = MR.stats_bounds(raw)
    assert 0 < bm < 1e-12 and 0 < bs < 1e-12
    assert MR.stats_bounds(raw * f32(1024))[0] == pytest.approx(bm * 1024, rel=1e-12)


# ---------------------------------------------------------------------------------------------------------------- gather
def _storage(T, n, seed):
    r = np.random.default_rng([T, n, seed])
    return [r.standard_normal((T, n, 7)).astype(f32), r.integers(-5, 5, (T, n, 1)).astype(np.int64), r.standard_normal((T, n, 1)).astype(f32)]


@pytest.mark.parametrize("T,n,nmb", [(5, 64, 4), (5, 13, 4), (20, 257, 4), (1, 65, 3), (3, 7, 7)])
def test_flat_mode_is_flat_idx_over_batch_samplers_slices(T, n, nmb):
    batch = T * n
    cols = _storage(T, n, 1)
    flat = [c.reshape(batch, -1) for c in cols]
    perm = torch.randperm(batch, generator=torch.Generator().manual_seed(batch)).numpy()
    slices = MR.sampler_slices(batch, nmb)
    sampler = BatchSampler(SubsetRandomSampler(range(batch)), batch // nmb, drop_last=False)
    assert [len(b) for b in sampler] == [ln for _, ln in slices]
    assert sum(ln for _, ln in slices) == batch and slices[0][0] == 0
    for s, ln in slices:  # the short last minibatch: a gather of `ln` rows on the index from `s` on
        outs, g, bad = MR.gather_ref(flat, perm[s:], ln, ln, 0, 1)
        idx = torch.from_numpy(perm[s:s + ln])
        assert bad == 0 and np.array_equal(g, perm[s:s + ln])
        for o, f in zip(outs, flat):
            assert o.tobytes() == torch.from_numpy(f)[idx].numpy().tobytes()  # rl/storage.py:80-88
    if batch % nmb == 0:  # equal minibatches: the cursor picks the slice
        mb = batch // nmb
        for c in range(nmb):
            outs, g, bad = MR.gather_ref(flat, perm, batch, mb, c, nmb)
            assert bad == 0 and np.array_equal(g, perm[c * mb:(c + 1) * mb])


@pytest.mark.parametrize("T,n,nmb", [(5, 64, 4), (5, 13, 4), (7, 257, 8), (1, 65, 5)])
def test_trajectory_mode_is_the_recurrent_generators_cat(T, n, nmb):
    cols = _storage(T, n, 2)
    flat = [c.reshape(T * n, -1) for c in cols]
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n)).numpy()
    per = n // nmb
    for s in range(0, n, per):  # rl/storage.py:96-122, with the slicing DeviceRollout.recurrent_generator uses
        idx = perm[s:s + per]
        cnt = len(idx)
        outs, g, bad = MR.gather_ref(flat, perm[s:], cnt, cnt * T, 0, 1, T, n)
        assert bad == 0
        for o, c in zip(outs, cols):
            t = torch.from_numpy(c)
            want = t[:, torch.from_numpy(idx)].transpose(0, 1).reshape(-1, *t.shape[2:])
            assert o.tobytes() == want.numpy().tobytes()
        assert np.array_equal(g, (idx[:, None] + (np.arange(T) * n)[None, :]).reshape(-1))  # FrameRollout's flat_idx
    if n % nmb == 0:
        for c in range(nmb):
            _, g, bad = MR.gather_ref(flat, perm, n, per * T, c, nmb, T, n)
            assert bad == 0 and np.array_equal(g[::T], perm[c * per:(c + 1) * per])


def test_out_of_range_rows_are_zero_minus_one_and_counted():
    src = [np.arange(1, 41, dtype=f32).reshape(10, 4), np.arange(100, 110, dtype=np.int64).reshape(10, 1)]
    index = np.array([3, -1, 10, 9, 0, 3, 2 ** 40, -2 ** 40], np.int64)
    outs, g, bad = MR.gather_ref(src, index, 8, 8, 0, 1)
    assert g.tolist() == [3, -1, -1, 9, 0, 3, -1, -1] and bad == 4
    assert (outs[0][[1, 2, 6, 7]] == 0).all() and (outs[1][[1, 2, 6, 7]] == 0).all()
    assert np.array_equal(outs[0][[0, 3, 4, 5]], src[0][[3, 9, 0, 3]])  # duplicates are legal
    # beyond n_index: the last minibatch of an index that is too short
    outs, g, bad = MR.gather_ref(src, index, 6, 4, 1, 2)
    assert g.tolist() == [0, 3, -1, -1] and bad == 2
    # a cursor at or beyond n_batches: nothing but zero rows
    outs, g, bad = MR.gather_ref(src, index, 8, 4, 2, 2)
    assert (g == -1).all() and bad == 4 and not outs[0].any()
    # trajectory mode: the row is judged by g = t * n + e (T = 2, n = 5)
    _, g, bad = MR.gather_ref(src, np.array([4, 5, -1], np.int64), 3, 6, 0, 1, 2, 5)
    assert g.tolist() == [4, 9, 5, -1, -1, 4] and bad == 2


def test_the_binding_declares_what_the_header_declares():
    import os
    import re

    from spacefortress_amd import _lib
    import spacefortress_amd

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "sfmi_minibatch.h")).read(), flags=re.S)
    decl = {m.group(1): m.group(2) for m in re.finditer(r"\b(sf_[a-z_0-9]+)\s*\(([^)]*)\)\s*;", hdr)}
    assert set(decl) == set(_lib.MINIBATCH_SYMBOLS)
    for name, args in decl.items():
        assert len(_lib.MINIBATCH_SYMBOLS[name][1]) == len([a for a in args.split(",") if a.strip()]), name
        assert hasattr(_lib.lib(), name), name
    assert re.search(r"#define\s+SF_MB_MAX_COLUMNS\s+%d\b" % _lib.MB_MAX_COLUMNS, hdr)
    assert re.search(r"#define\s+SF_MB_MAX_ROW_BYTES\s+%d\b" % _lib.MB_MAX_ROW_BYTES, hdr)
    assert "MiniBatcher" in spacefortress_amd.__all__
    for name in ("advantages", "batcher", "minibatches"):
        assert callable(getattr(spacefortress_amd.DeviceRollout, name)) and callable(getattr(spacefortress_amd.FrameRollout, name))
    for name in ("shuffle", "next", "errors", "cursor"):
        assert callable(getattr(spacefortress_amd.MiniBatcher, name))
