"""The episode log (spacefortress_amd/episodes.py, sfmi.h: sf_eplog_*) without a GPU: the numpy model of an update
(tests/eplog_np.py) equals a plain loop over (row, env); quantiles out of the histogram equal the order statistics of the
samples and torch's lower median; the entry points are declared, bound and exported; and two gloo ranks reduce statistics and
histogram in one collective to what the concatenated returns give."""
import math
import os
import re
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT
from eplog_np import RECORD, LoopEpisodeLog, NpEpisodeLog, make_rows


@pytest.mark.parametrize("n,K,density,capacity", [(1, 1, 1.0, 1), (5, 3, 0.5, 4), (70, 2, 0.02, 16), (33, 7, 0.5, 64),
                                                  (300, 1, 1.0, 128), (9, 4, 0.0, 8), (40, 5, 0.3, 1000)])
def test_model_equals_the_plain_loop(n, K, density, capacity):
    """Several updates in a row (the accumulators carry over, an env can finish twice inside one update, the ring wraps and,
    where an update emits more than `capacity`, only the last `capacity` stay)."""
    rng = np.random.default_rng(n * 100 + K)
    a, b = NpEpisodeLog(n, capacity, -60, 100), LoopEpisodeLog(n, capacity, -60, 100)
    for u in range(4):
        dt = (np.uint8, np.int32, np.int64, None)[u]
        rew, done, info, act = make_rows(rng, K, n, density, dt)
        before = a.total
        recs, seq = a.update(rew, done, info, act)
        b.update(rew, done, info, act)
        assert a.total == b.total == before + int(done.sum()) and a.rows_seen == b.rows_seen == (u + 1) * K
        assert np.array_equal(a.ring, b.ring_array()), u
        assert a.hist.tolist() == b.hist and int(a.hist.sum()) == a.total
        assert a.acc.tolist() == b.acc
        assert np.array_equal(seq, before + np.arange(len(recs)))
        # the emitted records are in (row, env) order
        key = (recs["end_row"] - (a.rows_seen - K)) * n + recs["env"]
        assert np.all(np.diff(key) > 0)
    a.restart()
    assert not a.acc.any() and a.total == b.total


def test_an_env_that_finishes_twice_in_one_update():
    a = NpEpisodeLog(2, 8, -10, 21)
    rew = np.array([[1, 10], [2, 20], [3, 30], [4, 40]])
    done = np.array([[0, 0], [1, 0], [0, 0], [1, 1]])
    recs, _ = a.update(rew, done, np.zeros_like(rew), np.ones_like(rew))
    assert recs["env"].tolist() == [0, 0, 1] and recs["episode_return"].tolist() == [3, 7, 100]
    assert recs["length"].tolist() == [2, 2, 4] and recs["fire_actions"].tolist() == [2, 2, 4] and recs["end_row"].tolist() == [1, 3, 3]
    assert a.hist[13] == 1 and a.hist[17] == 1 and a.hist[20] == 1  # 100 saturates into the top bin
    assert RECORD.itemsize == 32


@pytest.mark.parametrize("seed", range(6))
def test_quantile_from_histogram_equals_the_order_statistic(seed):
    from spacefortress_amd.stats import quantile_from_histogram

    rng = np.random.default_rng(seed)
    lo, bins = -256, 512
    n = int(rng.integers(1, 400))
    x = rng.integers(lo + 1, lo + bins - 1, n)  # strictly inside: nothing in the end bins
    hist = np.bincount(x - lo, minlength=bins)
    for q in (0.0, 0.1, 0.25, 0.5, 0.75, 0.9, 0.99, 1.0):
        v, sat = quantile_from_histogram(hist, lo, q)
        assert v == int(np.sort(x)[max(1, math.ceil(q * n)) - 1]) and sat == 0, (q, n)
    assert quantile_from_histogram(torch.from_numpy(hist), lo, 0.5)[0] == int(torch.median(torch.from_numpy(x)))


def test_quantile_reports_saturation_and_an_empty_histogram():
    from spacefortress_amd.stats import quantile_from_histogram, summarize

    lo, bins = -4, 8  # bins for -4 .. 3
    x = np.array([-100, -1, 0, 2, 50])
    hist = np.bincount(np.clip(x - lo, 0, bins - 1), minlength=bins)
    v, sat = quantile_from_histogram(hist, lo, 0.5)
    assert v == 0 and sat == 2
    assert quantile_from_histogram(hist, lo, 1.0) == (3, 2)  # the top bin: the value is a bound, and says so
    assert quantile_from_histogram(np.zeros(bins, np.int64), lo, 0.5) is None
    vec = torch.tensor([5, int(x.sum()), int((x * x).sum()), 0, 0, 0, -100, 50])
    s = summarize(vec, hist, lo)
    assert s["median_return"] == 0 and s["saturated_returns"] == 2 and s["episodes"] == 5
    assert "median_return" not in summarize(vec) and summarize(vec) == {k: s[k] for k in summarize(vec)}
    assert "median_return" not in summarize(torch.tensor([0, 0, 0, 0, 0, 0, (1 << 63) - 1, -(1 << 63)]), np.zeros(bins, np.int64), lo)


def test_header_declares_the_log_and_the_table_binds_it():
    from spacefortress_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "sfmi.h")).read()
    assert "rl/train.py:158-165" in hdr and "rl/evaluate.py:82-99" in hdr
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    names = sorted(set(re.findall(r"\b(sf_eplog_[a-z_0-9]+)\s*\(", hdr)))
    assert names == ["sf_eplog_clear", "sf_eplog_create", "sf_eplog_destroy", "sf_eplog_read", "sf_eplog_restart", "sf_eplog_update"]
    for name in names:
        m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, hdr, flags=re.S)
        assert m, name
        n_args = len([a for a in m.group(1).split(",") if a.strip()])
        assert name in _lib.SYMBOLS and len(_lib.SYMBOLS[name][1]) == n_args, name
    assert "sf_episode_log.hip" in __import__("spacefortress_amd.build", fromlist=["SOURCES"]).SOURCES


def test_episode_log_is_exported():
    import spacefortress_amd
    from spacefortress_amd import episodes, stats
    from spacefortress_amd.vecenv import SFVecEnv

    assert "EpisodeLog" in spacefortress_amd.__all__ and spacefortress_amd.EpisodeLog is episodes.EpisodeLog
    for name in ("update", "restart", "clear", "drain", "histogram", "read"):
        assert callable(getattr(episodes.EpisodeLog, name)), name
    assert callable(SFVecEnv.enable_episode_log)
    assert callable(stats.quantile_from_histogram) and callable(stats.reduce_episode_log)
    assert episodes.RECORD_DTYPE == RECORD


def test_bad_sizes_are_refused_before_a_device_is_looked_for():
    """The argument checks of sf_eplog_create come first (sfmi.h): SF_ERR_ARG with a text, with or without a GPU."""
    import ctypes as C

    from spacefortress_amd import _lib
    from spacefortress_amd import build as sfbuild

    sfbuild.build()
    L = _lib.lib()
    h = C.c_void_p()
    for n, cap, bins in ((0, 8, 8), (-1, 8, 8), (4, 0, 8), (4, -3, 8), (4, 8, 0), (4, 8, 65537), ((1 << 26) + 1, 8, 8)):
        assert L.sf_eplog_create(n, cap, 0, bins, 1, 0, C.byref(h)) == _lib.SF_ERR_ARG, (n, cap, bins)
        assert "sf_eplog_create" in _lib.last_error() and not h.value
    assert L.sf_eplog_update(None, None, None, None, None, 0, 1, None) == _lib.SF_ERR_ARG
    assert L.sf_eplog_destroy(None) == _lib.SF_OK


# ---------------------------------------------------------------- two gloo ranks
BINS, LO = 128, -64


def _rank_returns(rank):
    return np.random.default_rng(40 + rank).integers(LO + 1, LO + BINS - 1, 31 + 10 * rank)


def _vector(x):
    return np.array([len(x), x.sum(), (x * x).sum(), 3, 2, 1, x.min(), x.max()], np.int64)


def worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sys.path.insert(0, ROOT)
    from spacefortress_amd.stats import reduce_episode_log

    calls = []
    real = dist.all_gather

    def counted(rows, t, *a, **k):
        calls.append(("all_gather", t.numel(), str(t.dtype)))
        return real(rows, t, *a, **k)

    dist.all_gather = counted
    for name in ("all_reduce", "broadcast", "reduce", "gather", "all_gather_into_tensor", "reduce_scatter", "all_to_all"):
        setattr(dist, name, (lambda nm: lambda *a, **k: calls.append((nm,)))(name))
    x = _rank_returns(rank)
    vec, hist = reduce_episode_log(torch.from_numpy(_vector(x)), torch.from_numpy(np.bincount(x - LO, minlength=BINS)))
    dist.all_gather = real
    q.put((rank, calls, vec.tolist(), hist.tolist()))
    dist.destroy_process_group()


def test_two_rank_gloo_reduction_is_one_collective_and_gives_the_median():
    from spacefortress_amd.stats import reduce_episode_log, summarize

    world, port = 2, 31500 + os.getpid() % 2000
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=240) for _ in range(world))
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    xs = [_rank_returns(r) for r in range(world)]
    both = np.concatenate(xs)
    for rank, calls, vec, hist in res:
        assert calls == [("all_gather", 8 + BINS, "torch.int64")], calls  # ONE collective of 8 + bins int64 values
        assert hist == sum(np.bincount(x - LO, minlength=BINS) for x in xs).tolist()
        v = _vector(both)
        v[3:6] *= world
        assert vec == v.tolist()
        s = summarize(torch.tensor(vec), torch.tensor(hist), LO)
        assert s["median_return"] == int(torch.median(torch.from_numpy(both))) == int(np.sort(both)[math.ceil(len(both) / 2) - 1])
        assert s["saturated_returns"] == 0 and s["episodes"] == len(both)
    # one process, no group: the identity
    v1, h1 = reduce_episode_log(torch.from_numpy(_vector(xs[0])), np.bincount(xs[0] - LO, minlength=BINS))
    assert v1.tolist() == _vector(xs[0]).tolist() and h1.tolist() == np.bincount(xs[0] - LO, minlength=BINS).tolist()
