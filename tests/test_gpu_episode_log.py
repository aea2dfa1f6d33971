"""The episode log on the device (sfmi.h: sf_eplog_*, csrc/sf_episode_log.hip, spacefortress_amd/episodes.py) held to the
numpy statement of its contract (tests/eplog_np.py), exactly: ring bytes, histogram, totals -- on synthetic arrays through the
stand-alone ABI at every launch shape, in a captured graph, and behind every stepping path of a real batch."""
import ctypes as C
import math

import numpy as np
import pytest

from eplog_np import RECORD, NpEpisodeLog, make_rows
from lockstep import sfa

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FIELDS = ("env", "episode_return", "length", "kills", "fire_actions", "end_row")
ACT_DTYPES = (np.uint8, np.int32, np.int64, None)


def _p(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


class AbiLog:
    """The six entry points on raw pointers, nothing else."""

    def __init__(self, n, capacity, hist_lo, bins, fire_action=1):
        from spacefortress_amd import _lib
        self._lib, self.L = _lib, _lib.lib()
        self.n, self.capacity, self.bins = n, capacity, bins
        self.h = C.c_void_p()
        _lib.check(self.L.sf_eplog_create(n, capacity, hist_lo, bins, fire_action, torch.cuda.current_device(), C.byref(self.h)))

    def update(self, rew, done, info, act):
        dev = torch.device("cuda")
        t = [torch.from_numpy(np.ascontiguousarray(x)).to(dev) if x is not None else None for x in (rew, done, info, act)]
        at = act.dtype.itemsize if act is not None else 0
        self._lib.check(self.L.sf_eplog_update(self.h, _p(t[0]), _p(t[1]), _p(t[2]), _p(t[3]), at, rew.shape[0], None))
        return t  # (kept alive by the caller until the read)

    def read(self):
        total, rows = C.c_uint64(), C.c_uint64()
        ring, hist = np.zeros(self.capacity, RECORD), np.zeros(self.bins, np.int64)
        self._lib.check(self.L.sf_eplog_read(self.h, C.byref(total), C.byref(rows), ring.ctypes.data_as(C.c_void_p),
                                             hist.ctypes.data_as(C.c_void_p), None))
        return int(total.value), int(rows.value), ring, hist

    def close(self):
        self.L.sf_eplog_destroy(self.h)


def _run_case(n, K, density, capacity, seed, hist=(-60, 100)):
    """Three updates, read, compare; a fourth, and its records sit where the model says.  Returns the ring bytes."""
    rng = np.random.default_rng(seed)
    dev_log, model = AbiLog(n, capacity, *hist), NpEpisodeLog(n, capacity, *hist)
    keep = []
    try:
        for u in range(3):
            rows = make_rows(rng, K, n, density, ACT_DTYPES[(u + seed) % 4])
            keep.append(dev_log.update(*rows))
            model.update(*rows)
        total, seen, ring, histo = dev_log.read()
        assert (total, seen) == (model.total, model.rows_seen), (n, K, density)
        assert ring.tobytes() == model.ring.tobytes(), (n, K, density)
        assert np.array_equal(histo, model.hist) and int(histo.sum()) == total
        rows = make_rows(rng, K, n, density, ACT_DTYPES[(3 + seed) % 4])
        keep.append(dev_log.update(*rows))
        recs, seq = model.update(*rows)
        total, seen, ring, histo = dev_log.read()
        assert (total, seen) == (model.total, model.rows_seen) and np.array_equal(histo, model.hist)
        live = seq >= total - capacity
        assert np.array_equal(ring[seq[live] % capacity], recs[live]), (n, K, density)
        assert ring.tobytes() == model.ring.tobytes()
        return ring.tobytes()
    finally:
        dev_log.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 4097])
def test_kernel_equals_the_model_on_synthetic_rows(sfa, n):
    """The wave edge (63 / 64 / 65), the workgroup edge (255 / 256 / 257), 17 tiles in the scan (4097: the last tile holds one
    env), tiles without an end beside full ones (density 0.02), envs that finish twice inside one update (K = 7 at density
    0.5 and 1), a ring that wraps and one that overflows within a launch (capacity 1000 below 3 * K * n at the large shapes)."""
    seed = 0
    for K in (1, 2, 7):
        for density in (0.0, 0.02, 0.5, 1.0):
            _run_case(n, K, density, 1000, seed)
            seed += 1


@pytest.mark.parametrize("n,K", [(257, 33), (70, 70)])
def test_more_rows_than_one_group_of_launches(sfa, n, K):
    """Beyond SF_EPLOG_ROWS = 32 rows the update goes through count / scan / apply again: same sequence numbers."""
    _run_case(n, K, 0.3, 4096, 11)
    _run_case(n, K, 1.0, 500, 12)


def test_more_ends_than_slots(sfa):
    n = 300
    one = np.ones((1, n), np.uint8)
    rew = np.arange(n, dtype=np.int32).reshape(1, n) - 100
    log = sfa.EpisodeLog(n, "cuda", capacity=128, hist=(-128, 512))
    t = [torch.from_numpy(x).cuda() for x in (rew, one, one)]
    log.update(*t)
    total, seen, ring, _ = log.read()
    assert total == 300 and seen == 1
    seq = np.arange(172, 300)
    assert np.array_equal(ring[seq % 128]["env"], seq) and np.array_equal(ring[seq % 128]["episode_return"], seq - 100)
    log.update(*t)
    d = log.drain()
    assert d["dropped"] == 600 - 128 and np.array_equal(d["env"], seq) and np.array_equal(d["seq"], np.arange(472, 600))
    assert np.array_equal(d["end_row"], np.ones(128)) and np.array_equal(d["length"], np.ones(128)) and np.array_equal(d["kills"], np.ones(128))
    log.update(*t)
    d = log.drain()
    assert d["dropped"] == 172 and np.array_equal(d["env"], seq) and log.total == 900
    assert log.drain()["dropped"] == 0 and len(log.drain()["env"]) == 0
    assert int(log.histogram().sum()) == 900
    log.close()
    last = sfa.EpisodeLog(n, "cuda", capacity=1, hist=(-128, 512))
    last.update(*t)
    total, _, ring, _ = last.read()
    assert total == 300 and ring["env"].tolist() == [299] and ring["episode_return"].tolist() == [199]
    d = last.drain()
    assert d["dropped"] == 299 and d["env"].tolist() == [299]
    last.close()


def test_histogram_end_bins_saturate(sfa):
    rew = np.array([[-1000, -5, 0, 5, 1000, 3, -4, 2]], np.int32)
    n = rew.shape[1]
    log = sfa.EpisodeLog(n, "cuda", capacity=16, hist=(-4, 8))  # bins for the returns -4 .. 3
    ones = torch.ones((1, n), dtype=torch.uint8, device="cuda")
    log.update(torch.from_numpy(rew).cuda(), ones, ones)
    h = log.histogram()
    assert h.tolist() == [3, 0, 0, 0, 1, 0, 1, 3] and int(h.sum()) == log.total == n
    from spacefortress_amd.stats import quantile_from_histogram
    assert quantile_from_histogram(h, -4, 0.5) == (0, 6)
    log.clear()
    assert log.total == 0 and not log.histogram().any() and log.rows_seen == 0
    log.close()


def test_the_same_rows_give_the_same_ring_bytes(sfa):
    a = _run_case(4097, 7, 0.5, 1000, 5)
    b = _run_case(4097, 7, 0.5, 1000, 5)
    assert a == b
    c = _run_case(4097, 7, 0.5, 100000, 5)  # nothing overwritten: every record of the four updates
    assert c == _run_case(4097, 7, 0.5, 100000, 5)


def test_update_in_a_captured_graph(sfa):
    """One update captured on a side stream (a single linear stream), replayed three times = the model fed the rows three
    times: total and rows_seen advance on the device."""
    n, K = 1000, 3
    rng = np.random.default_rng(21)
    rows = make_rows(rng, K, n, 0.3, np.int64)
    t = [torch.from_numpy(x).cuda() for x in rows]
    log = sfa.EpisodeLog(n, "cuda", capacity=512, hist=(-60, 100))
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):  # (the kernels' code objects are loaded before the capture)
        log.update(*t)
        log.clear()
    side.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        log.update(*t)
    torch.cuda.synchronize()
    assert log.total == 0  # (a capture runs nothing)
    model = NpEpisodeLog(n, 512, -60, 100)
    for _ in range(3):
        g.replay()
        model.update(*rows)
    torch.cuda.synchronize()
    total, seen, ring, hist = log.read()
    assert (total, seen) == (model.total, 9) and ring.tobytes() == model.ring.tobytes() and np.array_equal(hist, model.hist)
    del g
    log.close()


# ---------------------------------------------------------------- a real batch
def _staggered(sfa, n=256, **kw):
    """A fresh batch whose env e ends its game d_e = 3 + e % 17 steps from here, with a log (set_field goes through _touch:
    the accumulators start over)."""
    env = sfa.SFVecEnv(n, **kw)
    log = env.enable_episode_log()
    d = 3 + np.arange(n) % 17
    env.set_field("time", (34 * (5295 - d)).astype(np.int32))
    return env, log


def _actions(n, T, n_actions, seed, dtype=torch.int64):
    rng = np.random.default_rng(seed)
    return torch.from_numpy(rng.integers(0, n_actions, (T, n))).to(dtype).cuda()


def _same_records(a, b):
    for k in FIELDS + ("seq",):
        assert np.array_equal(a[k], b[k]), k
    assert a["dropped"] == b["dropped"] == 0


def test_a_real_batch_against_the_host_accumulation(sfa):
    from spacefortress_amd.stats import summarize
    n, T = 256, 40
    env, log = _staggered(sfa, n, obs_type="features")
    base = env.episode_stats()
    acts = _actions(n, T, env.n_actions, 3)
    host = []
    for t in range(T):
        _, r, d, i = env.step_tensors(acts[t])
        host.append((r.cpu().numpy().copy(), d.cpu().numpy().copy(), i.cpu().numpy().copy()))
    rew, done, info = (np.stack([h[k] for h in host]) for k in range(3))
    model = NpEpisodeLog(n, log.capacity, log.hist_lo, log.bins)
    recs, seq = model.update(rew, done, info, acts.cpu().numpy())  # (one [T, n] update = T updates of a row)
    got = log.drain()
    assert len(recs) >= n and got["dropped"] == 0  # every env finished (at least) once
    for k in FIELDS:
        assert np.array_equal(got[k], recs[k]), k
    assert np.array_equal(got["seq"], seq)
    assert np.all(np.diff(got["end_row"] * n + got["env"]) > 0)  # (step, env) order
    assert np.array_equal(log.histogram(), model.hist) and log.total == len(recs) and log.rows_seen == T
    after = env.episode_stats()
    ret = got["episode_return"].astype(np.int64)
    assert after[0] - base[0] == len(ret) and after[1] - base[1] == ret.sum() and after[2] - base[2] == (ret * ret).sum()
    assert after[3] - base[3] == got["kills"].sum()
    assert after[6] == ret.min() and after[7] == ret.max()
    s = summarize(after, log.histogram(), log.hist_lo)
    assert s["median_return"] == int(np.sort(ret)[math.ceil(len(ret) / 2) - 1]) == int(torch.median(torch.from_numpy(ret)))
    assert (got["fire_actions"] > 0).any() and got["length"].min() >= 3
    env.close()


def test_every_stepping_path_reports(sfa):
    n, T = 256, 24
    ref_env, ref_log = _staggered(sfa, n, obs_type="features")
    acts = _actions(n, T, ref_env.n_actions, 4)
    for t in range(T):
        ref_env.step_tensors(acts[t])
    want = ref_log.drain()
    assert len(want["env"]) >= n

    env, log = _staggered(sfa, n, obs_type="features")  # rollout([K, N])
    env.rollout(acts, want_obs=False)
    _same_records(log.drain(), want)
    env.close()

    ro_env = sfa.SFVecEnv(n, obs_type="features")  # DeviceRollout.step
    ro = sfa.DeviceRollout(ro_env, T)
    ro.reset()
    log = ro_env.enable_episode_log()
    ro_env.set_field("time", (34 * (5295 - (3 + np.arange(n) % 17))).astype(np.int32))
    for t in range(T):
        ro.step(t, acts[t])
    _same_records(log.drain(), want)
    ro_env.close()

    env, log = _staggered(sfa, n, obs_type="features")  # SFVecNormalize's fused step
    vn = sfa.SFVecNormalize(env)
    for t in range(T):
        vn.step_tensors(acts[t])
    _same_records(log.drain(), want)
    env.close()

    # the sampled paths: what they played comes from their actions_out
    env, log = _staggered(sfa, n, obs_type="features")
    env.seed_actions(9)
    sampled = env.rollout_sampled(T, want_obs=False, want_actions=False)[4]
    assert sampled is not None and sampled.shape == (T, n)  # (allocated for the log)
    got_rs = log.drain()
    env.close()
    env, log = _staggered(sfa, n, obs_type="features")
    env.seed_actions(9)
    played = torch.empty((T, n), dtype=torch.uint8, device=env.device)
    for t in range(T):
        if t % 2:
            env.step_sampled(actions_out=played[t])
        else:
            env.step_sampled()  # (the log gets a buffer of its own)
            played[t] = sampled[t]
    assert torch.equal(played, sampled)
    got_ss = log.drain()
    env.close()
    env, log = _staggered(sfa, n, obs_type="features")
    for t in range(T):
        env.step_tensors(sampled[t])
    want_s = log.drain()
    _same_records(got_rs, want_s)
    _same_records(got_ss, want_s)

    # reset() in mid-episode drops the partial sums and keeps the finished records
    for t in range(3):
        env.step_tensors(sampled[t])
    before = log.read()
    env.reset()
    _, r, d, i, a = (x.cpu().numpy() if x is not None else None for x in env.rollout_sampled(5300, want_obs=False))
    got = log.drain()
    assert d.sum(0).tolist() == [1] * n  # one whole game each, counted from the reset and not from three steps before it
    first = (d != 0).argmax(0)
    upto = np.arange(len(d))[:, None] <= first[None]
    order = np.argsort(first * n + np.arange(n), kind="stable")
    assert np.array_equal(got["env"], order) and np.array_equal(got["length"], first[order] + 1)
    assert np.array_equal(got["episode_return"], (r * upto).sum(0)[order]) and np.array_equal(got["kills"], (i * upto).sum(0)[order])
    assert np.array_equal(got["fire_actions"], ((a == 1) & upto).sum(0)[order])
    now = log.read()
    assert now[0] == before[0] + n and np.array_equal(now[2][:before[0]], before[2][:before[0]])
    env.close()
    ref_env.close()


def test_frame_stack_reports(sfa):
    n, T = 64, 24
    ref_env, ref_log = _staggered(sfa, n, obs_type="image")
    acts = _actions(n, T, ref_env.n_actions, 5, torch.uint8)
    for t in range(T):
        ref_env.step_tensors(acts[t])
    want = ref_log.drain()
    env = sfa.SFVecEnv(n, obs_type="image")
    fs = sfa.FrameStack(env, 4)
    fs.reset()
    log = env.enable_episode_log()
    env.set_field("time", (34 * (5295 - (3 + np.arange(n) % 17))).astype(np.int32))
    for t in range(T):
        fs.step(acts[t])
    got = log.drain()
    assert len(got["env"]) >= n
    _same_records(got, want)
    env.close()
    ref_env.close()


def test_bad_arguments_launch_nothing(sfa):
    from spacefortress_amd import _lib
    L = _lib.lib()
    h = C.c_void_p()
    dev = torch.cuda.current_device()
    for n, cap, bins in ((0, 8, 8), (4, 0, 8), (4, 8, 0), (4, 8, 65537)):
        assert L.sf_eplog_create(n, cap, 0, bins, 1, dev, C.byref(h)) == _lib.SF_ERR_ARG
        assert "sf_eplog_create" in _lib.last_error()
    assert L.sf_eplog_create(4, 8, 0, 8, 1, 10 ** 6, C.byref(h)) == _lib.SF_ERR_ARG  # no such device
    log = AbiLog(4, 8, 0, 8)
    ones = torch.ones((1, 4), dtype=torch.uint8, device="cuda")
    rew = torch.ones((1, 4), dtype=torch.int32, device="cuda")
    for K in (0, -1):
        assert L.sf_eplog_update(log.h, _p(rew), _p(ones), _p(ones), None, 0, K, None) == _lib.SF_ERR_ARG
        assert "K >= 1" in _lib.last_error()
    assert L.sf_eplog_update(log.h, _p(rew), _p(ones), _p(ones), _p(ones), 2, 1, None) == _lib.SF_ERR_ARG  # act_type
    assert L.sf_eplog_update(log.h, None, _p(ones), _p(ones), None, 0, 1, None) == _lib.SF_ERR_ARG
    total, seen, ring, hist = log.read()
    assert total == 0 and seen == 0 and not hist.any() and ring.tobytes() == bytes(ring.nbytes)
    log.close()
    with pytest.raises(ValueError):
        sfa.EpisodeLog(4, "cuda", capacity=0)
    ok = sfa.EpisodeLog(4, "cuda", capacity=8)
    with pytest.raises(ValueError):
        ok.update(rew.float(), ones, ones)
    with pytest.raises(ValueError):
        ok.update(rew[:, :3].contiguous(), ones[:, :3].contiguous(), ones[:, :3].contiguous())
    ok.close()
