"""Episode statistics across GPUs.

The batch shards over GPUs as independent lane ranges (no state is shared between envs), so the
only cross-rank traffic of the whole path is this: the 8-element episode-statistics vector each
batch accumulates on its device (sfmi.h: sf_episode_stats) and, with an episode log (episodes.py), its histogram of
episode returns, reduced with RCCL over xGMI (`torch.distributed` backend "nccl", one all-gather) -- or gloo on CPU
tensors in the tests.  One call per log interval; the message is 64 bytes (+ 8 per histogram bin), latency-bound.

What this covers of the trainer's log line (rl/train.py:158-165) and `num_destruction += sum(info)` (rl/train.py:81), and
what it does not:
    fortress_kills                        the same quantity as num_destruction (before the trainer divides it by num_processes).
    mean / min / max / std_return         over the EPISODES that finished in the interval, on the engine's integer rewards.
    median_return                         likewise over the episodes finished in the interval (lower median, from the episode
                                          log's histogram; exact while no return falls into a saturating end bin).
The trainer's `final_rewards.mean() / .median() / .min() / .max()` are over ENVS: one entry per env, the return of its last
finished episode (0 until it has finished one), on the rewards the trainer saw.  That exact quantity is
`DeviceRollout.final_rewards`; the two agree only when every env finished exactly one episode in the interval.
"""
import math

import torch

# layout of the vector (include/sfmi.h)
EPISODES, SUM_RETURN, SUM_SQ_RETURN, FORT_KILLS, SHIP_DEATHS, SHOTS, MIN_RETURN, MAX_RETURN = range(8)
INT64_MAX = (1 << 63) - 1
INT64_MIN = -(1 << 63)


def shard_lanes(total_envs, world_size, rank):
    """Contiguous lane range [begin, end) of `rank`: the first `total % world` ranks get one more."""
    if world_size <= 0 or not 0 <= rank < world_size:
        raise ValueError("bad rank/world_size")
    base, extra = divmod(int(total_envs), int(world_size))
    begin = rank * base + min(rank, extra)
    return begin, begin + base + (1 if rank < extra else 0)


def reduce_episode_stats(local, group=None, force=False):
    """Reduce one rank's statistics vector (int64[8], any device) over all ranks: sums for the six counters,
    min / max for the two extremes.  ONE collective -- an all-gather of the 64-byte vectors -- and the fold is
    done locally in rank order (deterministic).  Returns the reduced tensor on the same device."""
    import torch.distributed as dist

    v = torch.as_tensor(local, dtype=torch.int64).clone()
    # force: run the collective for a single rank too (rehearsing the RCCL path on a one-GPU box)
    if dist.is_available() and dist.is_initialized() and (dist.get_world_size(group) > 1 or force):
        rows = [torch.empty_like(v) for _ in range(dist.get_world_size(group))]
        dist.all_gather(rows, v.contiguous(), group=group)
        m = torch.stack(rows)
        v = torch.cat([m[:, :6].sum(0), m[:, 6:7].min(0).values, m[:, 7:8].max(0).values])
    return v


def quantile_from_histogram(hist, hist_lo, q):
    """(v, saturated) from an episode log's histogram (bin b counts the returns hist_lo + b): v = the smallest value with
    count(<= v) >= ceil(q * n), i.e. sorted(x)[ceil(q * n) - 1] (q = 0.5: torch's lower median, what `final_rewards.median()`
    returns; q = 0: the minimum); saturated = how many counts sit in the two end bins, which also hold everything beyond
    them -- v is exact when it lies strictly between them.  None when the histogram is empty."""
    h = [int(x) for x in torch.as_tensor(hist).reshape(-1).tolist()]
    n = sum(h)
    if n == 0:
        return None
    if not 0.0 <= q <= 1.0:
        raise ValueError("q must lie in [0, 1]")
    need = max(1, math.ceil(q * n))
    saturated = h[0] + h[-1] if len(h) > 1 else h[0]
    c = 0
    for b, k in enumerate(h):
        c += k
        if c >= need:
            return int(hist_lo) + b, saturated
    raise AssertionError("unreachable")


def reduce_episode_log(stats_vec, hist, group=None, force=False):
    """reduce_episode_stats and the element-wise sum of the ranks' return histograms in ONE collective: an all-gather of
    8 + bins int64 values, folded locally in rank order.  Returns (vec int64[8], hist int64[bins]) on the inputs' device."""
    import torch.distributed as dist

    v = torch.as_tensor(stats_vec, dtype=torch.int64).reshape(-1)
    h = torch.as_tensor(hist, dtype=torch.int64).reshape(-1).to(v.device)
    if v.numel() != 8:
        raise ValueError("stats_vec must hold 8 values (sf_episode_stats)")
    m = torch.cat([v, h])
    if dist.is_available() and dist.is_initialized() and (dist.get_world_size(group) > 1 or force):
        rows = [torch.empty_like(m) for _ in range(dist.get_world_size(group))]
        dist.all_gather(rows, m.contiguous(), group=group)
        m = torch.stack(rows)
        m = torch.cat([m[:, :6].sum(0), m[:, 6:7].min(0).values, m[:, 7:8].max(0).values, m[:, 8:].sum(0)])
    return m[:8].clone(), m[8:].clone()


def summarize(v, hist=None, hist_lo=0):
    """Dict of the quantities the trainer logs (rl/train.py:158-170) from a (reduced) vector; with the (reduced) histogram of an
    episode log also `median_return` (lower median over the histogram's episodes) and `saturated_returns`."""
    v = [int(x) for x in torch.as_tensor(v).tolist()]
    n = v[EPISODES]
    out = {"episodes": n, "fortress_kills": v[FORT_KILLS], "ship_deaths": v[SHIP_DEATHS], "shots": v[SHOTS]}
    if n > 0:
        mean = v[SUM_RETURN] / n
        var = max(0.0, v[SUM_SQ_RETURN] / n - mean * mean)
        out.update(mean_return=mean, std_return=math.sqrt(var), min_return=v[MIN_RETURN], max_return=v[MAX_RETURN])
    if hist is not None:
        med = quantile_from_histogram(hist, hist_lo, 0.5)
        if med is not None:
            out.update(median_return=med[0], saturated_returns=med[1])
    return out
