"""numpy model of include/sfmi_minibatch.h: sf_advantages with exactly rounded sums, sf_minibatch_gather in both modes with its
out-of-range rules, and the bounds that hold the device's float64 statistics to the exact ones (profiles/minibatch.md)."""
import math

import numpy as np

f32 = np.float32
U64 = 2.0 ** -53  # float64's unit roundoff
BLOCK = 256       # elements per block of the fixed sum (sf_fixed_sum.h)

ADV_MS = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 4097, 65537, 327680)
GATHER_MBS = (1, 63, 64, 65, 257, 4096)
ROW_BYTES = (4, 8, 12, 16, 20, 60, 96, 1024, 1028)


# ------------------------------------------------------------------------------------------------------------ advantages
def advantages_apply(raw, mean, std, eps=1e-5):
    """The header's last line in float32 from given statistics: (raw - (float)mean) / ((float)std + (float)eps)."""
    with np.errstate(all="ignore"):
        return ((raw.astype(f32) - f32(mean)) / (f32(std) + f32(eps))).astype(f32)


def advantages_ref(ret, val, eps=1e-5):
    """-> (raw float32 [M], mean, std, out float32 [M]); the two sums exactly rounded (math.fsum), everything else as the header
    has it.  A NaN or an inf anywhere makes mean, std and every output NaN, as IEEE arithmetic does in any order."""
    with np.errstate(all="ignore"):
        raw = (np.asarray(ret, f32).reshape(-1) - np.asarray(val, f32).reshape(-1)).astype(f32)
    M = raw.size
    if not np.isfinite(raw).all():
        nan = float("nan")
        return raw, nan, nan, np.full(M, np.nan, f32)
    x = raw.astype(np.float64)
    mean = math.fsum(x.tolist()) / M
    S2 = math.fsum(((x - mean) ** 2).tolist())
    with np.errstate(all="ignore"):
        std = float(np.sqrt(np.float64(S2) / np.float64(M - 1)))
    return raw, mean, std, advantages_apply(raw, mean, std, eps)


def sum_depth(M):
    """The most float64 additions any one element goes through in the fixed order: 6 in the wave's tree, 3 among the block's
    four waves, one per block in front of and behind it in the chain of blocks."""
    return 6 + 3 + (M + BLOCK - 1) // BLOCK


def stats_bounds(raw):
    """(bound on |mean_dev - mean|, bound on |std_dev - std|) for finite float32 `raw`, from the kernel's float64 operation count
    (profiles/minibatch.md has the derivation):
      mean: a sum of depth d carries at most d u sum|raw| (first order), the division one more rounding; the reference's
            fsum and its division one each: (d + 3) u sum|raw| / M.
      std:  each term ((double)raw - mean)^2 carries 3 u (the subtraction once, squared; the product), the sum d u, the
            division by M - 1 one u; a mean off by dm moves S2 by at most M dm^2; the square root halves the relative error and
            adds its own (the device's sqrt: 1 ulp = 2 u).  The reference's own roundings -- its terms 3 u, fsum, the
            division, numpy's square root, one u each -- are counted too, and its mean is a rounded one: hence the cross
            term 2 dm sum|raw - mean|.
    Second-order terms are covered by the factor 1 + 1e-6."""
    x = np.asarray(raw, np.float64)
    M = x.size
    d = sum_depth(M)
    A = math.fsum(np.abs(x).tolist())
    bm = (d + 3) * U64 * A / M * (1 + 1e-6)
    if M < 2:
        return bm, 0.0
    mean = math.fsum(x.tolist()) / M
    S2 = math.fsum(((x - mean) ** 2).tolist())
    if S2 == 0.0:
        # every element equals the mean: the device's mean may be off by bm, and then S2 <= M bm^2
        return bm, math.sqrt(M * bm * bm / (M - 1)) * (1 + 1e-6)
    rel_S2 = (d + 3 + 1) * U64 + 5 * U64 + (M * bm * bm + 2 * bm * math.fsum(np.abs(x - mean).tolist())) / S2
    std = math.sqrt(S2 / (M - 1))
    return bm, std * (0.5 * rel_S2 + 3 * U64) * (1 + 1e-6)


# ---------------------------------------------------------------------------------------------------------------- gather
def gather_rows(index, n_index, n_rows_src, mb, c, n_batches, traj_T=0, traj_n=0):
    """-> g int64 [mb]: the source row of every output row, -1 for a bad one (sfmi_minibatch.h)."""
    index = np.asarray(index)
    g = np.full(mb, -1, np.int64)
    if c >= n_batches:
        return g
    for r in range(mb):
        if traj_T > 0:
            j, t = c * (mb // traj_T) + r // traj_T, r % traj_T
        else:
            j, t = c * mb + r, 0
        if j >= n_index:
            continue
        cand = t * int(traj_n) + int(index[j])
        if 0 <= cand < n_rows_src:
            g[r] = cand
    return g


def gather_ref(columns, index, n_index, mb, c, n_batches, traj_T=0, traj_n=0):
    """columns: arrays [n_rows_src, ...] -> ([mb, ...] per column, idx_out int64 [mb], the number of bad rows).  A bad row is
    zeros in every column."""
    n_rows_src = columns[0].shape[0]
    g = gather_rows(index, n_index, n_rows_src, mb, c, n_batches, traj_T, traj_n)
    ok = g >= 0
    outs = []
    for col in columns:
        assert col.shape[0] == n_rows_src
        out = np.zeros((mb,) + col.shape[1:], col.dtype)
        out[ok] = col[g[ok]]
        outs.append(out)
    return outs, g, int((~ok).sum())


def sampler_slices(total, num_mini_batch):
    """BatchSampler(SubsetRandomSampler(range(total)), total // num_mini_batch, drop_last=False): (start, length) of every
    minibatch, the short last one included."""
    mb = total // num_mini_batch
    return [(s, min(mb, total - s)) for s in range(0, total, mb)]
