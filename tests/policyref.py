"""The numpy model of the policy head: include/sfmi_policy.h restated, operation by operation.  No GPU, no torch.

float32 where the header says float32 and float64 where it says float64; the two transcendental calls (expf, logf) are
numpy's float64 ones rounded to float32, i.e. correctly rounded up to a double rounding -- the device's differ from them by
their documented ulp bounds, which is what the tests' bounds are derived from (profiles/policy_head.md).

policy_head(...) also returns, per row, the EDGE DISTANCE min_k |t - c[k]| / S: how far, as a share of the whole mass, the draw
landed from the nearest boundary between two actions.  A device whose e[k] differ by an ulp can play a neighbour only on rows
whose edge distance is below the margin derived there.
"""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
COUNTER_WORD = 0x504F4C  # the third counter word of the head's stream (sf_step_sampled's is 0)


def philox4x32_10(c, k):
    """Vectorised Philox4x32-10 on all four counter words: c = 4 uint32 arrays (or scalars), k = 2 key words; the 4 output
    words (the restatement of tests/test_gpu_sampled.py, which only ever passes zeros in words 2 and 3)."""
    c = [np.asarray(x, np.uint64) for x in np.broadcast_arrays(*[np.asarray(x, np.uint64) for x in c])]
    k = [np.uint64(int(k[0]) & 0xFFFFFFFF), np.uint64(int(k[1]) & 0xFFFFFFFF)]
    m32 = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & m32, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & m32]
        k = [(k[0] + np.uint64(W0)) & m32, (k[1] + np.uint64(W1)) & m32]
    return [x.astype(np.uint32) for x in c]


def draw_words(seed, first_lane, n, ticks):
    """w of every env: ticks = one tick for all, or uint32 [ceil(n / 64)] (env i reads ticks[i // 64])."""
    lanes = (np.arange(n, dtype=np.uint64) + np.uint64(first_lane)) & np.uint64(0xFFFFFFFF)
    t = np.asarray(ticks, np.uint64)
    if t.ndim:
        t = t[np.arange(n) // 64]
    return philox4x32_10((lanes, t, np.uint64(COUNTER_WORD), np.uint64(0)), (seed & 0xFFFFFFFF, seed >> 32))[0]


def bad_rows(x):
    """A NaN, a +inf, or nothing but -inf."""
    x = np.asarray(x, np.float32)
    return np.isnan(x).any(1) | (x == np.inf).any(1) | (x == -np.inf).all(1)


def policy_head(logits, mode=0, seed=0, first_lane=0, ticks=0, words=None):
    """logits float32 [n, A] -> dict(action int64 [n], logp float32 [n], entropy float32 [n], bad bool [n], edge float64 [n],
    t, c [n, A], S, e [n, A], m).  mode 0 samples with `words` (uint32 [n]) or the stream's (seed, first_lane, ticks);
    mode 1 takes the first maximum (edge is inf there)."""
    x = np.ascontiguousarray(logits, np.float32)
    n, A = x.shape
    bad = bad_rows(x)
    xs = np.where(bad[:, None], np.float32(0), x)  # (a bad row's arithmetic is not looked at)
    with np.errstate(all="ignore"):
        m = xs.max(1)                                                    # 1.
        d = (xs - m[:, None]).astype(np.float32)                         # x[k] - m, float32 (-inf stays -inf)
        e = np.exp(d.astype(np.float64)).astype(np.float32)              # 2. expf: exactly 0 at -inf
        c = np.zeros((n, A), np.float64)                                 # 3. float64 running sum, index order
        run = np.zeros(n, np.float64)
        dot = np.zeros(n, np.float32)
        for k in range(A):
            run = run + e[:, k].astype(np.float64)
            c[:, k] = run
            term = (e[:, k] * d[:, k]).astype(np.float32)
            dot = np.where(e[:, k] != 0, (dot + term).astype(np.float32), dot)
        S = c[:, -1]
        if mode == 0:
            w = draw_words(seed, first_lane, n, ticks) if words is None else np.asarray(words, np.uint32)
            t = ((w.astype(np.float64) + 0.5) * 2.0 ** -32) * S
            a = (c <= t[:, None]).sum(1)                                 # the smallest k with t < c[k]
            assert (a[~bad] < A).all()
            edge = np.abs(t[:, None] - c).min(1) / S
        else:
            t = np.full(n, np.nan)
            a = xs.argmax(1)                                             # the first index of the maximum
            edge = np.full(n, np.inf)
        a = np.where(bad, 0, np.minimum(a, A - 1)).astype(np.int64)
        Sf = S.astype(np.float32)
        lse = np.log(Sf.astype(np.float64)).astype(np.float32)           # logf((float)S)
        xa = np.take_along_axis(xs, a[:, None], 1)[:, 0]
        logp = ((xa - m).astype(np.float32) - lse).astype(np.float32)
        ent = (lse - (dot / Sf).astype(np.float32)).astype(np.float32)
    nan = np.float32(np.nan)
    return dict(action=a, logp=np.where(bad, nan, logp), entropy=np.where(bad, nan, ent), bad=bad,
                edge=np.where(bad, np.inf, edge), t=t, c=c, S=S, e=e, m=m, lse=lse, x=xs,
                xa_minus_m=np.abs((xa - m).astype(np.float32)))


def logp_of(out, actions):
    """The model's log-probability of OTHER actions than its own (a device that played a neighbour on an edge row)."""
    a = np.asarray(actions, np.int64)
    with np.errstate(all="ignore"):
        d = (np.take_along_axis(out["x"], a[:, None], 1)[:, 0] - out["m"]).astype(np.float32)
        return np.where(out["bad"], np.float32(np.nan), (d - out["lse"]).astype(np.float32)), np.abs(d)


# ---------------------------------------------------------------------------------------------------------------
# the bounds of profiles/policy_head.md, as the tests use them (formulas of the shape, never measured maxima)
def edge_margin(A):
    """A row is OFF THE EDGE when its edge distance exceeds this: (A + 4) * 2^-22."""
    return (A + 4) * 2.0 ** -22


def logp_bound(A, xa_minus_m):
    return (A + 8) * 2.0 ** -23 + np.asarray(xa_minus_m, np.float64) * 2.0 ** -23


def entropy_bound(A):
    """(A + 8) * (1 + ln A) * 2^-23: the logf(S) part as in logp_bound, the quotient's part ln A times as much."""
    return (A + 8) * (1.0 + np.log(A)) * 2.0 ** -23


def general_rows(n, A, scale, seed):
    """The GPU tests' general rows: normal * scale, a random quarter of the entries -inf, never a whole row."""
    r = np.random.default_rng([seed, n, A, int(scale * 10)])
    x = (r.standard_normal((n, A)) * scale).astype(np.float32)
    mask = r.random((n, A)) < 0.25
    mask[np.arange(n), r.integers(0, A, n)] = False
    x[mask] = -np.inf
    return x


def adjacent_nonzero(c, a):
    """For each row: the set {a, next action below a of non-zero probability, next one above} as two arrays (lo, hi); -1 where
    there is none.  Non-zero probability of k: c[k] > c[k-1]."""
    n, A = c.shape
    nz = np.diff(np.concatenate([np.zeros((n, 1)), c], 1), axis=1) > 0
    lo, hi = np.full(n, -1), np.full(n, -1)
    for i in range(n):
        below = np.nonzero(nz[i, :a[i]])[0]
        above = np.nonzero(nz[i, a[i] + 1:])[0]
        lo[i] = below[-1] if below.size else -1
        hi[i] = a[i] + 1 + above[0] if above.size else -1
    return lo, hi
