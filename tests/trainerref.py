"""TEST INFRASTRUCTURE ONLY -- what the tests of the trainer kernels share (sf_rollout_ops.hip: sf_record_step,
sf_record_step_f32, sf_compute_returns; the step kernel's bookkeeping epilogue, sf_step_record):

  * the reference: oracle/trainer_np.py (pinned to the reference's own code by tests/golden/trainer/), wrapped so that it
    takes float32 rewards, widens actions the way numpy does and follows the C ABI's optional outputs;
  * a second, independent evaluation: the reference's expressions written with torch CPU tensors and Python scalars, so
    that what a Python float or int becomes when it meets a float32 tensor is torch's own business and not restated;
  * seeded input generators, the (gamma, tau) table, the case tables of the GPU tests;
  * assert_bits_equal and guarded buffers.

test_trainer_ref_model.py shows on the CPU that the two evaluations agree bit for bit on every kind of input and every
(gamma, tau) pair, and that the inputs tell a reference with a seeded fault from the right one.
"""
import numpy as np

from oracle import trainer_np as TN

f32 = np.float32

# ---------------------------------------------------------------------------------------------------------------
# (gamma, tau).  The kernel gets (float)(gamma * tau): a double product rounded once, which is what torch makes of
# `gamma * tau * tensor`.  A kernel that rounded the factors first would compute float32(gamma) * float32(tau).
GAMMA_TAU = ((0.99, 0.95), (0.995, 0.9), (1 / 3, 2 / 3), (0.1, 0.7), (1.0, 1.0), (0.0, 0.3), (0.995, 0.0),
             (0.99, 0.92), (0.98, 0.94))  # the last two found by search_gamma_tau(): of the others only (1/3, 2/3) separates


def roundings_differ(gamma, tau):
    return f32(gamma * tau) != f32(gamma) * f32(tau)


def search_gamma_tau(limit=6):
    """Two-digit pairs a trainer might use whose two roundings differ, in order: (0.99, 0.99), (0.99, 0.92), (0.98, 0.98),
    (0.98, 0.94), ... -- about a quarter of all pairs (how the table's last two were found)."""
    out = []
    for g in range(99, 89, -1):
        for t in range(99, 89, -1):
            if roundings_differ(g / 100, t / 100):
                out.append((g / 100, t / 100))
                if len(out) == limit:
                    return out
    return out


SEPARATING = tuple(p for p in GAMMA_TAU if roundings_differ(*p))
assert len(SEPARATING) >= 2, "the (gamma, tau) table must tell the two roundings of gamma * tau apart"
assert (1 / 3, 2 / 3) in SEPARATING

# ---------------------------------------------------------------------------------------------------------------
# inputs, fixed seeds
KINDS = ("normal", "engine", "subnormal", "huge", "special", "masks-as-data", "overflow", "masks-uniform")
# normal         unit normals
# engine         integers in [-1, 3]: what the game hands the trainer
# subnormal      normals times 1e-39: every value and most intermediate results are float32 subnormals
# huge           normals times 1e37
# special        normals, about 1 % replaced from _SPECIAL
# masks-as-data  unit normals; masks drawn from {0, 1, 0.5, -0.0}
# overflow       normals times 1e38: a few become inf in float32, and sums of two overflow all the time (at 1e37 a sum would
#                have to be 20 deviations out)
# masks-uniform  unit normals; masks uniform in [0, 1): the products with a mask round, so a contracted multiply-add shows
#                in plain returns too (a product with 0, 1, 0.5 or -0.0 is exact)
# Masks of every other kind: 1 - done at a `done` rate of about 7 %.
_SPECIAL = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 1e-45, 3e38], f32)
_MASK_DATA = np.array([0.0, 1.0, 0.5, -0.0], f32)
DONE_RATE = 0.07
DONE_BYTES = np.array([0, 1, 2, 255], np.uint8)

SENTINEL_BYTE = 0xA5  # guard margins and unwritten outputs: every byte.  float32 -2.87e-16, int32 -1515870811
GUARD = 64            # elements in front of and behind a guarded buffer
_SENT32 = np.uint32(0xA5A5A5A5)


def _rng(kind, what, shape, seed):
    return np.random.default_rng([seed, KINDS.index(kind), what] + [int(s) for s in shape])


def _no_sentinel(x):
    assert not (np.ascontiguousarray(x).view(np.uint32) == _SENT32).any(), "a generator produced the sentinel's bit pattern"
    return x


def gen_values(kind, shape, seed=0, what=0):
    """float32 rewards / values of `kind`; `what` separates the arrays of one case."""
    rng = _rng(kind, what, shape, seed)
    if kind == "engine":
        return rng.integers(-1, 4, shape).astype(f32)
    x = rng.standard_normal(shape)
    if kind == "subnormal":
        x = x * 1e-39
    elif kind == "huge":
        x = x * 1e37
    elif kind == "overflow":
        x = x * 1e38
    with np.errstate(over="ignore"):
        x = x.astype(f32)
    if kind == "special":
        hit = rng.random(shape) < 0.01
        x[hit] = rng.choice(_SPECIAL, int(hit.sum()))
    return _no_sentinel(x)


def gen_masks(kind, shape, seed=0):
    rng = _rng(kind, 7, shape, seed)
    if kind == "masks-as-data":
        return rng.choice(_MASK_DATA, shape)
    if kind == "masks-uniform":
        return _no_sentinel(rng.random(shape).astype(f32))
    return np.where(rng.random(shape) < DONE_RATE, f32(0), f32(1)).astype(f32)


def gen_returns_case(kind, T, n, seed=0):
    """-> rewards [T][n], value_preds [T+1][n], masks [T+1][n], next_value [n]"""
    return (gen_values(kind, (T, n), seed, 0), gen_values(kind, (T + 1, n), seed, 1), gen_masks(kind, (T + 1, n), seed),
            gen_values(kind, (n,), seed, 2))


REWARD_KINDS = ("i32-engine", "i32-full") + tuple("f32-" + k for k in KINDS)
_I32_EDGES = np.array([-2 ** 31, 2 ** 31 - 1, 2 ** 24 + 1, -(2 ** 24) - 1, 2 ** 25 + 2, 2 ** 25 + 6, 2 ** 31 - 65, 2 ** 31 - 64, 0, -1],
                      np.int64)  # (float) must round to nearest, ties to even, as numpy's astype does


def gen_step_rewards(rkind, n, step, seed=0):
    """One step's rewards: int32 (`i32-engine`: [-1, 3]; `i32-full`: the whole range, with the values at which the
    conversion to float32 rounds) or float32 of a kind."""
    if rkind.startswith("f32-"):
        return gen_values(rkind[4:], (n,), seed, 100 + step)
    rng = np.random.default_rng([seed, 50 + REWARD_KINDS.index(rkind), n, step])
    if rkind == "i32-engine":
        return rng.integers(-1, 4, n).astype(np.int32)
    r = rng.integers(-2 ** 31, 2 ** 31, n)
    k = min(n, len(_I32_EDGES))
    r[rng.choice(n, k, replace=False)] = _I32_EDGES[:k]
    r[r == -1515870811] = 7
    return r.astype(np.int32)


def gen_done(n, step, seed=0):
    """`done` bytes from {0, 1, 2, 255}: seven in ten are 0, the rest spread over the three ways of saying yes"""
    rng = np.random.default_rng([seed, 60, n, step])
    return rng.choice(DONE_BYTES, n, p=[0.7, 0.1, 0.1, 0.1])


def gen_accumulators(rkind, n, seed=0):
    """episode_rewards, final_rewards to start from: never integers -- of the rewards' own kind where that is a float kind
    (so that subnormal accumulators meet subnormal rewards), otherwise normals of a few units."""
    kind = rkind[4:] if rkind.startswith("f32-") and rkind[4:] != "engine" else "normal"
    scale = f32(1) if kind in ("subnormal", "huge", "overflow") else f32(3.7)
    with np.errstate(over="ignore"):
        return gen_values(kind, (n,), seed, 200) * scale, gen_values(kind, (n,), seed, 201) * scale


ACT_DTYPES = (np.uint8, np.int32, np.int64)
_ACT_EDGES = {np.uint8: [0, 127, 128, 129, 200, 255], np.int32: [0, -1, -2 ** 31, 2 ** 31 - 1, 128, -128],
              np.int64: [0, -1, 2 ** 32, 2 ** 32 + 5, -(2 ** 40), -2 ** 63, 2 ** 63 - 1, 2 ** 31, -2 ** 31 - 1]}


def gen_actions(dtype, n, step, seed=0):
    """Anything the element type holds (sf_record_step copies, it does not play): uint8 up to 255, negative int32 with
    INT32_MIN, int64 beyond 2^32."""
    dtype = np.dtype(dtype).type
    rng = np.random.default_rng([seed, 70 + ACT_DTYPES.index(dtype), n, step])
    info = np.iinfo(dtype)
    a = rng.integers(info.min, info.max, n, dtype=dtype, endpoint=True)
    edges = np.array(_ACT_EDGES[dtype], dtype)
    k = min(n, len(edges))
    a[rng.choice(n, k, replace=False)] = rng.permutation(edges)[:k]
    if dtype is np.int64:
        a[a.view(np.uint64) == np.uint64(0xA5A5A5A5A5A5A5A5)] = 3
    return a


# ---------------------------------------------------------------------------------------------------------------
# the case tables of tests/test_gpu_trainer_kernels.py (here, so that the CPU suite can check what they cover)
RETURNS_NS = (1, 63, 64, 65, 255, 256, 257, 511, 513, 4097, 65537)
RETURNS_TS = (1, 2, 7, 128)
RETURNS_FULL = ("normal", (1 / 3, 2 / 3))        # the kind and pair of the full n x T cross product
RETURNS_OTHER_SHAPES = ((257, 7), (65537, 2))    # (n, T) of every other kind and pair: a partial last block, more than one
                                                 # block, more than 256 blocks
RECORD_NS = (1, 63, 64, 65, 255, 256, 257, 4097, 65537)
RECORD_STEPS = 12
NULL_N = 257
EPILOGUE_NS = (1, 63, 64, 65, 257, 1000, 4097, 8192, 24576, 49152, 90112)
EPILOGUE_STEPS = 40
EPILOGUE_CONFIGS = tuple((g, o, f64) for g in ("youturn", "autoturn")
                         for o, f64 in (("features", False), ("features", True), ("normalized-features", False)))


def epilogue_cases():
    """(n, gametype, obs_type, float64 observations, action dtype).  Every configuration at every size below 49 152, the
    two largest sizes with youturn features; the action type rotates so that every size and every configuration meets all
    three; an image batch at 64 and at 257 envs."""
    cases = []
    for i, n in enumerate(EPILOGUE_NS):
        if n >= 49152:
            cases.append((n, "youturn", "features", False, ACT_DTYPES[i % 3]))
            continue
        for j, (g, o, f64) in enumerate(EPILOGUE_CONFIGS):
            cases.append((n, g, o, f64, ACT_DTYPES[(i + j) % 3]))
    cases.append((64, "youturn", "image", False, np.int64))
    cases.append((257, "autoturn", "image", False, np.uint8))
    return cases


# ---------------------------------------------------------------------------------------------------------------
# the reference
def compute_returns(rewards, value_preds, masks, next_value, use_gae, gamma, tau):
    """oracle/trainer_np.compute_returns.  -> (returns [T+1][n], value_preds as the reference leaves them).  With use_gae
    the reference does not write returns[T]: that row comes back 0 here and is not part of any comparison."""
    with np.errstate(all="ignore"):
        return TN.compute_returns(rewards, value_preds, masks, next_value, use_gae, gamma, tau)


def record_step(reward, done, episode_rewards, final_rewards, actions=None):
    """oracle/trainer_np.record_step on int32 or float32 rewards and `done` bytes (anything but 0 is done); `actions`
    uint8 / int32 / int64 -> what rollouts.actions[step], a LongTensor, holds: numpy's widening.
    -> (reward float32, masks, episode_rewards, final_rewards, actions int64 or None)"""
    assert reward.dtype in (np.int32, np.float32) and done.dtype == np.uint8
    with np.errstate(all="ignore"):
        r, m, ep, fin = TN.record_step(reward, done, episode_rewards, final_rewards)
    return r, m, ep, fin, None if actions is None else actions.astype(np.int64)


def record_step_optional(reward, done, episode_rewards, final_rewards, actions=None):
    """record_step as the C ABI runs it when accumulators are missing (None): without episode_rewards nothing is
    accumulated and final_rewards stays as it is (sfmi.h); without final_rewards episode_rewards is kept all the same."""
    ep0 = episode_rewards if episode_rewards is not None else np.zeros(reward.shape, f32)
    fin0 = final_rewards if final_rewards is not None else np.zeros(reward.shape, f32)
    r, m, ep, fin, a = record_step(reward, done, ep0, fin0, actions)
    if episode_rewards is None:
        ep, fin = None, final_rewards
    elif final_rewards is None:
        fin = None
    return r, m, ep, fin, a


def _fma(a, b, c):
    """a * b + c rounded once (the product of two float32 is exact in float64; the one sum's rounding to float64 in
    front of the rounding to float32 does not matter to a seeded fault)"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(f32)


def compute_returns_faulty(rewards, value_preds, masks, next_value, use_gae, gamma, tau, split_rounding=False, contract=False):
    """trainer_np.compute_returns with a seeded fault, for test_trainer_ref_model.py to show that the inputs catch it:
    split_rounding  gamma * tau as float32(gamma) * float32(tau)
    contract        every a * b + c as one fused multiply-add (what the compiler makes of them without -ffp-contract=off)"""
    T = rewards.shape[0]
    vp = value_preds.astype(f32).copy()
    ret = np.zeros_like(vp)
    g = f32(gamma)
    gt = f32(gamma) * f32(tau) if split_rounding else f32(gamma * tau)
    mad = _fma if contract else (lambda a, b, c: a * b + c)
    with np.errstate(all="ignore"):
        if use_gae:
            vp[-1] = next_value
            gae = f32(0)
            for t in reversed(range(T)):
                delta = mad(g * vp[t + 1], masks[t + 1], rewards[t]) - vp[t]
                gae = mad(gt * masks[t + 1], gae, delta)
                ret[t] = gae + vp[t]
        else:
            ret[-1] = next_value
            for t in reversed(range(T)):
                ret[t] = mad(ret[t + 1] * g, masks[t + 1], rewards[t])
    return ret, vp


# ---------------------------------------------------------------------------------------------------------------
# the second evaluation: the reference's own expressions (quoted in sf_rollout_ops.hip) on torch CPU tensors
def torch_compute_returns(rewards, value_preds, masks, next_value, use_gae, gamma, tau):
    """numpy in, numpy out; gamma and tau stay Python floats and gae starts as the Python int 0."""
    import torch
    rewards, masks = torch.from_numpy(rewards.copy()), torch.from_numpy(masks.copy())
    value_preds, next_value = torch.from_numpy(value_preds.copy()), torch.from_numpy(next_value.copy())
    returns = torch.zeros_like(value_preds)
    if use_gae:
        value_preds[-1] = next_value
        gae = 0
        for step in reversed(range(rewards.size(0))):
            delta = rewards[step] + gamma * value_preds[step + 1] * masks[step + 1] - value_preds[step]
            gae = delta + gamma * tau * masks[step + 1] * gae
            returns[step] = gae + value_preds[step]
    else:
        returns[-1] = next_value
        for step in reversed(range(rewards.size(0))):
            returns[step] = returns[step + 1] * gamma * masks[step + 1] + rewards[step]
    return returns.numpy(), value_preds.numpy()


def torch_record_step(reward, done, episode_rewards, final_rewards, actions=None):
    """The trainer's five lines on [n, 1] torch CPU tensors; actions through a LongTensor's copy_."""
    import torch
    reward = torch.from_numpy(np.expand_dims(reward, 1).copy()).float()
    episode_rewards = torch.from_numpy(episode_rewards.copy()).unsqueeze(1)
    final_rewards = torch.from_numpy(final_rewards.copy()).unsqueeze(1)
    episode_rewards += reward
    masks = torch.FloatTensor([[0.0] if i else [1.0] for i in done.tolist()])
    final_rewards *= masks
    final_rewards += (1 - masks) * episode_rewards
    episode_rewards *= masks
    out = None
    if actions is not None:
        out = torch.zeros(actions.shape[0], dtype=torch.long)
        out.copy_(torch.from_numpy(actions.copy()))
        out = out.numpy()
    return reward[:, 0].numpy(), masks[:, 0].numpy(), episode_rewards[:, 0].numpy(), final_rewards[:, 0].numpy(), out


# ---------------------------------------------------------------------------------------------------------------
# comparisons and guarded buffers
def _np(x):
    return x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)


def assert_bits_equal(got, want, what=""):
    """float32 arrays: NaN in the same places, everywhere else the same 32 bits (-0.0 is not +0.0, subnormals count).  NaN
    payloads are not compared: x86 and the GPU may differ there."""
    g, w = np.ascontiguousarray(_np(got)), np.ascontiguousarray(_np(want))
    assert g.dtype == np.float32 and w.dtype == np.float32, (what, g.dtype, w.dtype)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    gn, wn = np.isnan(g), np.isnan(w)
    bad = (gn != wn) | (~gn & (g.view(np.uint32) != w.view(np.uint32)))
    if bad.any():
        i = tuple(int(k) for k in np.argwhere(bad)[0])
        raise AssertionError("%s: %d of %d differ, first at %s: got %r (0x%08x), want %r (0x%08x)"
                             % (what, int(bad.sum()), bad.size, i, g[i], int(g.view(np.uint32)[i]), w[i], int(w.view(np.uint32)[i])))


def guarded(shape, dtype, device, data=None):
    """A contiguous tensor of `shape` inside a larger allocation: GUARD elements in front and behind, every byte of the
    allocation SENTINEL_BYTE, then `data` (numpy) copied in if given.  margins_intact / untouched check it."""
    import torch
    shape = tuple(int(s) for s in (shape if hasattr(shape, "__len__") else (shape,)))
    numel = int(np.prod(shape))
    base = torch.empty(numel + 2 * GUARD, dtype=dtype, device=device)
    base.view(torch.uint8).fill_(SENTINEL_BYTE)
    v = base[GUARD:GUARD + numel].view(shape)
    if data is not None:
        v.copy_(torch.from_numpy(np.ascontiguousarray(data)).view(shape))
    return v


def refill(*views):
    import torch
    for v in views:
        v.view(torch.uint8).fill_(SENTINEL_BYTE)


def margins_intact(*views):
    """A lane i >= n that writes [t * n + i] lands in the next row, which the comparison of the values catches, or here."""
    import torch
    for k, v in enumerate(views):
        base = v._base
        assert base is not None and v.storage_offset() == GUARD and base.numel() == v.numel() + 2 * GUARD
        u, b = base.view(torch.uint8), GUARD * base.element_size()
        assert bool((u[:b] == SENTINEL_BYTE).all()), "buffer %d: the margin in front was written" % k
        assert bool((u[-b:] == SENTINEL_BYTE).all()), "buffer %d: the margin behind was written" % k


def untouched(*views):
    import torch
    return all(bool((v.view(torch.uint8) == SENTINEL_BYTE).all()) for v in views)
