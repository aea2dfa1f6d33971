"""The reference the trainer kernels are held to (tests/trainerref.py), on the CPU: oracle/trainer_np.py against the
reference's own expressions evaluated by torch on CPU tensors, bit for bit, for every kind of input and every
(gamma, tau) pair the GPU tests use; that the case tables cover what they say; and that the inputs tell a reference with
a seeded fault (gamma * tau rounded factor by factor, multiply-adds contracted, uint8 actions sign-extended) from the
right one.  No GPU."""
import numpy as np
import pytest

import trainerref as R

torch = pytest.importorskip("torch")

T_MODEL, N_MODEL = 37, 1000


@pytest.mark.parametrize("gae", [True, False], ids=["gae", "plain"])
@pytest.mark.parametrize("pair", range(len(R.GAMMA_TAU)), ids=["%.4g-%.4g" % p for p in R.GAMMA_TAU])
@pytest.mark.parametrize("kind", R.KINDS)
def test_compute_returns_numpy_equals_torch(kind, pair, gae):
    gamma, tau = R.GAMMA_TAU[pair]
    rewards, vp, masks, nv = R.gen_returns_case(kind, T_MODEL, N_MODEL)
    ret, vp_out = R.compute_returns(rewards, vp, masks, nv, gae, gamma, tau)
    t_ret, t_vp = R.torch_compute_returns(rewards, vp, masks, nv, gae, gamma, tau)
    R.assert_bits_equal(ret, t_ret, "returns")  # (row T with GAE: neither writes it, both start from zeros)
    R.assert_bits_equal(vp_out, t_vp, "value_preds")
    if gae:
        R.assert_bits_equal(vp_out[-1], nv, "value_preds[T]")
        R.assert_bits_equal(vp_out[:-1], vp[:-1], "value_preds[:T]")
    else:
        R.assert_bits_equal(vp_out, vp, "value_preds")
        R.assert_bits_equal(ret[-1], nv, "returns[T]")


@pytest.mark.parametrize("rkind", R.REWARD_KINDS)
def test_record_step_numpy_equals_torch(rkind):
    n = N_MODEL
    ep, fin = R.gen_accumulators(rkind, n)
    if rkind not in ("f32-huge", "f32-overflow"):  # (those are far above 2^24: whole numbers with full mantissas, sums round)
        # (the special kind keeps its 1 % of inf, 0 and 3e38 in the accumulators too)
        assert (ep != np.round(ep)).mean() > 0.98 and (fin != np.round(fin)).mean() > 0.98, "the accumulators must not start from integers"
    t_ep, t_fin = ep.copy(), fin.copy()
    seen = set()
    for step in range(50):
        r, d = R.gen_step_rewards(rkind, n, step), R.gen_done(n, step)
        a = R.gen_actions(R.ACT_DTYPES[step % 3], n, step)
        seen |= set(np.unique(d).tolist())
        rf, m, ep, fin, act = R.record_step(r, d, ep, fin, a)
        t_rf, t_m, t_ep, t_fin, t_act = R.torch_record_step(r, d, t_ep, t_fin, a)
        for x, y, what in ((rf, t_rf, "reward"), (m, t_m, "masks"), (ep, t_ep, "episode_rewards"), (fin, t_fin, "final_rewards")):
            R.assert_bits_equal(x, y, "%s, step %d" % (what, step))
        assert act.dtype == np.int64 and np.array_equal(act, t_act), step
        assert np.array_equal(m == 0, d != 0)
    assert seen == {0, 1, 2, 255}


def test_record_step_optional_follows_the_abi():
    n = 300
    r, d = R.gen_step_rewards("f32-normal", n, 0), R.gen_done(n, 0)
    ep0, fin0 = R.gen_accumulators("f32-normal", n)
    full = R.record_step(r, d, ep0, fin0)
    _, _, ep, fin, _ = R.record_step_optional(r, d, None, fin0)
    assert ep is None and fin is fin0
    _, _, ep, fin, _ = R.record_step_optional(r, d, ep0, None)
    assert fin is None
    R.assert_bits_equal(ep, full[2])
    _, _, ep, fin, _ = R.record_step_optional(r, d, ep0, fin0)
    R.assert_bits_equal(ep, full[2])
    R.assert_bits_equal(fin, full[3])


def test_case_tables_cover_what_they_say():
    for ns in (R.RETURNS_NS, R.RECORD_NS):
        for edge in (64, 256, 65536):
            assert any(n < edge for n in ns) and any(n > edge for n in ns) and (edge in ns or edge == 65536), (ns, edge)
        assert 1 in ns and 255 in ns and 257 in ns and 65537 in ns
    assert 1 in R.RETURNS_TS and max(R.RETURNS_TS) == 128
    assert all(n in R.RETURNS_NS and T in R.RETURNS_TS for n, T in R.RETURNS_OTHER_SHAPES)
    assert any(n % 256 and n > 256 for n, _ in R.RETURNS_OTHER_SHAPES) and any(n > 65536 for n, _ in R.RETURNS_OTHER_SHAPES)
    assert 65537 * 129 * 4 * 4 + 65537 * 128 * 4 < 170e6  # the largest returns case: five arrays, 34 MB each at the most
    # (gamma, tau): the issue's seven pairs, and at least two that tell the roundings apart
    for p in ((0.99, 0.95), (0.995, 0.9), (1 / 3, 2 / 3), (0.1, 0.7), (1, 1), (0, 0.3), (0.995, 0)):
        assert p in R.GAMMA_TAU
    assert len(R.SEPARATING) >= 2 and R.RETURNS_FULL[1] in R.SEPARATING and R.RETURNS_FULL[0] in R.KINDS
    assert set(R.search_gamma_tau()) >= set(R.GAMMA_TAU[-2:])
    # every kind is there and is what it says
    assert set(R.KINDS) >= {"normal", "engine", "subnormal", "huge", "special", "masks-as-data"}
    assert {k[4:] for k in R.REWARD_KINDS if k.startswith("f32-")} == set(R.KINDS) and {"i32-engine", "i32-full"} <= set(R.REWARD_KINDS)
    tiny = np.finfo(np.float32).tiny
    for kind in R.KINDS:
        rewards, vp, masks, nv = R.gen_returns_case(kind, T_MODEL, N_MODEL)
        assert rewards.dtype == vp.dtype == masks.dtype == nv.dtype == np.float32
        assert rewards.shape == (T_MODEL, N_MODEL) and vp.shape == masks.shape == (T_MODEL + 1, N_MODEL) and nv.shape == (N_MODEL,)
        if kind == "masks-as-data":
            assert set(np.unique(masks).tolist()) == {0.0, 0.5, 1.0} and (np.signbit(masks) & (masks == 0)).any()
        elif kind == "masks-uniform":
            assert ((masks >= 0) & (masks < 1)).all() and len(np.unique(masks)) > 1000
        else:
            assert set(np.unique(masks).tolist()) == {0.0, 1.0} and 0.05 < (masks == 0).mean() < 0.09
        ret, _ = R.compute_returns(rewards, vp, masks, nv, True, 0.99, 0.95)
        if kind == "engine":
            assert set(np.unique(rewards).tolist()) == {-1, 0, 1, 2, 3}
        if kind == "subnormal":
            assert (np.abs(rewards) < tiny).all() and (rewards != 0).mean() > 0.99
            assert ((np.abs(ret[:-1]) < tiny) & (ret[:-1] != 0)).mean() > 0.9, "the results must be subnormals too"
        if kind == "huge":
            assert np.isfinite(rewards).all() and 1e36 < np.abs(rewards).mean(dtype=np.float64) < 1e37
        if kind == "overflow":
            assert np.isinf(ret[:-1]).any() and np.isinf(rewards).any() and np.isinf(rewards).mean() < 0.01
        if kind == "special":
            bits = set(rewards.view(np.uint32)[~np.isnan(rewards)].tolist())
            for v in (np.inf, -np.inf, 0.0, -0.0, 1e-45, 3e38):
                assert int(np.float32(v).view(np.uint32)) in bits, v
            assert 0.001 < np.isnan(rewards).mean() < 0.005
    # bookkeeping inputs
    for n in (1, 257):
        assert (R.gen_step_rewards("i32-engine", n, 0) <= 3).all() and (R.gen_step_rewards("i32-engine", n, 0) >= -1).all()
    full = np.concatenate([R.gen_step_rewards("i32-full", 257, s) for s in range(R.RECORD_STEPS)])
    assert full.dtype == np.int32 and full.min() == -2 ** 31 and full.max() == 2 ** 31 - 1
    assert (full.astype(np.float32).astype(np.float64) != full).mean() > 0.9, "most of them must round on the way to float32"
    u8, i32, i64 = (np.concatenate([R.gen_actions(dt, 257, s) for s in range(R.RECORD_STEPS)]) for dt in R.ACT_DTYPES)
    assert u8.dtype == np.uint8 and (u8 >= 128).any() and 255 in u8 and 128 in u8
    assert i32.dtype == np.int32 and (i32 < 0).any() and -2 ** 31 in i32
    assert i64.dtype == np.int64 and (np.abs(i64.astype(np.float64)) > 2.0 ** 32).any() and 2 ** 32 + 5 in i64
    # the epilogue's cases
    cases = R.epilogue_cases()
    assert {c[0] for c in cases} == set(R.EPILOGUE_NS) and R.EPILOGUE_NS[-4:] == (8192, 24576, 49152, 90112)
    for n in R.EPILOGUE_NS:
        mine = [c for c in cases if c[0] == n and c[2] != "image"]
        if n >= 49152:
            assert [c[1:4] for c in mine] == [("youturn", "features", False)]
        else:
            assert {c[1:4] for c in mine} == set(R.EPILOGUE_CONFIGS) and {c[4] for c in mine} == set(R.ACT_DTYPES), n
    for cfg in R.EPILOGUE_CONFIGS:
        assert {c[4] for c in cases if c[1:4] == cfg} == set(R.ACT_DTYPES), cfg
    assert {c[0] for c in cases if c[2] == "image"} == {64, 257}
    assert {g for g, _, _ in R.EPILOGUE_CONFIGS} == {"youturn", "autoturn"}
    assert {(o, f) for _, o, f in R.EPILOGUE_CONFIGS} == {("features", False), ("features", True), ("normalized-features", False)}


def test_bits_equal_and_guards_notice():
    a = np.array([0.0, 1.0, np.nan, 1e-45], np.float32)
    R.assert_bits_equal(a, a.copy())
    b = a.copy()
    b.view(np.uint32)[2] |= 1  # another NaN payload: not compared
    R.assert_bits_equal(a, b)
    for i, v in ((0, -0.0), (3, 0.0), (1, np.nan), (2, 1.0)):
        b = a.copy()
        b[i] = v
        with pytest.raises(AssertionError):
            R.assert_bits_equal(a, b)
    for dt in (torch.float32, torch.uint8, torch.int32, torch.int64, torch.float64):
        v = R.guarded((3, 5), dt, "cpu")
        assert v.shape == (3, 5) and v.is_contiguous() and v.data_ptr() % 16 == 0 and R.untouched(v)
        assert v._base.numel() == 15 + 2 * R.GUARD
        R.margins_intact(v)
        v.fill_(1)
        assert not R.untouched(v)
        R.margins_intact(v)
        for off in (R.GUARD - 1, R.GUARD + 15):
            keep = v._base[off].clone()
            v._base[off] = 0
            with pytest.raises(AssertionError):
                R.margins_intact(v)
            v._base[off] = keep
        R.refill(v)
        assert R.untouched(v)
    v = R.guarded(4, torch.float32, "cpu", np.arange(4, dtype=np.float32))
    assert v.tolist() == [0, 1, 2, 3]


# ---------------------------------------------------------------------------------------------------------------
# seeded faults: the GPU tests' own inputs (kind, pair, shape) must tell a faulty evaluation from the right one
@pytest.mark.parametrize("n,T", R.RETURNS_OTHER_SHAPES)
def test_inputs_catch_gamma_tau_rounded_by_factor(n, T):
    kind = R.RETURNS_FULL[0]
    rewards, vp, masks, nv = R.gen_returns_case(kind, T, n)
    for gamma, tau in R.GAMMA_TAU:
        want, _ = R.compute_returns(rewards, vp, masks, nv, True, gamma, tau)
        got, _ = R.compute_returns_faulty(rewards, vp, masks, nv, True, gamma, tau, split_rounding=True)
        if (gamma, tau) in R.SEPARATING:
            with pytest.raises(AssertionError):
                R.assert_bits_equal(got, want)
        else:
            R.assert_bits_equal(got, want)
        # plain returns do not use tau
        want, _ = R.compute_returns(rewards, vp, masks, nv, False, gamma, tau)
        got, _ = R.compute_returns_faulty(rewards, vp, masks, nv, False, gamma, tau, split_rounding=True)
        R.assert_bits_equal(got, want)


@pytest.mark.parametrize("n,T", R.RETURNS_OTHER_SHAPES)
def test_inputs_catch_contracted_multiply_adds(n, T):
    """GAE: `delta + (gamma tau mask) * gae` rounds twice, and 0 / 1 masks are enough to see it.  Plain returns: the
    product with the mask is the only one in front of an addition, and it is exact for masks of 0, 1, 0.5 and -0.0 -- the
    masks-uniform kind is there for that."""
    gamma, tau = R.RETURNS_FULL[1]
    for kind, gae, shows in (("normal", True, True), ("masks-uniform", True, True), ("masks-uniform", False, True),
                             ("normal", False, False), ("masks-as-data", False, False)):
        rewards, vp, masks, nv = R.gen_returns_case(kind, T, n)
        want, _ = R.compute_returns(rewards, vp, masks, nv, gae, gamma, tau)
        got, _ = R.compute_returns_faulty(rewards, vp, masks, nv, gae, gamma, tau, contract=True)
        if shows:
            with pytest.raises(AssertionError):
                R.assert_bits_equal(got, want)
        else:
            R.assert_bits_equal(got, want)
    # without a fault the faulty evaluation is the reference
    got, _ = R.compute_returns_faulty(rewards, vp, masks, nv, True, gamma, tau)
    R.assert_bits_equal(got, R.compute_returns(rewards, vp, masks, nv, True, gamma, tau)[0])


def test_inputs_catch_sign_extended_uint8_actions():
    a = R.gen_actions(np.uint8, R.NULL_N, 0)
    want = R.record_step(R.gen_step_rewards("i32-engine", R.NULL_N, 0), R.gen_done(R.NULL_N, 0), *R.gen_accumulators("i32-engine", R.NULL_N), a)[4]
    assert (want >= 0).all() and not np.array_equal(want, a.astype(np.int8).astype(np.int64))
    a = R.gen_actions(np.int32, R.NULL_N, 1)
    assert not np.array_equal(a.astype(np.int64), a.astype(np.uint32).astype(np.int64))  # (and zero-extended int32)
