"""The policy head on the device (include/sfmi_policy.h: sf_policy_sample; PolicyHead; DeviceRollout.step_logits), held to the
numpy model tests/policyref.py.

The device's expf and logf are not numpy's, so nothing here is compared bit for bit where they enter -- and nothing is compared
loosely where they do not.  profiles/policy_head.md derives the three bounds used (policyref.edge_margin / logp_bound /
entropy_bound) from float32's roundings and the ulp bounds of the device's two functions:
  * a row whose draw lies further than the margin from every boundary between two actions must play the model's action; a row
    nearer to one plays the model's action or the adjacent one of non-zero probability, and at most 0.5 % of a case's rows are
    that near (tests/test_policy_model.py checks that of the model, for the seeds below);
  * log-probability (of the action the device played) and entropy lie within their bounds of the model's;
  * the exact cases -- all logits equal, one finite logit, argmax with ties -- and everything about ticks, shards, bad rows,
    refusals, graphs and rollouts are exact.
Every output of a raw call lives in a guarded buffer (trainerref.guarded) whose margins must stay untouched.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import policyref as PR
import trainerref as TR
from lockstep import sfa

SEED, FIRST_LANE = 0x0123456789ABCDEF, 4_000_000_000  # (first_lane + i wraps past 2^32 in the larger cases)
NS, AS, SCALES = (1, 63, 64, 65, 130, 4097), (1, 3, 5, 16, 32), (0.1, 1.0, 10.0)
# The seed of a case's rows is 1 unless the model's own edge count for it exceeds 0.5 % of the rows at one of the three ticks
# (a condition on the case, checked on the CPU by tests/test_policy_model.py): then the next seed that meets it.
ROW_SEEDS = {(65, 32, 0.1): 2}
# (n, A, scale, seed of the rows): every n x A x scale, and 65 537 envs once
GENERAL_CASES = [(n, A, s, ROW_SEEDS.get((n, A, s), 1)) for n in NS for A in AS for s in SCALES] + [(65537, 5, 1.0, 1)]
ACT_DTYPES = (torch.uint8, torch.int32, torch.int64)
ACT_TYPE = {torch.uint8: 1, torch.int32: 4, torch.int64: 8}


class Raw:
    """One raw sf_policy_sample call's buffers, all guarded: logits [n, stride] (sentinel padding behind every row), ticks,
    actions, logp, entropy, the bad-row counter."""

    def __init__(self, sfa, x, stride=None, act_dtype=torch.int64):
        from spacefortress_amd import _lib
        self.lib, self.L = _lib, _lib.lib()
        self.dev = torch.device("cuda", torch.cuda.current_device())
        self.n, self.A = x.shape
        self.stride = stride or self.A
        self.logits = TR.guarded((self.n, self.stride), torch.float32, self.dev)
        self.logits[:, :self.A].copy_(torch.from_numpy(x))
        self.ticks = TR.guarded((self.n + 63) // 64, torch.int32, self.dev, np.zeros((self.n + 63) // 64, np.int32))
        self.act = TR.guarded(self.n, act_dtype, self.dev)
        self.logp = TR.guarded(self.n, torch.float32, self.dev)
        self.ent = TR.guarded(self.n, torch.float32, self.dev)
        self.bad = TR.guarded(1, torch.int64, self.dev, np.zeros(1, np.int64))

    def call(self, mode=0, seed=SEED, first_lane=FIRST_LANE, **over):
        a = dict(logits=self.logits.data_ptr(), n=self.n, A=self.A, stride=self.stride, mode=mode, ticks=self.ticks.data_ptr(),
                 act=self.act.data_ptr(), at=ACT_TYPE[self.act.dtype], logp=self.logp.data_ptr(), ent=self.ent.data_ptr(),
                 bad=self.bad.data_ptr())
        a.update(over)
        vp = lambda p: C.c_void_p(p) if p else None
        return self.L.sf_policy_sample(vp(a["logits"]), a["n"], a["A"], a["stride"], a["mode"], seed, first_lane, vp(a["ticks"]),
                                       vp(a["act"]), a["at"], vp(a["logp"]), vp(a["ent"]), vp(a["bad"]),
                                       self.lib.raw_stream(self.dev))

    def host(self):
        torch.cuda.synchronize()
        TR.margins_intact(self.logits, self.ticks, self.act, self.logp, self.ent, self.bad)
        return (self.act.cpu().numpy().astype(np.int64), self.logp.cpu().numpy(), self.ent.cpu().numpy(),
                self.ticks.cpu().numpy().view(np.uint32), int(self.bad.item()))


def hold_to_model(x, got_a, got_logp, got_ent, model, what):
    """The general comparison: actions exact off the edge and adjacent on it, logp and entropy within their bounds."""
    n, A = x.shape
    a_m, near = model["action"], model["edge"] <= PR.edge_margin(A)
    assert near.sum() <= 0.005 * n, (what, "rows on the edge", int(near.sum()))
    assert (got_a >= 0).all() and (got_a < A).all(), what
    assert np.array_equal(got_a[~near], a_m[~near]), (what, "an action off the edge differs", int((got_a != a_m).sum()))
    if (got_a != a_m).any():
        lo, hi = PR.adjacent_nonzero(model["c"], a_m)
        other = got_a != a_m
        assert ((got_a[other] == lo[other]) | (got_a[other] == hi[other])).all(), (what, "an edge row played a far action")
    want_logp, dist = PR.logp_of(model, got_a)
    dl, de = np.abs(got_logp.astype(np.float64) - want_logp), np.abs(got_ent.astype(np.float64) - model["entropy"])
    bl, be = PR.logp_bound(A, dist), PR.entropy_bound(A)
    print("%s: edge rows %d, other action %d, logp err / bound max %.3f, entropy err / bound %.3f"
          % (what, near.sum(), (got_a != a_m).sum(), (dl / bl).max(), de.max() / be))
    assert np.isfinite(got_logp).all() and (dl <= bl).all(), (what, "logp", float(dl.max()))
    assert np.isfinite(got_ent).all() and (de <= be).all(), (what, "entropy", float(de.max()), be)


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("A", AS)
def test_general_rows_equal_the_model_at_three_successive_ticks(sfa, n, A):
    for j, scale in enumerate(SCALES):
        x = PR.general_rows(n, A, scale, ROW_SEEDS.get((n, A, scale), 1))
        raw = Raw(sfa, x, act_dtype=ACT_DTYPES[(j + A + n) % 3])
        for tick in range(3):
            assert raw.call() == 0
            a, logp, ent, ticks, bad = raw.host()
            assert (ticks == tick + 1).all() and bad == 0
            hold_to_model(x, a, logp, ent, PR.policy_head(x, seed=SEED, first_lane=FIRST_LANE, ticks=tick), (n, A, scale, tick))


@pytest.mark.gpu
def test_a_batch_beyond_two_to_the_sixteen(sfa):
    n, A, scale, seed = GENERAL_CASES[-1]
    x = PR.general_rows(n, A, scale, seed)
    raw = Raw(sfa, x, act_dtype=torch.uint8)
    assert raw.call() == 0
    a, logp, ent, ticks, bad = raw.host()
    assert (ticks == 1).all() and ticks.size == 1025 and bad == 0
    hold_to_model(x, a, logp, ent, PR.policy_head(x, seed=SEED, first_lane=FIRST_LANE, ticks=0), (n, A))


@pytest.mark.gpu
def test_a_row_stride_beyond_the_row_reads_no_padding(sfa):
    n, A = 130, 5
    x = PR.general_rows(n, A, 1.0, 2)
    raw, dense = Raw(sfa, x, stride=A + 3, act_dtype=torch.int32), Raw(sfa, x, act_dtype=torch.int32)
    assert raw.call() == 0 and dense.call() == 0
    got, want = raw.host(), dense.host()
    assert all(np.array_equal(g, w) for g, w in zip(got[:4], want[:4])) and got[4] == want[4] == 0
    assert TR.untouched(raw.logits[:, A:])  # (the sentinel is a small negative float: read as a logit it would change rows)
    hold_to_model(x, got[0], got[1], got[2], PR.policy_head(x, seed=SEED, first_lane=FIRST_LANE, ticks=0), "strided")


@pytest.mark.gpu
@pytest.mark.parametrize("A", AS)
def test_equal_logits_are_exact(sfa, A):
    for n, level, dt in ((130, 0.0, torch.uint8), (65, -3.25, torch.int32), (4097, 17.5, torch.int64)):
        x = np.full((n, A), level, np.float32)
        raw = Raw(sfa, x, act_dtype=dt)
        for tick in range(2):
            assert raw.call() == 0
            a, logp, ent, ticks, bad = raw.host()
            w = PR.draw_words(SEED, FIRST_LANE, n, tick).astype(np.uint64)
            assert np.array_equal(a, (((2 * w + 1) * np.uint64(A)) >> np.uint64(33)).astype(np.int64))  # floor((w + 0.5) A / 2^32)
            assert np.array_equal(a, PR.policy_head(x, seed=SEED, first_lane=FIRST_LANE, ticks=tick)["action"])
            # logp = -logf(A), entropy = logf(A): one value each, each other's negation, within the device logf's ulp of ln A
            assert np.unique(ent).size == 1 and np.array_equal(logp, -ent) and bad == 0
            want = np.float32(np.log(float(A)))
            assert ent[0] == 0 if A == 1 else abs(float(ent[0]) - float(want)) <= np.spacing(want)


@pytest.mark.gpu
@pytest.mark.parametrize("A", AS)
def test_one_finite_logit_is_always_played(sfa, A):
    n = 130
    r = np.random.default_rng(A)
    x = np.full((n, A), -np.inf, np.float32)
    k = r.integers(0, A, n)
    x[np.arange(n), k] = (r.standard_normal(n) * 30).astype(np.float32)
    raw = Raw(sfa, x, act_dtype=torch.uint8)
    assert raw.call() == 0
    a, logp, ent, ticks, bad = raw.host()
    assert np.array_equal(a, k) and (logp == 0).all() and (ent == 0).all() and bad == 0 and (ticks == 1).all()


@pytest.mark.gpu
@pytest.mark.parametrize("A", AS)
def test_argmax_takes_the_first_maximum_and_leaves_the_ticks(sfa, A):
    n = 130
    r = np.random.default_rng(100 + A)
    x = r.integers(-2, 3, (n, A)).astype(np.float32)  # small integers: ties in most rows
    x[r.random((n, A)) < 0.2] = -np.inf
    x[np.arange(n), r.integers(0, A, n)] = 2.0
    raw = Raw(sfa, x, act_dtype=ACT_DTYPES[A % 3])
    raw.ticks.fill_(7)
    assert raw.call(mode=1) == 0
    a, logp, ent, ticks, bad = raw.host()
    assert np.array_equal(a, x.argmax(1)) and (ticks == 7).all() and bad == 0
    model = PR.policy_head(x, mode=1)
    hold_to_model(x, a, logp, ent, model, ("argmax", A))
    # NULL ticks are fine here
    TR.refill(raw.act)
    assert raw.call(mode=1, ticks=0) == 0
    assert np.array_equal(raw.host()[0], a)


@pytest.mark.gpu
def test_ticks_count_calls_and_equal_seeds_draw_equal_actions(sfa):
    n, A = 4097, 5
    x = PR.general_rows(n, A, 1.0, 3)
    one, two = Raw(sfa, x, act_dtype=torch.uint8), Raw(sfa, x, act_dtype=torch.uint8)
    seen = []
    for j in range(1, 5):
        assert one.call() == 0 and two.call() == 0
        a1, a2 = one.host(), two.host()
        assert (a1[3] == j).all() and all(np.array_equal(p, q) for p, q in zip(a1[:4], a2[:4]))
        seen.append(a1[0])
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
    assert one.call(seed=SEED + 1) == 0  # another key: other draws at the same tick
    assert not np.array_equal(one.host()[0], PR.policy_head(x, seed=SEED, first_lane=FIRST_LANE, ticks=4)["action"])


def _logits(sfa, x):
    return torch.from_numpy(x).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 64, 100])
def test_shards_draw_what_the_whole_batch_draws(sfa, k):
    n, A = 130, 5
    x = PR.general_rows(n, A, 1.0, 4)
    whole = sfa.PolicyHead(n, A, seed=SEED)
    parts = [sfa.PolicyHead(k, A, seed=SEED, first_lane=0), sfa.PolicyHead(n - k, A, seed=SEED, first_lane=k)]
    xs = _logits(sfa, x)
    for call in range(2):
        w = whole.sample(xs)
        p = [parts[0].sample(xs[:k]), parts[1].sample(xs[k:])]
        for j in range(3):
            assert torch.equal(w[j], torch.cat([p[0][j], p[1][j]])), (call, j)
    assert w[0].shape == (n, 1) and w[0].dtype == torch.int64 and w[1].shape == (n, 1) and w[2].shape == (n,)
    assert np.array_equal(w[0][:, 0].cpu().numpy(), PR.policy_head(x, seed=SEED, ticks=1)["action"])


@pytest.mark.gpu
def test_bad_rows_play_action_zero_and_are_counted(sfa):
    n, A = 130, 5
    good = PR.general_rows(n, A, 1.0, 5)
    x = good.copy()
    nan_rows, inf_rows, empty_rows = [0, 63, 70], [64, 129], [5, 65, 100]
    for i in nan_rows:
        x[i, i % A] = np.nan
    for i in inf_rows:
        x[i, (i + 1) % A] = np.inf
    for i in empty_rows:
        x[i] = -np.inf
    bad = np.zeros(n, bool)
    bad[nan_rows + inf_rows + empty_rows] = True
    for mode in (0, 1):
        raw, ref = Raw(sfa, x, act_dtype=torch.int32), Raw(sfa, good, act_dtype=torch.int32)
        assert raw.call(mode=mode) == 0 and ref.call(mode=mode) == 0
        (a, logp, ent, ticks, count), (a0, logp0, ent0, ticks0, count0) = raw.host(), ref.host()
        assert count == bad.sum() and count0 == 0 and np.array_equal(ticks, ticks0)  # (a bad row consumes its tick)
        assert (a[bad] == 0).all() and np.isnan(logp[bad]).all() and np.isnan(ent[bad]).all()
        assert np.array_equal(a[~bad], a0[~bad]) and np.array_equal(logp[~bad], logp0[~bad]) and np.array_equal(ent[~bad], ent0[~bad])
        model = PR.policy_head(x, mode=mode, seed=SEED, first_lane=FIRST_LANE, ticks=0)
        assert np.array_equal(model["bad"], bad) and np.array_equal(a[bad], model["action"][bad])
        assert raw.call(mode=mode, bad=0) == 0  # the counter is optional
        assert raw.host()[4] == bad.sum()
    head = sfa.PolicyHead(n, A, seed=SEED, first_lane=FIRST_LANE)
    xs = _logits(sfa, x)
    head.sample(xs)
    head.sample(xs, deterministic=True)
    assert head.check() == 2 * bad.sum() and head.check() == 0
    head.sample(_logits(sfa, good))
    assert head.check() == 0


@pytest.mark.gpu
def test_refusals_launch_nothing(sfa):
    from spacefortress_amd import _lib
    n, A = 130, 5
    raw = Raw(sfa, PR.general_rows(n, A, 1.0, 6), stride=A + 3)
    TR.refill(raw.ticks, raw.bad)
    cases = [dict(logits=0), dict(act=0), dict(n=0), dict(n=-5), dict(A=0), dict(A=33, stride=40), dict(stride=A - 1), dict(mode=2),
             dict(mode=-1), dict(at=2), dict(at=0), dict(ticks=0), dict(logits=raw.logits.data_ptr() + 2)]
    for over in cases:
        assert raw.call(**over) == _lib.SF_ERR_ARG, over
        assert "sf_policy_sample" in _lib.last_error(), over
    torch.cuda.synchronize()
    assert TR.untouched(raw.act, raw.logp, raw.ent, raw.ticks, raw.bad)
    TR.margins_intact(raw.act, raw.logp, raw.ent, raw.ticks, raw.bad)
    with pytest.raises(ValueError, match="sf_policy_sample"):
        _lib.check(raw.call(mode=3))
    # the class refuses what it can see before the call
    with pytest.raises(ValueError):
        sfa.PolicyHead(4, 33)
    head = sfa.PolicyHead(4, 3)
    with pytest.raises(ValueError):
        head.sample(torch.zeros(4, 5, device="cuda"))
    with pytest.raises(ValueError):
        head.sample(torch.zeros(4, 3, device="cuda"), out=(torch.zeros(4, device="cuda"), None, None))  # float actions


@pytest.mark.gpu
def test_the_class_converts_what_is_not_dense_float32_and_carries_its_state(sfa):
    n, A = 130, 5
    x = PR.general_rows(n, A, 1.0, 7)
    head = sfa.PolicyHead(n, A, seed=SEED, first_lane=77)
    want = head.sample(_logits(sfa, x))
    wide = torch.zeros(n, A + 3, device="cuda")
    wide[:, :A] = _logits(sfa, x)
    views = [_logits(sfa, x).double(), wide[:, :A], _logits(sfa, x).t().contiguous().t()]
    for v in views:
        head.seed(SEED, 77)
        got = head.sample(v)
        assert all(torch.equal(g, w) for g, w in zip(got, want))
    sd = head.state_dict()
    assert sd["seed"] == SEED and sd["first_lane"] == 77 and (sd["ticks"] == 1).all() and sd["ticks"].dtype == np.uint32
    nxt = head.sample(_logits(sfa, x))
    twin = sfa.PolicyHead(n, A)
    twin.load_state_dict(sd)
    assert all(torch.equal(g, w) for g, w in zip(twin.sample(_logits(sfa, x)), nxt))
    # out: written in place, None for an output nobody needs
    act = torch.zeros(n, dtype=torch.uint8, device="cuda")
    twin.load_state_dict(sd)
    a, lp, en = twin.sample(_logits(sfa, x), out=(act, None, None))
    assert lp is None and en is None and a.data_ptr() == act.data_ptr() and torch.equal(act.long(), nxt[0][:, 0])


@pytest.mark.gpu
def test_a_captured_graph_draws_from_the_logits_anew_at_every_replay(sfa):
    n = 2048
    env, twin = sfa.SFVecEnv(n, reuse_buffers=True), sfa.SFVecEnv(n, reuse_buffers=True)
    A = env.n_actions
    x = PR.general_rows(n, A, 1.0, 8)
    head = sfa.PolicyHead(n, A, seed=SEED, device=env.device)
    xs = torch.from_numpy(x).to(env.device)
    env.reset()
    twin.reset()
    act = torch.zeros(n, dtype=torch.uint8, device=env.device)
    logp, ent = torch.zeros(n, device=env.device), torch.zeros(n, device=env.device)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=env.device)
    side.wait_stream(torch.cuda.current_stream(env.device))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        head.sample(xs, out=(act, logp, ent))  # the warm-up: tick 0
        out = env.step_tensors(act)
        torch.cuda.synchronize()
        warm = act.clone()
        with torch.cuda.graph(g, stream=side):
            head.sample(xs, out=(act, logp, ent))
            out = env.step_tensors(act)
    torch.cuda.current_stream(env.device).wait_stream(side)
    torch.cuda.synchronize()
    twin.step_tensors(warm)
    for rep in range(3):
        g.replay()
        torch.cuda.synchronize()
        model = PR.policy_head(x, seed=SEED, ticks=rep + 1)
        hold_to_model(x, act.cpu().numpy().astype(np.int64), logp.cpu().numpy(), ent.cpu().numpy(), model, ("replay", rep))
        want = twin.step_tensors(act.clone())
        assert all(torch.equal(o, w) for o, w in zip(out, want)), rep
    assert (head.ticks == 4).all() and head.check() == 0
    env.close()
    twin.close()


def _storages(ro):
    names = ["rewards", "masks", "actions", "action_log_probs", "value_preds", "episode_rewards", "final_rewards"]
    names += ["frames", "starts"] if hasattr(ro, "frames") else ["observations"]
    return {k: getattr(ro, k) for k in names}


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["features", "normalized", "frames", "frames-skip2"])
def test_step_logits_equals_step_with_the_heads_actions(sfa, kind):
    n, T = 65, 8

    def make():
        if kind == "features":
            return sfa.DeviceRollout(sfa.SFVecEnv(n, spawn_stride=1), T)
        if kind == "normalized":
            return sfa.DeviceRollout(sfa.SFVecNormalize(sfa.SFVecEnv(n, spawn_stride=1)), T)
        return sfa.FrameRollout(sfa.SFVecEnv(n, obs_type="image", spawn_stride=1, frame_skip=2 if kind == "frames-skip2" else 1), T)

    a, b = make(), make()
    A, dev = a.env.n_actions, a.env.device
    r = np.random.default_rng(9)
    logits = [torch.from_numpy(PR.general_rows(n, A, 1.0, 20 + t)).to(dev) for t in range(T)]
    values = [torch.from_numpy(r.standard_normal((n, 1)).astype(np.float32)).to(dev) for t in range(T)]
    assert a.policy is None
    a.seed_policy(SEED, 11)
    head = sfa.PolicyHead(n, A, seed=SEED, first_lane=11, device=dev)
    a.reset()
    b.reset()
    for t in range(T):
        det = t == 5  # one deterministic step: the argmax, the ticks as they were
        ticks = a.policy.ticks.clone()
        ra = a.step_logits(t, logits[t], value_pred=values[t], deterministic=det)
        act, logp, ent = head.sample(logits[t], deterministic=det)
        rb = b.step(t, act, value_pred=values[t], action_log_prob=logp)
        assert all(torch.equal(p, q) for p, q in zip(ra, rb)), t
        assert torch.equal(a.policy_entropy, ent) and torch.equal(a.policy.ticks, head.ticks)
        if det:
            assert torch.equal(a.policy.ticks, ticks) and torch.equal(a.actions[t][:, 0], logits[t].argmax(1))
        else:
            assert torch.equal(a.policy.ticks, ticks + 1)
    sa, sb = _storages(a), _storages(b)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert a.actions.dtype == torch.int64 and bool((a.actions != b.actions[0]).any())  # (not one action all the way through)
    assert a.policy.check() == 0 and isinstance(a.policy, sfa.PolicyHead)
    a.env.close()
    b.env.close()
