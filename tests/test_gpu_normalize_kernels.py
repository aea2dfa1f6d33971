"""sf_norm_reduce_kernel / sf_norm_merge_kernel / sf_norm_apply_kernel on synthetic data, through the C ABI
(sf_normalizer_create / sf_normalize / get_state / set_state) with torch tensors: no game, so every launch shape is
reachable.  Everything is compared with the exact reference of tests/normref.py within the error bound derived there
from the kernels' own sequence of float64 operations (MARGIN = 2 times the bound, nothing tuned); counts and the
per-env returns are compared exactly.  test_normalize_model.py shows on the CPU that reference and bound are sound.

Batch sizes and what each is there for (reduce: 1024 waves, 64 rows a chunk; apply: at most 2048 workgroups, rounded up
to a multiple of dim, times 256 threads -- 27 648 rows at dim 19):

      n       reduction                                        apply
      1       one row, batch variance exactly 0                one thread
     63       ragged only chunk                                one workgroup of dim
     64       exactly one chunk
     65       a full chunk and a chunk of one row
    333       6 chunks, the last ragged
  4 096       64 chunks: the size the suite has always run
 27 648       432 chunks                                       dim 19: the capped grid covers it exactly, no 2nd pass
 65 536       1024 chunks: every wave exactly one              grid-stride loop, 3 passes
 65 537       wave 0 loops a second time for one row           ragged last pass
100 000       1563 chunks: 539 waves take two                  4 passes
262 144       4096 chunks: every wave four
262 145       wave 0 a fifth, of one row                       every tail at once
"""
import ctypes as C

import numpy as np
import pytest

import normref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PATTERN, Norm = R.PATTERN, R.Norm
STEPS = 10

# (n, dim, float64).  Every n with dim 19 float32 and with another dim in float64; every dim with an n above 65 536
# and with one that is not a multiple of 64.
CASES = [(1, 19, False), (1, 1, True), (63, 19, False), (63, 3, True), (64, 19, False), (64, 4, True), (65, 19, False),
         (65, 5, True), (333, 19, False), (333, 10, True), (333, 21, False), (333, 24, True), (333, 1, False), (333, 17, True),
         (333, 4, False), (4096, 19, False), (4096, 17, True), (27648, 19, False), (27648, 21, True), (65536, 19, False),
         (65536, 24, True), (65537, 19, False), (65537, 1, True), (65537, 3, False), (65537, 10, True), (100000, 19, False),
         (100000, 5, True), (100000, 17, False), (262144, 19, False), (262144, 4, True), (262145, 19, False), (262145, 21, True),
         (262145, 24, False)]


def test_case_table_covers_what_it_says():
    ns = {1, 63, 64, 65, 333, 4096, 27648, 65536, 65537, 100000, 262144, 262145}
    dims = {1, 3, 4, 5, 10, 17, 19, 21, 24}
    assert {c[0] for c in CASES} == ns and {c[1] for c in CASES} == dims
    for n in ns:
        assert (n, 19, False) in CASES and any(c[0] == n and c[1] != 19 and c[2] for c in CASES), n
    for d in dims:
        assert any(c[1] == d and c[0] > 65536 for c in CASES) and any(c[1] == d and c[0] % 64 for c in CASES), d


@pytest.fixture(scope="module")
def lib():
    import spacefortress_amd  # noqa: F401  (the package loads and checks libsfmi.so)
    from spacefortress_amd import _lib
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    yield _lib
    print()
    for line in R.record_lines():
        print(line)


def _run(lib, fam, n, dim, f64, ob=True, ret=True, obs_kind="game", rew_kind="game", steps=STEPS, start=None):
    """A reset-form call, then `steps` training calls on fresh data, in place on even steps and out of place on odd ones;
    everything compared after every call.  -> the largest observation error seen (for the record)"""
    z = Norm(lib, n, dim, f64, ob, ret)
    ex = R.ExactVecNormalize(n, dim, ob=ob, ret=ret)
    d_ob, d_ret = R.depth_standalone(n, dim)
    if start is not None:
        z.set_state(start)
        ex.load(start)
    init = z.state()[0]
    worst_abs = 0.0

    def compare(tag, got_obs, x, want_obs, tol_obs, got_rew=None, want_rew=None, tol_rew=None):
        nonlocal worst_abs
        if ob:
            R.check(fam, "obs", got_obs.cpu().numpy(), want_obs, tol_obs, where=tag)
            worst_abs = max(worst_abs, float(np.abs(got_obs.cpu().numpy().astype(np.float64) - want_obs).max()))
        else:  # VecNormalize(ob=False): observations are not this call's business
            assert bool((got_obs == PATTERN).all()), tag
        if got_rew is not None:
            if ret:
                R.check(fam, "rew", got_rew.cpu().numpy(), want_rew, tol_rew, where=tag)
            else:
                assert bool((got_rew == PATTERN).all()), tag
        st, rt = z.state()
        R.check_stats(fam, ex, st, rt, where=tag)
        if not ob:
            assert np.array_equal(st[:2 * dim], init[:2 * dim]) and st[2 * dim + 2] == init[2 * dim + 2], tag
        if not ret:
            assert np.array_equal(st[2 * dim:2 * dim + 2], init[2 * dim:2 * dim + 2]) and st[2 * dim + 3] == init[2 * dim + 3], tag
            assert not rt.any(), tag

    # VecNormalize.reset: observations only
    x = R.gen_obs(obs_kind, n, dim, 1000, z.ndt)
    src = z.dev_obs(x)
    assert z.call(src[1:-1], z.obs_out) == 0
    want, tol = ex.obfilt(x, z.ndt, d_ob)
    compare("reset", z.obs_out, x, want, tol)
    assert torch.equal(src[1:-1].cpu(), torch.from_numpy(x.astype(z.ndt))), "out-of-place call changed its input"
    z.guards_intact(src)
    for t in range(steps):
        x, r = R.gen_obs(obs_kind, n, dim, t, z.ndt), R.gen_rew(rew_kind, n, t)
        src, rew = z.dev_obs(x), torch.from_numpy(r).to(z.dev)
        z.obs_out.fill_(PATTERN)
        z.rew_out.fill_(PATTERN)
        inplace = t % 2 == 0 and ob
        out = src[1:-1] if inplace else z.obs_out
        assert z.call(src[1:-1], out, rew, z.rew_out) == 0
        want, tol, wr, tr = ex.step(x, r, z.ndt, d_ob, d_ret)
        compare("step %d" % t, out, x, want, tol, z.rew_out, wr, tr)
        if not inplace:
            assert torch.equal(src[1:-1].cpu(), torch.from_numpy(x.astype(z.ndt))), "out-of-place call changed its input"
        assert torch.equal(rew.cpu(), torch.from_numpy(r)), "the raw rewards were changed"
        z.guards_intact(src)
    z.close()
    return worst_abs


@pytest.mark.parametrize("n,dim,f64", CASES)
def test_every_launch_shape(lib, n, dim, f64):
    rew_kind = R.REW_KINDS[(n + dim) % len(R.REW_KINDS)]
    _run(lib, "standalone/shapes", n, dim, f64, rew_kind=rew_kind)


@pytest.mark.parametrize("n,dim,f64", [(65, 19, False), (4096, 10, True), (65537, 19, False), (100000, 24, True)])
@pytest.mark.parametrize("ob,ret", [(True, False), (False, True)])
def test_ob_only_and_ret_only(lib, n, dim, f64, ob, ret):
    _run(lib, "standalone/ob-only" if ob else "standalone/ret-only", n, dim, f64, ob=ob, ret=ret, rew_kind="game")


# two reward kinds per observation kind; every reward kind twice
@pytest.mark.parametrize("obs_kind,rew_kind", [(k, R.REW_KINDS[(i + j) % 4]) for i, k in enumerate(R.WELL_CONDITIONED) for j in (0, 2)])
def test_generators_at_65537x19(lib, obs_kind, rew_kind):
    _run(lib, "standalone/" + obs_kind, 65537, 19, False, obs_kind=obs_kind, rew_kind=rew_kind)


@pytest.mark.parametrize("n", [65537, 100000])
def test_constant_columns_in_float64(lib, n):
    """Columns of one value that float64 does not hold exactly (355.1, 0.1, 1e-3): every partial sum rounds, so the one-pass
    batch variance comes out a rounding error above or BELOW zero where the exact one is 0.  The kernel clamps it at 0; the
    variance's lower bound (normref: ev_lo) holds it to that -- a constant column must not pull the running variance down."""
    _run(lib, "standalone/constant-f64", n, 19, True, obs_kind="constant", rew_kind="equal")


@pytest.mark.parametrize("f64", [False, True])
@pytest.mark.parametrize("obs_kind", ["ill-1e-2", "ill-3e-4"])
def test_ill_conditioned_at_65537x19(lib, obs_kind, f64):
    """mean 1000, deviation 1e-2 / 3e-4, from the state of a long-trained normaliser (normref.ill_start): the one-pass
    batch variance is only good to mean(x^2) / var * 2^-53 relative, and so is the bound these cases are held to
    (3e-5 and 3e-2 on an output here).  sfmi.h states the limit; profiles/norm_tests.md has the measured errors."""
    worst = _run(lib, "standalone/%s/%s" % (obs_kind, "f64" if f64 else "f32"), 65537, 19, f64, obs_kind=obs_kind, rew_kind="big",
                 start=R.ill_start(obs_kind, 19))
    print("NORMREC ill-conditioned %s %s: largest |out - exact| = %.3e" % (obs_kind, "f64" if f64 else "f32", worst))


@pytest.mark.parametrize("n,dim,f64", [(1, 19, False), (333, 5, True), (65537, 19, False), (262145, 17, True)])
def test_frozen_before_and_after_updates(lib, n, dim, f64):
    z, ex = Norm(lib, n, dim, f64), R.ExactVecNormalize(n, dim)
    d_ob, d_ret = R.depth_standalone(n, dim)
    fam = "standalone/frozen"
    for phase in range(2):
        before = z.state()
        x, r = R.gen_obs("game", n, dim, 50 + phase, z.ndt), R.gen_rew("game", n, 50 + phase)
        src, rew = z.dev_obs(x), torch.from_numpy(r).to(z.dev)
        z.obs_out.fill_(PATTERN)
        assert z.call(src[1:-1], z.obs_out, rew, z.rew_out, frozen=True) == 0
        want, tol, wr, tr = ex.step(x, r, z.ndt, d_ob, d_ret, update=False)
        R.check(fam, "obs", z.obs_out.cpu().numpy(), want, tol, where="phase %d" % phase)
        R.check(fam, "rew", z.rew_out.cpu().numpy(), wr, tr, where="phase %d" % phase)
        after = z.state()
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]), "a frozen call changed the state"
        z.guards_intact(src)
        for t in range(3):  # some updates in between
            x, r = R.gen_obs("game", n, dim, t, z.ndt), R.gen_rew("game", n, t)
            src, rew = z.dev_obs(x), torch.from_numpy(r).to(z.dev)
            assert z.call(src[1:-1], src[1:-1], rew, z.rew_out) == 0
            ex.step(x, r, z.ndt, d_ob, d_ret)
    z.close()


def _feed(z, steps, first=0, kind="game"):
    outs = []
    for t in range(first, first + steps):
        x, r = R.gen_obs(kind, z.n, z.dim, t, z.ndt), R.gen_rew("big", z.n, t)
        src, rew = z.dev_obs(x), torch.from_numpy(r).to(z.dev)
        assert z.call(src[1:-1], src[1:-1], rew, z.rew_out) == 0
        outs.append((src[1:-1].cpu().numpy().copy(), z.rew_out.cpu().numpy().copy()))
    return outs


def _same(a, b):
    return all(np.array_equal(x[0].view(np.uint8), y[0].view(np.uint8)) and np.array_equal(x[1].view(np.uint8), y[1].view(np.uint8))
               for x, y in zip(a, b)) and len(a) == len(b)


@pytest.mark.parametrize("n,dim,f64", [(100000, 19, False), (65537, 24, True)])
def test_run_to_run_determinism(lib, n, dim, f64):
    a, b = Norm(lib, n, dim, f64), Norm(lib, n, dim, f64)
    start = a.state()
    oa, ob_ = _feed(a, 10), _feed(b, 10)
    assert _same(oa, ob_), "two normalisers fed the same ten steps differ"
    sa, sb = a.state(), b.state()
    assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1])
    a.set_state(*start)  # the same normaliser again, from its own start state
    assert _same(oa, _feed(a, 10))
    sa2 = a.state()
    assert np.array_equal(sa[0], sa2[0]) and np.array_equal(sa[1], sa2[1])
    a.close()
    b.close()


@pytest.mark.parametrize("n,dim,f64", [(65537, 19, False), (333, 10, True)])
def test_state_moves_across_buffer_parity(lib, n, dim, f64):
    """The statistics are double-buffered and the buffer in use flips at every training call; set_state writes the current
    one only.  A state saved after an odd number of calls continues identically in a fresh normaliser (parity 0)."""
    a, b = Norm(lib, n, dim, f64), Norm(lib, n, dim, f64)
    _feed(a, 3)
    b.set_state(*a.state())
    oa, ob_ = _feed(a, 3, first=3), _feed(b, 3, first=3)
    assert _same(oa, ob_)
    sa, sb = a.state(), b.state()
    assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1])
    # and the numbers are the right ones, not merely equal: statistics against the exact reference
    ex = R.ExactVecNormalize(n, dim)
    d_ob, d_ret = R.depth_standalone(n, dim)
    for t in range(6):
        ex.step(R.gen_obs("game", n, dim, t, a.ndt), R.gen_rew("big", n, t), a.ndt, d_ob, d_ret)
    R.check_stats("standalone/parity", ex, sb[0], sb[1])
    a.close()
    b.close()


def test_training_call_is_refused_inside_a_capture(lib):
    """sfmi.h: a call that updates the statistics flips the double buffer on the host, which a replayed graph would not do:
    refused with SF_ERR_ARG before anything is launched; the capture ends cleanly and the normaliser works on."""
    n, dim = 4096, 19
    z = Norm(lib, n, dim)
    x, r = R.gen_obs("game", n, dim, 0), R.gen_rew("game", n, 0)
    src, rew = z.dev_obs(x), torch.from_numpy(r).to(z.dev)
    before = z.state()
    scratch = torch.zeros(16, device=z.dev)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        scratch.add_(1)  # (the graph is not empty)
        rc = z.call(src[1:-1], z.obs_out, rew, z.rew_out)
        rc_reset = z.call(src[1:-1], z.obs_out)
    assert rc == lib.SF_ERR_ARG and rc_reset == lib.SF_ERR_ARG, (rc, rc_reset)
    g.replay()
    torch.cuda.synchronize()
    assert bool((z.obs_out == PATTERN).all()) and bool((z.rew_out == PATTERN).all()), "a refused call launched something"
    after = z.state()
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    # eager again: the refused calls did not flip the buffer
    ex = R.ExactVecNormalize(n, dim)
    assert z.call(src[1:-1], z.obs_out, rew, z.rew_out) == 0
    want, tol, wr, tr = ex.step(x, r, z.ndt, *R.depth_standalone(n, dim))
    R.check("standalone/capture", "obs", z.obs_out.cpu().numpy(), want, tol)
    R.check_stats("standalone/capture", ex, *z.state())
    z.guards_intact(src)
    z.close()


def test_frozen_call_replays_from_a_graph(lib):
    n, dim = 65537, 19
    z = Norm(lib, n, dim)
    _feed(z, 3)
    x, r = R.gen_obs("game", n, dim, 77), R.gen_rew("game", n, 77)
    src, rew = z.dev_obs(x), torch.from_numpy(r).to(z.dev)
    assert z.call(src[1:-1], z.obs_out, rew, z.rew_out, frozen=True) == 0
    eager = (z.obs_out.cpu().numpy().copy(), z.rew_out.cpu().numpy().copy())
    st = z.state()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        rc = z.call(src[1:-1], z.obs_out, rew, z.rew_out, frozen=True)
    assert rc == 0
    for it in range(3):
        z.obs_out.fill_(PATTERN)
        z.rew_out.fill_(PATTERN)
        g.replay()
        torch.cuda.synchronize()
        assert _same([eager], [(z.obs_out.cpu().numpy(), z.rew_out.cpu().numpy())]), it
    after = z.state()
    assert np.array_equal(st[0], after[0]) and np.array_equal(st[1], after[1])
    z.guards_intact(src)
    z.close()
