"""Lane states on the device (include/sfmi.h: sf_save_lanes / sf_load_lanes / sf_copy_lanes / sf_check_lanes): a state saved
from one lane and loaded into another -- another tile, another batch, many lanes at once -- plays on exactly as the original
does, against the batch itself and against the CPU oracle."""

import numpy as np
import pytest

from sfcompare import compare_state, obs_close
from sfscript import firing_actions, largest_pool, open_loop_actions
from lockstep import sfa

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _acts(env, T, rng, policy="hunter"):
    a = open_loop_actions(policy, (T, env.num_envs), env.n_actions, rng, phase=np.arange(env.num_envs) % 40)
    return torch.from_numpy(a).to(env.device)


def _play(env, T, rng, policy="hunter"):
    env.rollout(_acts(env, T, rng, policy), want_obs=False)


def _near_game_over(env, rng, every=3, within=30):
    t = env.get_field("time")
    t[::every] = 180000 - 34 * rng.integers(1, within, len(t[::every]))
    env.set_field("time", t)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def _sd_permuted_equal(sd_dst, sd_src, perm):
    """sd_dst[..., perm[k]] == sd_src[..., k] for every field, bit for bit; the names of the fields that differ"""
    return [f for f in sd_src if not _same_bits(np.asarray(sd_dst[f])[..., perm], sd_src[f])]


def _bits(t):
    return t.contiguous().view(torch.int64 if t.element_size() == 8 else torch.int32) if t.is_floating_point() else t


@pytest.mark.parametrize("gametype,n", [("youturn", 200), ("autoturn", 200), ("youturn", 65536), ("autoturn", 131072)])
def test_permuted_load_continues_bit_identically(sfa, gametype, n):
    """Batch A plays (hunter script: full pools, kills, deaths, respawns), every lane is saved and loaded into batch B under a
    random permutation (lanes change tiles); both play on with the correspondingly permuted actions across episode ends and
    auto-resets.  200 lanes: a partial tile; 65 536: the split launches; 131 072: several waves per SIMD."""
    rng = np.random.default_rng(n + len(gametype))
    A = sfa.SFVecEnv(n, gametype=gametype, spawn_stride=1)
    B = sfa.SFVecEnv(n, gametype=gametype, spawn_stride=1)
    _play(A, 150, rng)
    _play(B, 7, rng, "charger")  # (B's own pools and states are overwritten everywhere)
    _near_game_over(A, rng)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(n)).to(A.device)
    pn = perm.cpu().numpy()
    B.load_lanes(A.save_lanes(), lanes=perm)
    sdA = A.state_dict()
    assert not _sd_permuted_equal(B.state_dict(), sdA, pn)
    evA, evB = A.enable_events(), B.enable_events()
    acts = _acts(A, 40, rng)
    n_done = 0
    for t in range(40):
        a = acts[t].contiguous()
        ap = torch.empty_like(a)
        ap[perm] = a
        oA, rA, dA, iA = (x.clone() for x in A.step_tensors(a))
        oB, rB, dB, iB = B.step_tensors(ap)
        assert torch.equal(_bits(oB[perm]), _bits(oA)), t
        assert torch.equal(rB[perm], rA) and torch.equal(dB[perm], dA) and torch.equal(iB[perm], iA), t
        assert torch.equal(evB[perm], evA), t
        n_done += int(dA.sum())
    assert n_done >= n // 3 - 1
    assert not _sd_permuted_equal(B.state_dict(), A.state_dict(), pn)
    A.check_lanes()
    B.check_lanes()


def test_one_row_into_every_lane_against_the_oracle(sfa, oracle_mod):
    """One saved state forked into 256 lanes, each stepped with actions of its own, equals the oracle loaded with that state
    (OracleVecEnv.load_snapshots) and stepped with the same actions."""
    O = oracle_mod
    rng = np.random.default_rng(5)
    A = sfa.SFVecEnv(64, gametype="youturn", spawn_stride=1, obs_dtype=torch.float64)
    src = O.OracleVecEnv("youturn", 64, spawn_stride=1)
    acts = open_loop_actions("hunter", (160, 64), A.n_actions, rng, phase=np.arange(64) % 40)
    A.rollout(torch.from_numpy(acts).to(A.device), want_obs=False)
    for t in range(160):
        src.step(acts[t].astype(np.int32))
    assert not compare_state(A.state_dict(), src.snapshots())
    mm = A.get_field("missile_mask")
    j = int(np.argmax([bin(int(m)).count("1") for m in mm]))
    n = 256
    B = sfa.SFVecEnv(n, gametype="youturn", spawn_stride=1, obs_dtype=torch.float64)
    B.load_lanes(A.save_lanes([j]), rows=torch.zeros(n, dtype=torch.int64, device=B.device))
    orc = O.OracleVecEnv("youturn", n, spawn_stride=1)
    orc.load_snapshots(np.repeat(src.snapshots()[j:j + 1], n), np.repeat(src.prev_vlner()[j:j + 1], n))
    assert not compare_state(B.state_dict(), orc.snapshots())
    b_acts = rng.integers(0, B.n_actions, (60, n)).astype(np.uint8)
    for t in range(60):
        o, r, d, i = (x.cpu().numpy() for x in B.step_tensors(torch.from_numpy(b_acts[t]).to(B.device)))
        oo, orw, od, oi = orc.step(b_acts[t].astype(np.int32))
        assert np.array_equal(r, orw) and np.array_equal(d.astype(bool), od) and np.array_equal(i.astype(bool), oi), t
        assert obs_close(o, oo, True).all(), t
    assert not compare_state(B.state_dict(), orc.snapshots())


def _expected_copy(sd, dst, src):
    out = {k: np.array(v, copy=True) for k, v in sd.items()}
    for d, s in zip(dst, src):  # in order: the last occurrence of a destination wins
        for k in out:
            out[k][..., d] = sd[k][..., s]
    return out


def test_copy_lanes_in_place_equals_the_host_copy(sfa):
    """copy_lanes inside one batch with overlapping source and destination sets -- a rotation inside a tile, a swap across
    tiles, a destination named twice -- equals the same copy made through state_dict() on the host."""
    rng = np.random.default_rng(3)
    A = sfa.SFVecEnv(200, gametype="youturn", spawn_stride=1)
    _play(A, 120, rng)
    sd = A.state_dict()
    dst = list(range(10)) + [70, 130, 5, 199]
    src = list(range(1, 10)) + [0] + [130, 70, 150, 5]
    exp = _expected_copy(sd, dst, src)
    A.copy_lanes(dst, src)
    H = sfa.SFVecEnv(200, gametype="youturn", spawn_stride=1)
    H.load_state_dict(exp)
    sdA = A.state_dict()
    assert not [k for k in exp if not _same_bits(sdA[k], exp[k])]
    acts = _acts(A, 30, rng)
    for t in range(30):
        oA, rA, dA, _ = (x.clone() for x in A.step_tensors(acts[t].contiguous()))
        oH, rH, dH, _ = H.step_tensors(acts[t].contiguous())
        assert torch.equal(_bits(oA), _bits(oH)) and torch.equal(rA, rH) and torch.equal(dA, dH), t
    # another batch of the same preset, seed and table; then incompatible ones, refused before any launch
    C2 = sfa.SFVecEnv(64, gametype="youturn", spawn_stride=1)
    C2.copy_lanes([0, 1], [5, 6], src=A)
    sdC = C2.state_dict()
    sdA = A.state_dict()
    assert not [k for k in sdA if not _same_bits(np.asarray(sdC[k])[..., [0, 1]], np.asarray(sdA[k])[..., [5, 6]])]
    for other in (sfa.SFVecEnv(64, gametype="youturn", seed=2, spawn_stride=1), sfa.SFVecEnv(64, gametype="autoturn", spawn_stride=1),
                  sfa.SFVecEnv(64, gametype="youturn", spawn_stride=1, spawn_table_len=1 << 18)):
        with pytest.raises(ValueError):
            C2.copy_lanes([0], [0], src=other)


def test_whole_batch_round_trip_equals_state_dict(sfa):
    rng = np.random.default_rng(4)
    A = sfa.SFVecEnv(300, gametype="autoturn", spawn_stride=2)
    _play(A, 90, rng)
    C1 = sfa.SFVecEnv(300, gametype="autoturn", spawn_stride=2)
    C2 = sfa.SFVecEnv(300, gametype="autoturn", spawn_stride=2)
    C1.load_lanes(A.save_lanes())
    C2.load_state_dict(A.state_dict())
    s1, s2 = C1.state_dict(), C2.state_dict()
    assert not [k for k in s1 if not _same_bits(s1[k], s2[k])]
    acts = _acts(A, 30, rng)
    for t in range(30):
        o1 = C1.step_tensors(acts[t].contiguous())[0].clone()
        o2 = C2.step_tensors(acts[t].contiguous())[0]
        assert torch.equal(_bits(o1), _bits(o2)), t


def test_refused_rows_leave_their_lanes_alone(sfa):
    rng = np.random.default_rng(6)
    B = sfa.SFVecEnv(100, gametype="youturn", spawn_stride=1)
    _play(B, 40, rng)
    before = B.state_dict()
    good = sfa.SFVecEnv(8, gametype="youturn", spawn_stride=1)
    _play(good, 30, rng)
    bad = [sfa.SFVecEnv(8, gametype="youturn", seed=9, spawn_stride=1).save_lanes(),
           sfa.SFVecEnv(8, gametype="youturn", spawn_stride=1, spawn_table_len=1 << 18).save_lanes(),
           sfa.SFVecEnv(8, gametype="test-youturn", spawn_stride=1).save_lanes()]
    for rows in bad:
        with pytest.raises(ValueError):
            B.load_lanes(rows, lanes=[3, 70])
        B.load_lanes(rows, lanes=[3, 70], check=False)
        with pytest.raises(ValueError):
            B.check_lanes()
        B.check_lanes()  # (read and cleared)
    rows = good.save_lanes()
    for lanes, ridx in (([100], [0]), ([-1], [0]), ([4], [8]), ([4], [-2])):
        with pytest.raises(ValueError):
            B.load_lanes(rows, lanes=lanes, rows=ridx)
    after = B.state_dict()
    assert not [k for k in before if not _same_bits(before[k], after[k])]
    # valid and refused pairs in one call: the valid ones land
    with pytest.raises(ValueError):
        B.load_lanes(rows, lanes=[10, 200, 11], rows=[2, 0, 7])
    sdg, sdb = good.state_dict(), B.state_dict()
    assert not [k for k in sdg if not _same_bits(np.asarray(sdb[k])[..., [10, 11]], np.asarray(sdg[k])[..., [2, 7]])]
    with pytest.raises(ValueError):  # a save of a lane outside the batch: a row nobody takes, counted
        good.save_lanes([8])
        good.check_lanes()


@pytest.mark.parametrize("obs_type", ["features", "normalized-features", "monitors"])
@pytest.mark.parametrize("f64", [False, True])
def test_load_writes_the_source_observation(sfa, obs_type, f64):
    """obs written by a load = what the source lane's last step returned (lanes that just auto-reset included), bit for bit;
    and a new game's = what reset() returned, with SF_FLAG_REF_RESET_OBS too."""
    rng = np.random.default_rng(7)
    dt = torch.float64 if f64 else torch.float32
    for ref in (False, True):
        A = sfa.SFVecEnv(130, gametype="youturn", obs_type=obs_type, obs_dtype=dt, spawn_stride=1, ref_reset_obs=ref)
        B = sfa.SFVecEnv(130, gametype="youturn", obs_type=obs_type, obs_dtype=dt, spawn_stride=1, ref_reset_obs=ref)
        o0 = A.reset().clone()
        buf = torch.full_like(o0, 7.0)
        B.load_lanes(A.save_lanes(), obs=buf)
        assert torch.equal(_bits(buf), _bits(o0))
        _play(A, 80, rng)
        _near_game_over(A, rng, every=2, within=6)
        acts = _acts(A, 8, rng)
        for t in range(8):
            last = A.step_tensors(acts[t].contiguous())[0].clone()
        perm = torch.randperm(130, generator=torch.Generator().manual_seed(1)).to(A.device)
        buf = torch.full_like(last, 7.0)
        B.load_lanes(A.save_lanes(), lanes=perm, obs=buf)
        assert torch.equal(_bits(buf[perm]), _bits(last))


@pytest.mark.parametrize("geometry", [None, (.25, (130, 80, 450, 460), 3)])
def test_frames_after_a_load(sfa, geometry):
    """Image batches: frames after a load (raw and 84x84) equal the source lanes' frames, lanes restored mid-explosion among
    them, the destination's explosion cache holding other explosions; and after further steps the twins' frames agree."""
    rng = np.random.default_rng(8)
    n = 192
    A = sfa.SFVecEnv(n, gametype="youturn", obs_type="image", spawn_stride=1, image_geometry=geometry)
    B = sfa.SFVecEnv(n, gametype="youturn", obs_type="image", spawn_stride=1, image_geometry=geometry)
    acts = _acts(A, 120, rng, "charger")
    for t in range(120):
        A.step_tensors(acts[t].contiguous())
    for t in range(40):
        B.step_tensors(_acts(B, 1, rng, "charger")[0].contiguous())
    dead = np.flatnonzero((A.get_field("flags") & 1) == 0)
    assert len(dead) > 0  # (lanes restored mid-explosion)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(2)).to(A.device)
    B.load_lanes(A.save_lanes(), lanes=perm)
    for mode in ("image", "image-raw"):
        fA, fB = A.render(mode), B.render(mode)
        assert torch.equal(fB[perm], fA), mode
    if geometry is None:
        rA, rB = A.draw_records(from_state=True), B.draw_records(from_state=False)
        assert np.array_equal(rB[perm.cpu().numpy(), :48], rA[:, :48])
    acts = _acts(A, 20, rng, "charger")
    for t in range(20):
        a = acts[t].contiguous()
        ap = torch.empty_like(a)
        ap[perm] = a
        oA = A.step_tensors(a)[0].clone()
        oB = B.step_tensors(ap)[0]
        assert torch.equal(oB[perm], oA), t


def test_ssf_env_clone_and_restore(sfa):
    rng = np.random.default_rng(9)
    env = sfa.SSF_Env("youturn", obs_type="features")
    g = env.g
    for t in range(150):
        env.step(int(rng.integers(0, 5)) if t % 8 else 1)
    s = env.clone_state()
    names = ("dump", "points", "raw_points", "vulnerability", "time", "tick", "ship_alive", "ship_x", "ship_y", "ship_angle",
             "fortress_alive", "fortress_angle", "missiles", "shells", "stats", "timers", "events", "aim", "vdir", "ndist",
             "thrust_durations", "shot_durations", "shot_intervals_vul", "shot_intervals_invul")
    def look(e):
        out = {}
        for k in names:
            v = getattr(e.g, k)
            out[k] = v() if callable(v) else v
        return repr(out)
    ref = look(env)
    for t in range(20):
        env.step(int(rng.integers(0, 5)))
    assert look(env) != ref
    env.restore_state(s)
    assert look(env) == ref and g is env.g
    other = sfa.SSF_Env("youturn", obs_type="features")
    other.step(2)
    other.restore_state(s)
    assert look(other) == ref
    o1 = env.step(3)
    o2 = other.step(3)
    assert np.array_equal(o1[0], o2[0]) and o1[1:] == o2[1:]


def test_graph_capture_of_load_and_step(sfa):
    """A captured load_lanes(check=False) + step_tensors replays with new index and row tensors and matches eager calls."""
    rng = np.random.default_rng(10)
    n = 256
    A = sfa.SFVecEnv(n, gametype="youturn", spawn_stride=1)
    _play(A, 60, rng)
    rows = A.save_lanes().rows
    G = sfa.SFVecEnv(n, gametype="youturn", spawn_stride=1, reuse_buffers=True)
    E = sfa.SFVecEnv(n, gametype="youturn", spawn_stride=1)
    lanes = torch.arange(0, 32, dtype=torch.int64, device=G.device)
    ridx = torch.zeros(32, dtype=torch.int64, device=G.device)
    act = torch.zeros(n, dtype=torch.uint8, device=G.device)
    s = torch.cuda.Stream(device=G.device)
    s.wait_stream(torch.cuda.current_stream(G.device))
    with torch.cuda.stream(s):  # warm-up, eager
        G.load_lanes(rows, lanes=lanes, rows=ridx, check=False)
        G.step_tensors(act)
    torch.cuda.current_stream(G.device).wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        G.load_lanes(rows, lanes=lanes, rows=ridx, check=False)
        out = G.step_tensors(act)
    E.load_lanes(rows, lanes=lanes, rows=ridx, check=False)
    E.step_tensors(act)
    for it in range(3):
        lanes.copy_(torch.from_numpy(rng.choice(n, 32, replace=False)).to(G.device))
        ridx.copy_(torch.from_numpy(rng.integers(0, n, 32)).to(G.device))
        act.copy_(_acts(G, 1, rng)[0])
        graph.replay()
        E.load_lanes(rows, lanes=lanes, rows=ridx, check=False)
        oE = E.step_tensors(act)
        torch.cuda.synchronize()
        assert torch.equal(_bits(out[0]), _bits(oE[0])) and torch.equal(out[1], oE[1]), it
    G.check_lanes()
    sg, se = G.state_dict(), E.state_dict()
    assert not [k for k in sg if not _same_bits(sg[k], se[k])]


def test_every_pool_rebuild_plays_the_same_games(sfa):
    """A tile's missile pool is rebuilt in three places (sf_state_ops.hip: pool_rebuild): by a lane-state load, by the slot view
    behind load_state_dict and by the masked reset.  Batch A plays until its pools span more than one row; B takes A's lane
    states, C its state_dict; all three get the same masked reset (marks in the first tile and in the partial last one, where
    the lanes behind the batch count as kept and have no missiles) and then play the same 60 random actions: every output
    equal bit for bit at every tick, state_dict() equal field by field at the end.  160 envs: two full tiles and one of 32."""
    n = 160
    A, B, C = (sfa.SFVecEnv(n, gametype="youturn", action_set=1, spawn_stride=1) for _ in range(3))
    A.rollout(torch.from_numpy(firing_actions(400, n, A.n_actions, seed=11)).to(A.device), want_obs=False)
    pool = largest_pool(A)
    assert pool > 64, "the largest pool holds %d entries: one row" % pool
    mask = np.zeros(n, np.uint8)
    mask[0:64:2] = 1      # the first tile: every other lane
    mask[128:160:3] = 1   # the partial tile
    owns = A.get_field("missile_mask") != 0
    mixed = [t for t in range(3) if (owns & (mask != 0))[64 * t:64 * t + 64].any() and (owns & (mask == 0))[64 * t:64 * t + 64].any()]
    print("largest pool %d entries; tiles where a marked and a kept lane own missiles: %s" % (pool, mixed))
    assert mixed, "no tile in which a marked lane and a kept lane both own a missile"
    B.load_lanes(A.save_lanes())
    C.load_state_dict(A.state_dict())
    md = torch.from_numpy(mask).to(A.device)
    sel = md != 0
    oa, ob, oc = (E.reset_lanes(mask=md) for E in (A, B, C))
    assert torch.equal(_bits(oa)[sel], _bits(ob)[sel]) and torch.equal(_bits(oa)[sel], _bits(oc)[sel])
    acts = torch.from_numpy(np.random.default_rng(12).integers(0, A.n_actions, (60, n)).astype(np.uint8)).to(A.device)
    for t in range(60):
        ra, rb, rc = (E.step_tensors(acts[t]) for E in (A, B, C))
        for name, x, y, z in zip(("obs", "reward", "done", "info"), ra, rb, rc):
            assert torch.equal(_bits(x), _bits(y)), (t, name, "lane states")
            assert torch.equal(_bits(x), _bits(z)), (t, name, "state_dict")
    sa, sb, sc = A.state_dict(), B.state_dict(), C.state_dict()
    assert not [k for k in sa if not _same_bits(sa[k], sb[k])]
    assert not [k for k in sa if not _same_bits(sa[k], sc[k])]
    for E in (A, B, C):
        E.close()
