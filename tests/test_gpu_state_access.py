"""The state accessors and the lane-row kernels against an independent codec of the lane-state row (tests/lanerow_np.py).

sf_get_field / sf_set_field, the per-slot view of the missile pools behind them and state_dict() / load_state_dict() on top
are the instrument every parity test reads the device through; sf_save_lanes / sf_load_lanes move the same bits as rows whose
format sfmi.h and sf_layout.h document.  Here each is held to the numpy codec of that format, byte for byte: reads against
decoded rows, writes against encoded expectations over the whole row table (a write changes its own bits and nothing else),
rows in and fields out, the slot view as a state machine (write orders, dead slots, every entry point that has to flush it),
and one tick at the edges of the packed words against the oracle.  Nothing here has a tolerance.

Sizes: 1, 63, 64, 65, 255, 256, 257, 321 envs -- 256-thread copy kernels, 64-lane tile kernels, a state padded to 256 lanes,
partial last tiles of 1, 63 and 1 lanes.  The all-ones and NaN batches are never stepped, drawn or rendered.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import lanerow_np as R
from lockstep import sfa
from sfcompare import compare_state
from sfscript import firing_actions, open_loop_actions

pytestmark = pytest.mark.gpu

SIZES = [1, 63, 64, 65, 255, 256, 257, 321]
MISSILE_VIEW = ("missile_x", "missile_y", "missile_angle")
MISSILE_ALL = ("missile_mask",) + MISSILE_VIEW


# ------------------------------------------------------------------ helpers

def _rows(env, lanes=None):
    return env.save_lanes(lanes).rows.cpu().numpy()


def _load(env, rows, lanes=None, row_idx=None):
    env.load_lanes(torch.from_numpy(np.ascontiguousarray(rows)).to(env.device), lanes=lanes, rows=row_idx)


def _where(byte):
    """what a byte of a row belongs to (for a failure's text)"""
    if byte < 16:
        return "header"
    if byte < 128:
        return "%s+%d" % (R.CHUNKS[(byte - 16) // 16], (byte - 16) % 16)
    for at, name, size in ((R.PAD_AT, "pad", 8), (R.MISSILE_ANG_AT, "heading", 2), (R.MISSILE_POS_AT, "missile_pos", 16),
                           (R.SHELL_VEL_AT, "shell_vel", 16), (R.SHELL_POS_AT, "shell_pos", 16)):
        if byte >= at:
            return "%s[%d]+%d" % (name, (byte - at) // size, (byte - at) % size)


def _assert_rows(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got != want)
        r, b = (int(v) for v in bad[0])
        raise AssertionError("%s: %d bytes differ in %d rows; first: row %d byte %d (%s) is 0x%02x, expected 0x%02x; more: %s"
                             % (what, len(bad), len(set(bad[:, 0].tolist())), r, b, _where(b), got[r, b], want[r, b],
                                [(int(x), _where(int(y))) for x, y in bad[1:6]]))


def _assert_field(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.argwhere(got.view("u%d" % got.dtype.itemsize) != want.view("u%d" % want.dtype.itemsize))
        i = tuple(int(v) for v in bad[0])
        raise AssertionError("%s: %d elements differ; first at %s: %r, expected %r" % (what, len(bad), i, got[i], want[i]))


def _alive(mask):
    """[slot, env] bool from the envs' alive masks"""
    return ((np.asarray(mask, np.uint32)[None, :] >> np.arange(R.NSLOT, dtype=np.uint32)[:, None]) & 1).astype(bool)


def _after_write(cur, name, value):
    """The fields after set_field(name, value) and a flush of the slot view: that field replaced -- and, as the pools hold live
    missiles only, whatever the view holds for a dead slot gone."""
    new = dict(cur)
    count = R.FIELD_COUNT[name]
    v = np.asarray(value)
    new[name] = v.astype(R.FIELD_DTYPE[name]).reshape((-1,) if count == 1 else (count, -1))
    if name in MISSILE_ALL:
        dead = ~_alive(new["missile_mask"])
        for k in MISSILE_VIEW:
            a = new[k].copy()
            a[dead] = 0
            new[k] = a
    return new


F64_BITS = np.array([0x7FF8DEADBEEF0001, 0xFFF0000000000000, 0x7FF0000000000000, 0x0000000000000000, 0x8000000000000000,
                     0x0000000000000001, 0x7FEFFFFFFFFFFFFF, 0xFFF8000000000123], np.uint64)  # NaN + payload, -inf, +inf, +0, -0, subnormal, largest, -NaN
F32_BITS = np.array([0x7FC12345, 0xFF800000, 0x7F800000, 0x00000000, 0x80000000, 0x00000001, 0x7F7FFFFF, 0xFFC00123], np.uint32)
EP_RETURNS = np.array([-(1 << 31), (1 << 31) - 1, -1, 0x0000FFFF, 0x00010000, 0x7FFF8000], np.int64)


def _patterns(name, n):
    """(label, value) for every pattern the field is written with: value has the field's dtype, [n] or [count, n]."""
    dt, count = R.FIELD_DTYPE[name], R.FIELD_COUNT[name]
    e = np.arange(n)
    idx = e if count == 1 else e[None, :] + 3 * np.arange(count)[:, None]  # differs per lane AND per slot
    shape = idx.shape
    const = lambda v: np.full(shape, v, np.int64).astype(dt)
    out = []
    if name == "stats":
        for r in range(R.NSTAT):
            if r == R.ST_SHIP:
                continue
            v = np.zeros((R.NSTAT, n), np.int64)
            v[r] = R.STAT_MAX[r]
            out.append(("row %d at its maximum" % r, v))
        out.append(("every row at its maximum", np.repeat(R.STAT_MAX[:, None], n, 1)))
        bits = np.log2(R.STAT_MAX + 1).astype(np.int64)
        out.append(("a walking bit", np.int64(1) << ((e[None, :] + np.arange(R.NSTAT)[:, None]) % bits[:, None])))
        out.append(("zero", np.zeros((R.NSTAT, n), np.int64)))
        res = []
        for label, v in out:
            v = v.copy()
            v[R.ST_SHIP] = v[R.ST_BIG] + v[R.ST_SMALL] + v[R.ST_SHELL]
            res.append((label, v.astype(np.int32)))
        return res
    if name == "ep_return":
        out = [("%#x" % (int(v) & 0xFFFFFFFF), const(v)) for v in EP_RETURNS]
        return out + [("one per lane", EP_RETURNS[e % len(EP_RETURNS)].astype(dt))]
    if name in R.BITFIELDS or name == "missile_angle":
        shift, bits, signed = R.BITFIELDS.get(name, (0, R.HEADING_BITS, 0))
        if signed:
            lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
            return [(str(v), const(v)) for v in (lo, hi, -1, 0)] + [("extremes by lane", np.where(idx % 2 == 0, lo, hi).astype(dt))]
        full = (1 << bits) - 1
        return [("zero", const(0)), ("all ones", const(full)), ("alternating by lane", np.where(idx % 2 == 0, full, 0).astype(dt)),
                ("a walking bit", (np.int64(1) << (idx % bits)).astype(dt))]
    if dt.kind == "f":
        table = (F64_BITS if dt.itemsize == 8 else F32_BITS)
        return [("bit patterns, rotation %d" % k, table[(idx + k) % 8].view(dt)) for k in (range(8) if n < 8 else (0, 3))]
    info = np.iinfo(dt)
    vals = [info.min, info.max] + ([-1] if info.min < 0 else [1])
    return [(str(v), const(v)) for v in vals] + [("extremes by lane", np.where(idx % 2 == 0, info.min, info.max).astype(dt))]


def _background_rows(hdr, n, kind):
    rows = np.zeros((n, R.ROW_BYTES), np.uint8)
    if kind == "ones":  # every bit a field can set: not the tile's pool count, not the shell word's four bits of nobody
        rows[:, 16:R.MISSILE_ANG_AT] = 0xFF
        w = rows[:, 96:112].copy().view("<u4")
        w[:, 2] &= 0x000FFFFF
        w[:, 3] &= 0xFF0FFFFF
        rows[:, 96:112] = w.view(np.uint8)
        rows[:, R.MISSILE_ANG_AT:R.PAD_AT] = np.full((n, R.NSLOT), 511, "<u2").view(np.uint8)
    rows[:, :16] = np.asarray(hdr, "<u4").view(np.uint8)
    return rows


# ------------------------------------------------------------------ (a) reads against the codec

# ticks of play after which the batch is where the test wants it (worked out once with the oracle, asserted below on the
# device): the last tile, partial or not, owns a missile, and in youturn games some tile's pool spans more than one row
TICKS = {"youturn": {1: 150, 63: 150, 64: 150, 65: 150, 255: 150, 256: 150, 257: 152, 321: 160},
         "autoturn": {1: 150, 63: 150, 64: 150, 65: 140, 255: 150, 256: 150, 257: 152, 321: 162}}


def _script(n, n_actions):
    """[180, n]: even lanes fire half of the time (many missiles in flight), odd lanes play the hunter (kills, vlner resets)"""
    rng = np.random.default_rng(1000 + n)
    fire = firing_actions(180, n, n_actions, seed=n)
    hunt = open_loop_actions("hunter", (180, n), n_actions, rng, phase=rng.integers(0, 96, n))
    return np.where((np.arange(n) % 2 == 0)[None, :], fire, hunt).astype(np.uint8)


def _played(sfa, gametype, n, **kw):
    env = sfa.SFVecEnv(n, gametype=gametype, spawn_stride=1, **kw)
    acts = torch.from_numpy(_script(n, env.n_actions)).to(env.device)
    T = TICKS[gametype][n]
    env.reset()
    env.rollout(acts[:T].contiguous(), want_obs=False)
    return env, acts, T


def _fields_equal_rows(env, what):
    rows = _rows(env)
    assert R.is_canonical(rows).all(), (what, np.flatnonzero(~R.is_canonical(rows))[:5])
    hdr, dec = R.decode(rows)
    assert np.array_equal(hdr, np.tile(env.lane_state_header(), (env.num_envs, 1)))
    assert list(env.field_names()) == list(R.FIELD_NAMES)
    for name in R.FIELD_NAMES:
        _assert_field(env.get_field(name), dec[name], (what, name))
    return dec


@pytest.mark.parametrize("gametype", ["youturn", "autoturn"])
@pytest.mark.parametrize("n", SIZES)
def test_every_read_equals_the_decoded_rows(sfa, gametype, n):
    env, acts, T = _played(sfa, gametype, n)
    per_env = np.array([bin(int(m)).count("1") for m in env.get_field("missile_mask")])
    pools = np.concatenate([per_env, np.zeros((-n) % 64, int)]).reshape(-1, 64).sum(1)
    print("pools per tile: %s" % pools.tolist())
    assert pools[-1] > 0, "no lane of the last tile owns a missile"
    if gametype == "youturn" and n >= 63:
        assert pools.max() > 64, "the largest pool holds %d entries: one row" % pools.max()
    t = env.get_field("time")
    t[::3] = 34 * 5294  # a third of the lanes one tick from game over
    env.set_field("time", t)
    dec = _fields_equal_rows(env, "after %d ticks" % T)
    assert dec["stats"][R.ST_SHOTS].max() > 0 and (dec["time"][1::3] == 34 * T).all()
    # the device-side read, issued behind a step on the same stream without a synchronise in between
    # (every output a view into a larger buffer of guard bytes: a copy kernel that handles one env too many shows there)
    tdt = {"f8": torch.float64, "f4": torch.float32, "i4": torch.int32, "u4": torch.int32, "i2": torch.int16, "u1": torch.uint8, "i1": torch.int8}
    bufs = {}
    for name in R.FIELD_NAMES:
        if name not in MISSILE_VIEW:
            size = R.FIELD_COUNT[name] * n * R.FIELD_DTYPE[name].itemsize
            buf = torch.full((size + 256,), 0x5A, dtype=torch.uint8, device=env.device)
            bufs[name] = (buf, buf[:size].view(tdt[R.FIELD_DTYPE[name].str[1:]]).view(R.FIELD_COUNT[name], n), size)
    out = env.step_tensors(acts[T])
    for name, (buf, view, size) in bufs.items():
        env.get_field_tensor(name, out=view)
    for name, (buf, view, size) in bufs.items():
        host = env.get_field(name)
        got = view.cpu().numpy().view(host.dtype)
        _assert_field(got[0] if host.ndim == 1 else got, host, ("get_field_tensor", name))
        assert (buf[size:] == 0x5A).all(), ("get_field_tensor wrote behind its output", name)
    assert out[2].cpu().numpy()[::3].all()  # those lanes have started new games
    for name in MISSILE_VIEW:
        with pytest.raises(KeyError):
            env.get_field_tensor(name)
    _fields_equal_rows(env, "after the step that ended a third of the games")
    env.close()


# ------------------------------------------------------------------ (b) a write changes its own bits and nothing else

@pytest.mark.parametrize("background", ["zeros", "ones"])
@pytest.mark.parametrize("n", SIZES)
def test_a_write_changes_its_own_bits_and_nothing_else(sfa, n, background):
    env = sfa.SFVecEnv(n, gametype="youturn")
    hdr = env.lane_state_header()
    base_rows = _background_rows(hdr, n, background)
    _, base = R.decode(base_rows)
    assert np.array_equal(R.encode(hdr, base), base_rows) and R.is_canonical(base_rows).all()
    _load(env, base_rows)
    _assert_rows(_rows(env), base_rows, "the background as loaded")
    writes = 0
    for name in R.FIELD_NAMES:
        cur = base
        for label, value in _patterns(name, n):
            env.set_field(name, value)
            cur = _after_write(cur, name, value)
            _assert_rows(_rows(env), R.encode(hdr, cur), "%s <- %s on %s" % (name, label, background))
            _assert_field(env.get_field(name), cur[name], "%s read back after %s" % (name, label))
            writes += 1
        # back to the background (a slot that comes alive reads (0, 0, 0): the mask takes its view along)
        for k in (MISSILE_ALL if name == "missile_mask" else (name,)):
            env.set_field(k, base[k])
        _assert_rows(_rows(env), base_rows, "the background after the writes to %s" % name)
    print("%d writes checked over %d rows" % (writes, n))
    env.close()


# ------------------------------------------------------------------ (c) rows in, fields out

def _extreme_fields(rng, n, variant):
    """Every packed field at an extreme while its word-neighbours hold the opposite.  Variants 0 / 1: the parts of a word
    alternate all ones / zero, starting with ones / zero; 2: signed parts at their largest (0x7FFF) under neighbours of all
    ones; 3: signed parts at their smallest (0x8000) under neighbours of zero.  Every other field random."""
    f = R.random_fields(rng, n, headings=512)
    stats = f["stats"].astype(np.int64)
    ep = np.zeros(n, np.uint32)
    for parts in R.WORDS.values():
        k = 0
        for owner, shift, bits, signed in parts:
            if owner in ("pool_count", "spare"):
                continue
            ones = (1 << bits) - 1
            if variant < 2:
                raw = ones if (k + variant) % 2 == 0 else 0
            elif signed:
                raw = ones >> 1 if variant == 2 else 1 << (bits - 1)
            else:
                raw = ones if variant == 2 else 0
            k += 1
            if isinstance(owner, str):
                v = raw - (1 << bits) if signed and raw >> (bits - 1) else raw
                f[owner] = np.full(n, v, np.int64).astype(R.FIELD_DTYPE[owner])
            elif owner[0] == "stats":
                stats[owner[1]] = raw
            else:
                ep |= np.uint32(raw << (0 if owner[1] == "lo" else 16))
    stats[R.ST_SHOTS:R.ST_RIGHTS + 1] = np.array({0: [65535, 0, 65535, 0], 1: [0, 65535, 0, 65535], 2: [65535] * 4, 3: [0] * 4}[variant])[:, None]
    stats[R.ST_SHIP] = stats[R.ST_BIG] + stats[R.ST_SMALL] + stats[R.ST_SHELL]
    f["stats"] = stats.astype(np.int32)
    f["ep_return"] = ep.view(np.int32).copy()
    return _after_write(f, "missile_mask", f["missile_mask"])  # (the mask changed: dead slots hold nothing)


@pytest.mark.parametrize("n", SIZES)
def test_rows_in_fields_out(sfa, n):
    rng = np.random.default_rng(40 + n)
    parts = [_extreme_fields(rng, 8, v) for v in range(4)] + [R.random_fields(rng, 32, headings=512)]
    fields = {k: np.concatenate([p[k] for p in parts], axis=-1) for k in R.FIELD_NAMES}
    env = sfa.SFVecEnv(n, gametype="autoturn")
    hdr = env.lane_state_header()
    table = R.encode(hdr, fields)
    assert table.shape[0] == 64 and R.is_canonical(table).all()
    lanes = rng.permutation(n)                   # across tiles
    row_of = np.empty(n, np.int64)
    row_of[lanes] = (7 * np.arange(n) + 3) % 64  # beyond 64 lanes a row is forked into several

    def load(rows):
        half = n // 2
        dev_rows = torch.from_numpy(rows).to(env.device)
        for sl, dt in ((slice(0, half), torch.int32), (slice(half, n), torch.int64)):
            if lanes[sl].size:
                env.load_lanes(dev_rows, lanes=torch.from_numpy(lanes[sl]).to(env.device, dt),
                               rows=torch.from_numpy(row_of[lanes[sl]]).to(env.device, dt))

    def check(what):
        for name in R.FIELD_NAMES:
            _assert_field(env.get_field(name), fields[name][..., row_of], (what, name))
        _assert_rows(_rows(env), table[row_of], what)
        some = lanes[:max(1, n // 3)]
        for dt in (torch.int32, torch.int64):
            _assert_rows(_rows(env, torch.from_numpy(some).to(env.device, dt)), table[row_of[some]], (what, "chosen lanes", dt))

    load(table)
    check("canonical rows")
    # rows that carry a pool count (as if copied out of a tile raw) load as if they carried none, and save canonical
    env.close()
    env = sfa.SFVecEnv(n, gametype="autoturn")
    raw = table.copy()
    w = raw[:, 96:112].copy().view("<u4")
    w[:, 2] |= 0xFFF00000
    raw[:, 96:112] = w.view(np.uint8)
    assert not R.is_canonical(raw).any()
    load(raw)
    check("rows with pool-count bits set")
    env.close()


# ------------------------------------------------------------------ (d) the missile view

def _missile_values(n):
    e, s = np.arange(n)[None, :], np.arange(R.NSLOT)[:, None]
    return {"missile_x": 1000.0 * e + s + 0.25, "missile_y": -(1000.0 * e + s) - 0.5,
            "missile_angle": ((7 * e + 13 * s) % 360).astype(np.int16)}


def _shapes(n, rng):
    last = 64 * ((n - 1) // 64)
    one = np.zeros(n, np.uint32)
    one[min(63, n - 1)] = 1 << 19
    tail = np.zeros(n, np.uint32)
    tail[last:] = rng.integers(1, 1 << 20, n - last)
    return (("empty pools", np.zeros(n, np.uint32)), ("one missile, lane %d slot 19" % min(63, n - 1), one),
            ("every slot of every lane", np.full(n, 0xFFFFF, np.uint32)), ("the last tile alone", tail),
            ("random", rng.integers(0, 1 << 20, n).astype(np.uint32)))


ORDERS = (("missile_mask", "missile_x", "missile_y", "missile_angle"), ("missile_x", "missile_y", "missile_angle", "missile_mask"),
          ("missile_x", "missile_mask", "missile_y", "missile_angle"), ("missile_angle", "missile_y", "missile_mask", "missile_x"))


@pytest.mark.parametrize("n", SIZES)
def test_the_missile_view_in_every_order_of_writes(sfa, n):
    rng = np.random.default_rng(60 + n)
    env = sfa.SFVecEnv(n, gametype="youturn")
    hdr = env.lane_state_header()
    _, fresh = R.decode(_rows(env))
    assert not fresh["missile_mask"].any()
    values = _missile_values(n)
    for what, mask in _shapes(n, rng):
        want = _after_write(dict(fresh, **values), "missile_mask", mask)
        want_rows = R.encode(hdr, want)
        for order in ORDERS:
            env.set_field("missile_mask", np.zeros(n, np.uint32))
            _assert_rows(_rows(env), R.encode(hdr, fresh), (what, "cleared"))
            for k in order:
                env.set_field(k, mask if k == "missile_mask" else values[k])
            _assert_rows(_rows(env), want_rows, (what, order))  # (values written to dead slots are gone)
            for k in MISSILE_ALL:
                _assert_field(env.get_field(k), want[k], (what, order, k))
        # a slot that comes alive without ever being written reads (0, 0, 0)
        more = (mask | rng.integers(0, 1 << 20, n).astype(np.uint32)).astype(np.uint32)
        env.set_field("missile_mask", more)
        grown = dict(want, missile_mask=more)
        _assert_rows(_rows(env), R.encode(hdr, grown), (what, "slots come alive"))
        for k in MISSILE_ALL:
            _assert_field(env.get_field(k), grown[k], (what, "slots come alive", k))
    env.close()


# ------------------------------------------------------------------ (e) every reader sees an edited view

def _edit(env, seed, order):
    rng = np.random.default_rng(seed)
    n = env.num_envs
    vals = {"missile_mask": (rng.integers(0, 1 << 20, n) & rng.integers(0, 1 << 20, n)).astype(np.uint32),  # a quarter alive
            "missile_x": rng.uniform(60, 650, (R.NSLOT, n)), "missile_y": rng.uniform(60, 560, (R.NSLOT, n)),
            "missile_angle": rng.integers(0, 360, (R.NSLOT, n)).astype(np.int16)}
    for k in order:
        env.set_field(k, vals[k])


def _bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype != torch.uint8 else t


@pytest.mark.parametrize("n", SIZES)
def test_every_reader_sees_an_edited_view(sfa, n):
    """Twin batches, the same missile edits.  In A the edit is followed directly by the reader, in B by save_lanes (a flush
    point that parts (b) and (d) pin) and then the reader: the same rows afterwards, the same output."""
    from test_gpu_image import _live_record_bytes

    A, _, T = _played(sfa, "youturn", n)
    B, acts, _ = _played(sfa, "youturn", n)
    D, _, _ = _played(sfa, "youturn", n)             # a source of lanes nobody edits
    CA, CB = (sfa.SFVecEnv(n, gametype="youturn", spawn_stride=1) for _ in range(2))  # destinations
    _assert_rows(_rows(A), _rows(B), "the twins before any edit")
    rng = np.random.default_rng(80 + n)
    k = max(1, n // 2)
    dst = torch.from_numpy(rng.permutation(n)[:k]).to(A.device)
    src = torch.from_numpy(rng.permutation(n)[:k]).to(A.device)
    marked = torch.from_numpy((rng.random(n) < 0.4).astype(np.uint8)).to(A.device)
    marked[n - 1] = 1
    nobody = torch.zeros(n, dtype=torch.uint8, device=A.device)

    def masked_reset(mask):
        def f(E, other):
            out = torch.zeros((n, E.obs_dim), dtype=E.obs_dtype, device=E.device)
            E.reset_lanes(mask=mask, out=out)
            return [out]
        return f

    def step(E, other):
        return [x.clone() for x in E.step_tensors(acts[T])]

    def copy_from(E, other):
        other.copy_lanes(dst, src, src=E)
        return [other.save_lanes().rows]

    def copy_into(E, other):
        E.copy_lanes(dst, src, src=D)
        return []

    def records(E, other):
        return [torch.from_numpy(_live_record_bytes(E.draw_records(from_state=True)))]

    def mask_tensor(E, other):
        return [E.get_field_tensor("missile_mask")]

    readers = (("step", step), ("reset_lanes, no lane marked", masked_reset(nobody)), ("reset_lanes, some lanes marked", masked_reset(marked)),
               ("copy_lanes from the edited batch", copy_from), ("copy_lanes into the edited batch", copy_into),
               ("draw_records(from_state=1)", records), ("get_field_tensor(missile_mask)", mask_tensor))
    for i, (what, reader) in enumerate(readers):
        for E in (A, B):
            _edit(E, 1000 * n + i, ORDERS[i % len(ORDERS)])
        out_a = reader(A, CA)
        B.save_lanes()
        out_b = reader(B, CB)
        _assert_rows(_rows(A), _rows(B), what)
        assert len(out_a) == len(out_b)
        for j, (x, y) in enumerate(zip(out_a, out_b)):
            assert torch.equal(_bits(x.cpu()), _bits(y.cpu())), (what, "output %d" % j)
    # sf_reset after an edit: new games everywhere, no missile anywhere, and nothing of the edit comes back later
    _edit(A, 7, ORDERS[1])
    A.reset()
    B.reset()
    rows = _rows(A)
    _assert_rows(rows, _rows(B), "reset after an edit")
    _, dec = R.decode(rows)
    assert not any(dec[k].any() for k in MISSILE_ALL)
    for t in range(3):
        A.step_tensors(acts[t])
        B.step_tensors(acts[t])
    _assert_rows(_rows(A), _rows(B), "three ticks after the reset")
    for E in (A, B, D, CA, CB):
        E.close()


# ------------------------------------------------------------------ (f) one tick at the edges, against the oracle

def test_one_tick_at_the_edges_of_the_packed_words(sfa, oracle_mod):
    """Key timers two NOOP ticks above -32768 (lanes 0 mod 4), `time` two ticks below 2^24 (lanes 1 mod 4), both (2 mod 4),
    neither (3 mod 4); in every other group of four the word-neighbours -- resets, missed, both halves of ep_return, shell deaths --
    sit at their maxima, else at zero.  One tick on, nothing is flagged and every lane is the oracle's; after the third tick
    the batch is flagged and every lane that was not pushed over still is the oracle's."""
    from lockstep import load_both

    O = oracle_mod
    L = O.oracle_lib()
    n = 128
    lane = np.arange(n)
    timers, clock = (lane % 4 == 0) | (lane % 4 == 2), (lane % 4 == 1) | (lane % 4 == 2)
    maxed = (lane // 4) % 2 == 0
    base = O.OracleVecEnv("youturn", n).snapshots()
    for k in ("fire_timer", "thrust_timer", "left_timer", "right_timer"):
        base[k][timers] = -32766
    ticks = (1 << 24) // 34 + 1 - 2  # the second tick from here reaches 2^24 ms
    base["time"][clock] = 34 * ticks
    base["tick"][clock] = ticks
    assert 34 * (ticks + 1) < (1 << 24) <= 34 * (ticks + 2)
    base["stats"][maxed, R.ST_RESETS] = 65535
    base["stats"][maxed, R.ST_MISSED] = 65535
    base["stats"][maxed, R.ST_SHELL] = 255
    base["stats"][:, R.ST_SHIP] = base["stats"][:, :3].sum(1)
    env, orc = load_both(sfa, O, "youturn", base, auto_reset=False)
    ep = np.where(maxed, -1, 0).astype(np.int32)
    env.set_field("ep_return", ep)
    noop = torch.zeros(n, dtype=torch.uint8, device=env.device)

    def tick():
        rew = env.step_tensors(noop)[1].cpu().numpy()
        obs = np.empty(orc.obs_dim, np.float64)
        r, d, i = C.c_int(), C.c_int(), C.c_int()
        want = np.empty(n, np.int32)
        for e in range(n):  # the bare env's step: the oracle's vec env would start a new game where the clock says game over
            assert L.sfo_env_step(L.sfo_vec_env_at(orc.h, e), 0, obs.ctypes.data_as(C.c_void_p), C.byref(r), C.byref(d), C.byref(i)) == 0
            want[e] = r.value
        assert np.array_equal(rew, want)
        return rew

    ep = ep + tick()  # (int32 arithmetic: -1 + 0 stays -1)
    env.check_state()
    sd = env.state_dict()
    bad = compare_state(sd, orc.snapshots())
    assert not bad, bad
    assert np.array_equal(sd["ep_return"], ep)
    assert (sd["fire_timer"][timers] == -32767).all() and (sd["time"][clock] == 34 * (ticks + 1)).all()
    rows = _rows(env)
    assert R.is_canonical(rows).all()
    for name, v in R.decode(rows)[1].items():
        _assert_field(sd[name], v, ("one tick on", name))
    ep = ep + tick()
    ep = ep + tick()
    with pytest.raises(OverflowError):
        env.check_state()
    ok = np.flatnonzero(~(timers | clock))
    sd = env.state_dict()
    bad = compare_state(sd, orc.snapshots()[ok], lanes=ok)
    assert not bad, bad
    assert np.array_equal(sd["ep_return"][ok], ep[ok])
    assert (sd["stats"][R.ST_RESETS][ok] == np.where(maxed, 65535, 0)[ok]).all()
    env.close()
