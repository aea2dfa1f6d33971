"""A lane-state row in plain numpy: the reference every state accessor and the row kernels are held to.

Written from two documents and from nothing else: the lane-state block of include/sfmi.h (which bytes of the 1136 hold
what) and the packed-word table of spacefortress_amd/csrc/sf_layout.h (which bits of a 32-bit word hold what).  It shares no
code with sf_get_field / sf_set_field, the slot view of the missile pools or the save / load kernels, and it does not read
the header: tests/test_lane_row_model.py pins it with words worked out by hand and ties it to the header's tables through a
small native program, so that a change of the layout shows up as a disagreement and not as a silent re-derivation.

A row (little endian):
    0    .. 15    header, four uint32: magic | version, preset, seed, spawn table length
    16   .. 127   seven 16-byte chunks: ship_pos, ship_vel, timers_a, timers_b, score, misc, small
    128  .. 767   shells: 20 x (x, y), then 20 x (vx, vy), doubles
    768  .. 1087  missiles by slot, 20 x (x, y), doubles; zero where the slot holds none
    1088 .. 1127  their headings, uint16 [20]
    1128 .. 1135  zeros

decode() gives the fields under the names, dtypes and shapes of SFVecEnv.state_dict(): [n], or [count, n] slot-major.
encode() gives CANONICAL rows: the pool-count bits of the missile word zero (the count belongs to the tile, not to the lane),
the eight trailing bytes zero, dead missile slots zero -- and the four bits of the shell word that no field owns (20 .. 23,
between the alive mask and ep_kills) zero as well: the table gives them to nobody, so no field can say what they hold.
"""
import numpy as np

ROW_BYTES = 1136
NSLOT = 20
NSTAT = 13
MAGIC = 0x53464C00
VERSION = 1

# the seven chunks, in row order, and the byte at which each starts
CHUNKS = ("ship_pos", "ship_vel", "timers_a", "timers_b", "score", "misc", "small")
CHUNK_AT = {name: 16 + 16 * i for i, name in enumerate(CHUNKS)}
SHELL_POS_AT, SHELL_VEL_AT, MISSILE_POS_AT, MISSILE_ANG_AT, PAD_AT = 128, 448, 768, 1088, 1128

# (name, numpy dtype, elements per env, is_float): the order of sf_field_info
FIELDS = (
    ("ship_x", np.float64, 1, 1), ("ship_y", np.float64, 1, 1), ("ship_vx", np.float64, 1, 1), ("ship_vy", np.float64, 1, 1),
    ("missile_x", np.float64, NSLOT, 1), ("missile_y", np.float64, NSLOT, 1),
    ("shell_x", np.float64, NSLOT, 1), ("shell_y", np.float64, NSLOT, 1),
    ("shell_vx", np.float64, NSLOT, 1), ("shell_vy", np.float64, NSLOT, 1),
    ("ship_death_timer", np.int32, 1, 0),
    ("fire_timer", np.int32, 1, 0), ("thrust_timer", np.int32, 1, 0), ("left_timer", np.int32, 1, 0),
    ("right_timer", np.int32, 1, 0),
    ("fort_timer", np.int32, 1, 0), ("fort_death_timer", np.int32, 1, 0), ("fort_vuln_timer", np.int32, 1, 0),
    ("points", np.float32, 1, 1), ("raw_points", np.float32, 1, 1),
    ("vlner", np.int32, 1, 0), ("time", np.int32, 1, 0),
    ("stats", np.int32, NSTAT, 0),
    ("prev_vlner", np.int32, 1, 0),
    ("spawn_cursor", np.uint32, 1, 0), ("missile_mask", np.uint32, 1, 0), ("shell_mask", np.uint32, 1, 0),
    ("ep_return", np.int32, 1, 0), ("ep_kills", np.int32, 1, 0),
    ("ship_angle", np.int16, 1, 0), ("fort_angle", np.int16, 1, 0), ("fort_last_angle", np.int16, 1, 0),
    ("missile_angle", np.int16, NSLOT, 0),
    ("flags", np.uint8, 1, 0), ("last_reward", np.int8, 1, 0),
)
FIELD_NAMES = tuple(f[0] for f in FIELDS)
FIELD_DTYPE = {f[0]: np.dtype(f[1]) for f in FIELDS}
FIELD_COUNT = {f[0]: f[2] for f in FIELDS}

# One element at a fixed byte of a chunk: name -> (chunk, byte in chunk).  (The dtype is the field's.)
PLAIN = {
    "ship_x": ("ship_pos", 0), "ship_y": ("ship_pos", 8), "ship_vx": ("ship_vel", 0), "ship_vy": ("ship_vel", 8),
    "fort_timer": ("timers_b", 4), "fort_death_timer": ("timers_b", 8), "fort_vuln_timer": ("timers_b", 12),
    "points": ("score", 0), "raw_points": ("score", 4),
    "ship_death_timer": ("misc", 0),
    "ship_angle": ("small", 0), "fort_angle": ("small", 2), "fort_last_angle": ("small", 4),
    "flags": ("small", 6), "last_reward": ("small", 7),
}

# stats rows (the reference's order); row 3, ship deaths, is the sum of rows 0 .. 2 and is stored nowhere
ST_BIG, ST_SMALL, ST_SHELL, ST_SHIP, ST_RESETS, ST_DESTROYED, ST_MISSED = 0, 1, 2, 3, 4, 5, 6
ST_SHOTS, ST_THRUSTS, ST_LEFTS, ST_RIGHTS, ST_VLNER_INCS, ST_MAX_VLNER = 7, 8, 9, 10, 11, 12
KEYCOUNT_AT = 8  # small chunk, bytes 8 .. 15: shots, thrusts, lefts, rights as four uint16
STAT_MAX = np.array([255, 255, 255, 765, 65535, 255, 65535, 65535, 65535, 65535, 65535, 4095, 4095], np.int64)

# The packed words: (chunk, byte in chunk) -> parts (owner, shift, bits, signed).  An owner is a field name, ("stats", row),
# ("ep_return", "lo" | "hi"), "pool_count" (the tile's, never the lane's) or "spare" (nobody's).
WORDS = {
    ("timers_a", 0): (("prev_vlner", 0, 12, 0), (("stats", ST_VLNER_INCS), 12, 12, 0), (("stats", ST_BIG), 24, 8, 0)),
    ("timers_a", 4): (("fire_timer", 0, 16, 1), (("stats", ST_RESETS), 16, 16, 0)),
    ("timers_a", 8): (("thrust_timer", 0, 16, 1), (("stats", ST_MISSED), 16, 16, 0)),
    ("timers_a", 12): (("left_timer", 0, 16, 1), (("ep_return", "lo"), 16, 16, 0)),
    ("timers_b", 0): (("right_timer", 0, 16, 1), (("ep_return", "hi"), 16, 16, 0)),
    ("score", 8): (("vlner", 0, 12, 0), (("stats", ST_MAX_VLNER), 12, 12, 0), (("stats", ST_SMALL), 24, 8, 0)),
    ("score", 12): (("time", 0, 24, 0), (("stats", ST_SHELL), 24, 8, 0)),
    ("misc", 4): (("spawn_cursor", 0, 24, 0), (("stats", ST_DESTROYED), 24, 8, 0)),
    ("misc", 8): (("missile_mask", 0, 20, 0), ("pool_count", 20, 12, 0)),
    ("misc", 12): (("shell_mask", 0, 20, 0), ("spare", 20, 4, 0), ("ep_kills", 24, 8, 0)),
}
# field -> (shift, bits, signed) for the fields that are ONE bit field of a word (the table's B(...) rows)
BITFIELDS = {p[0]: (p[1], p[2], p[3]) for parts in WORDS.values() for p in parts if isinstance(p[0], str) and p[0] in FIELD_NAMES}
POOL_COUNT_MASK = np.uint32(0xFFF00000)
SHELL_SPARE_MASK = np.uint32(0x00F00000)
HEADING_BITS = 9  # a pool entry's heading: what sf_set_field("missile_angle") can hold


def header(preset, seed, spawn_table_len, n=1):
    """The header rows of a batch: preset = bit 0 autoturn, bit 1 shaped scoring."""
    return np.tile(np.array([MAGIC | VERSION, preset, seed, spawn_table_len], np.uint32), (n, 1))


def _rows(rows):
    rows = np.ascontiguousarray(rows, np.uint8)
    if rows.ndim != 2 or rows.shape[1] != ROW_BYTES:
        raise ValueError("rows must be uint8 [n, %d]" % ROW_BYTES)
    return rows


def _view(rows, at, dtype, count=1):
    """`count` elements of `dtype` from byte `at` of every row: [n, count]."""
    dt = np.dtype(dtype)
    return np.ascontiguousarray(rows[:, at:at + dt.itemsize * count]).view(dt.newbyteorder("<")).astype(dt)


def _word(rows, chunk, byte):
    return _view(rows, CHUNK_AT[chunk] + byte, np.uint32)[:, 0]


def _bits(word, shift, bits, signed):
    v = (word.astype(np.uint64) >> np.uint64(shift)) & np.uint64((1 << bits) - 1)
    v = v.astype(np.int64)
    if signed:
        v = np.where(v >= (1 << (bits - 1)), v - (1 << bits), v)
    return v


def decode(rows):
    """rows uint8 [n, 1136] -> (header uint32 [n, 4], {field: array}) -- see the module text."""
    rows = _rows(rows)
    n = rows.shape[0]
    hdr = _view(rows, 0, np.uint32, 4)
    f = {}
    for name, (chunk, byte) in PLAIN.items():
        f[name] = _view(rows, CHUNK_AT[chunk] + byte, FIELD_DTYPE[name])[:, 0]
    stats = np.zeros((NSTAT, n), np.int64)
    ep = np.zeros(n, np.uint32)
    for (chunk, byte), parts in WORDS.items():
        w = _word(rows, chunk, byte)
        for owner, shift, bits, signed in parts:
            v = _bits(w, shift, bits, signed)
            if owner in ("pool_count", "spare"):
                continue
            if isinstance(owner, str):
                f[owner] = v.astype(FIELD_DTYPE[owner])
            elif owner[0] == "stats":
                stats[owner[1]] = v
            else:  # ep_return: bits 0 .. 15 above the left timer, bits 16 .. 31 above the right timer
                ep |= (v.astype(np.uint32) << np.uint32(0 if owner[1] == "lo" else 16))
    f["ep_return"] = ep.view(np.int32).copy()
    keys = _view(rows, CHUNK_AT["small"] + KEYCOUNT_AT, np.uint16, 4)
    stats[ST_SHOTS:ST_RIGHTS + 1] = keys.T
    stats[ST_SHIP] = stats[ST_BIG] + stats[ST_SMALL] + stats[ST_SHELL]
    f["stats"] = stats.astype(np.int32)
    sp = _view(rows, SHELL_POS_AT, np.float64, 2 * NSLOT).reshape(n, NSLOT, 2)
    sv = _view(rows, SHELL_VEL_AT, np.float64, 2 * NSLOT).reshape(n, NSLOT, 2)
    mp = _view(rows, MISSILE_POS_AT, np.float64, 2 * NSLOT).reshape(n, NSLOT, 2)
    f["shell_x"], f["shell_y"] = np.ascontiguousarray(sp[:, :, 0].T), np.ascontiguousarray(sp[:, :, 1].T)
    f["shell_vx"], f["shell_vy"] = np.ascontiguousarray(sv[:, :, 0].T), np.ascontiguousarray(sv[:, :, 1].T)
    f["missile_x"], f["missile_y"] = np.ascontiguousarray(mp[:, :, 0].T), np.ascontiguousarray(mp[:, :, 1].T)
    f["missile_angle"] = np.ascontiguousarray(_view(rows, MISSILE_ANG_AT, np.uint16, NSLOT).T).view(np.int16).copy()
    return hdr, {name: f[name] for name in FIELD_NAMES}


def _put(rows, at, values, dtype):
    """values [n] or [n, count] of `dtype` to byte `at` of every row"""
    v = np.ascontiguousarray(np.asarray(values).reshape(rows.shape[0], -1), np.dtype(dtype).newbyteorder("<"))
    rows[:, at:at + v.shape[1] * v.dtype.itemsize] = v.view(np.uint8).reshape(rows.shape[0], -1)


def _field(fields, name, n):
    """the field as the accessor would take it: its own dtype, [count, n], bits kept"""
    a = np.asarray(fields[name])
    dt = FIELD_DTYPE[name]
    if a.dtype != dt:
        same_width_ints = a.dtype.kind in "iu" and dt.kind in "iu" and a.dtype.itemsize == dt.itemsize
        a = np.ascontiguousarray(a).view(dt) if same_width_ints else a.astype(dt)
    return a.reshape(FIELD_COUNT[name], n)


def check_range(fields):
    """ValueError for a value its bit field cannot hold, or a stats row 3 that is not the sum: what encode refuses."""
    for name, (shift, bits, signed) in BITFIELDS.items():
        v = np.asarray(fields[name]).astype(np.int64)
        lo, hi = (-(1 << (bits - 1)), (1 << (bits - 1)) - 1) if signed else (0, (1 << bits) - 1)
        if v.size and (v.min() < lo or v.max() > hi):
            raise ValueError("%s: a value outside [%d, %d]" % (name, lo, hi))
    st = np.asarray(fields["stats"]).astype(np.int64)
    if st.size and ((st < 0).any() or (st > STAT_MAX[:, None]).any()):
        raise ValueError("stats: a value that does not fit its bits")
    if not np.array_equal(st[ST_SHIP], st[ST_BIG] + st[ST_SMALL] + st[ST_SHELL]):
        raise ValueError("stats: row 3 is not the sum of rows 0 .. 2")
    ang = np.asarray(fields["missile_angle"]).astype(np.int64)
    if ang.size and (ang.min() < 0 or ang.max() >= (1 << HEADING_BITS)):
        raise ValueError("missile_angle: a heading outside the 9 bits of a pool entry")


def encode(header, fields):
    """(header uint32 [n, 4] or [4], fields as decode returns them) -> canonical rows uint8 [n, 1136]."""
    n = np.asarray(fields["ship_x"]).reshape(-1).shape[0]
    check_range(fields)
    rows = np.zeros((n, ROW_BYTES), np.uint8)
    _put(rows, 0, np.broadcast_to(np.asarray(header, np.uint32).reshape(-1, 4), (n, 4)), np.uint32)
    for name, (chunk, byte) in PLAIN.items():
        _put(rows, CHUNK_AT[chunk] + byte, _field(fields, name, n)[0], FIELD_DTYPE[name])
    stats = _field(fields, "stats", n).astype(np.int64)
    ep = _field(fields, "ep_return", n)[0].view(np.uint32)
    for (chunk, byte), parts in WORDS.items():
        w = np.zeros(n, np.uint64)
        for owner, shift, bits, signed in parts:
            if owner in ("pool_count", "spare"):
                continue
            if isinstance(owner, str):
                v = _field(fields, owner, n)[0].astype(np.int64)
            elif owner[0] == "stats":
                v = stats[owner[1]]
            else:
                v = (ep >> np.uint32(0 if owner[1] == "lo" else 16)).astype(np.int64)
            w |= (v.astype(np.uint64) & np.uint64((1 << bits) - 1)) << np.uint64(shift)
        _put(rows, CHUNK_AT[chunk] + byte, w.astype(np.uint32), np.uint32)
    _put(rows, CHUNK_AT["small"] + KEYCOUNT_AT, stats[ST_SHOTS:ST_RIGHTS + 1].T.astype(np.uint16), np.uint16)
    pair = lambda x, y: np.stack([_field(fields, x, n).T, _field(fields, y, n).T], axis=2).reshape(n, 2 * NSLOT)
    _put(rows, SHELL_POS_AT, pair("shell_x", "shell_y"), np.float64)
    _put(rows, SHELL_VEL_AT, pair("shell_vx", "shell_vy"), np.float64)
    alive = ((_field(fields, "missile_mask", n)[0][:, None] >> np.arange(NSLOT, dtype=np.uint32)[None, :]) & 1).astype(bool)  # [n, slot]
    mp = pair("missile_x", "missile_y").view(np.uint64).reshape(n, NSLOT, 2).copy()  # (as bits: a NaN's payload is data)
    mp[~alive] = 0
    _put(rows, MISSILE_POS_AT, mp.reshape(n, 2 * NSLOT), np.uint64)
    ang = _field(fields, "missile_angle", n).T.view(np.uint16).copy()
    ang[~alive] = 0
    _put(rows, MISSILE_ANG_AT, ang, np.uint16)
    return rows


def is_canonical(rows):
    """[n] bool: pool-count bits zero, trailing pad zero, dead missile slots zero (and the shell word's four spare bits)."""
    rows = _rows(rows)
    n = rows.shape[0]
    mw, sw = _word(rows, "misc", 8), _word(rows, "misc", 12)
    alive = ((mw[:, None] >> np.arange(NSLOT, dtype=np.uint32)[None, :]) & 1).astype(bool)
    mp = _view(rows, MISSILE_POS_AT, np.uint64, 2 * NSLOT).reshape(n, NSLOT, 2)
    ang = _view(rows, MISSILE_ANG_AT, np.uint16, NSLOT)
    dead_zero = ~((mp.any(axis=2) | (ang != 0)) & ~alive).any(axis=1)
    return ((mw & POOL_COUNT_MASK) == 0) & ((sw & SHELL_SPARE_MASK) == 0) & ~rows[:, PAD_AT:].any(axis=1) & dead_zero


def random_fields(rng, n, headings=360):
    """In-range values for every field, the whole width of each (floats: finite numbers of every magnitude)."""
    f = {}
    for name, dt, count, isf in FIELDS:
        dt = np.dtype(dt)
        shape = (n,) if count == 1 else (count, n)
        if isf:
            f[name] = (rng.standard_normal(shape) * 10.0 ** rng.integers(-3, 6, shape)).astype(dt)
        else:
            info = np.iinfo(dt)
            f[name] = rng.integers(info.min, int(info.max) + 1, shape, dtype=np.int64).astype(dt)
    for name, (shift, bits, signed) in BITFIELDS.items():
        lo, hi = (-(1 << (bits - 1)), 1 << (bits - 1)) if signed else (0, 1 << bits)
        f[name] = rng.integers(lo, hi, n, dtype=np.int64).astype(FIELD_DTYPE[name])
    st = rng.integers(0, STAT_MAX[:, None] + 1, (NSTAT, n), dtype=np.int64)
    st[ST_SHIP] = st[ST_BIG] + st[ST_SMALL] + st[ST_SHELL]
    f["stats"] = st.astype(np.int32)
    alive = ((f["missile_mask"][None, :] >> np.arange(NSLOT, dtype=np.uint32)[:, None]) & 1).astype(bool)  # [slot, n]
    f["missile_angle"] = np.where(alive, rng.integers(0, headings, (NSLOT, n)), 0).astype(np.int16)
    f["missile_x"] = np.where(alive, f["missile_x"], 0.0)
    f["missile_y"] = np.where(alive, f["missile_y"], 0.0)
    return f


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype.itemsize == b.dtype.itemsize and a.tobytes() == b.tobytes()
