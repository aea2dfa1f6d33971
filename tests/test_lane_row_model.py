"""The numpy row codec (tests/lanerow_np.py) against itself, against words worked out by hand from the packed-word table of
sf_layout.h and the byte ranges of sfmi.h, and against the library's own field table.  No GPU: tests/test_gpu_state_access.py
then holds every state accessor and the row kernels to this codec."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import lanerow_np as R
from conftest import ROOT


def _canonicalize(rows):
    n = rows.shape[0]
    w = rows[:, 96:112].view("<u4")   # the misc chunk
    w[:, 2] &= 0x000FFFFF             # the tile's pool count
    w[:, 3] &= 0xFF0FFFFF             # the four bits nobody owns
    rows[:, 1128:] = 0
    alive = ((w[:, 2][:, None] >> np.arange(20, dtype=np.uint32)[None, :]) & 1).astype(bool)
    rows[:, 768:1088].view("<u8").reshape(n, 20, 2)[~alive] = 0
    ang = rows[:, 1088:1128].view("<u2")
    ang &= 511                        # a pool entry's heading has nine bits
    ang[~alive] = 0
    return rows


def _canonical_random_rows(rng, n):
    """Random bytes everywhere a lane owns them (NaNs, infinities and subnormals among the doubles), made canonical."""
    return _canonicalize(rng.integers(0, 256, (n, R.ROW_BYTES), dtype=np.uint8))


def test_rows_survive_decode_then_encode():
    rng = np.random.default_rng(1)
    rows = _canonical_random_rows(rng, 600)
    assert R.is_canonical(rows).all()
    hdr, f = R.decode(rows)
    assert list(f) == list(R.FIELD_NAMES)
    for name, dt, count, _ in R.FIELDS:
        assert f[name].dtype == np.dtype(dt) and f[name].shape == ((600,) if count == 1 else (count, 600)), name
    back = R.encode(hdr, f)
    assert back.dtype == np.uint8 and back.shape == rows.shape
    bad = np.argwhere(back != rows)
    assert bad.size == 0, bad[:8].tolist()


def test_fields_survive_encode_then_decode():
    rng = np.random.default_rng(2)
    f = R.random_fields(rng, 500, headings=512)
    hdr = R.header(3, 12345, 65536, 500)
    rows = R.encode(hdr, f)
    assert R.is_canonical(rows).all()
    hdr2, g = R.decode(rows)
    assert np.array_equal(hdr, hdr2)
    for name in R.FIELD_NAMES:
        assert R.same_bits(f[name], g[name]) and f[name].dtype == g[name].dtype, name
    # one header for all rows
    assert np.array_equal(R.encode(hdr[0], f), rows)


def _hand_row():
    """One row written byte by byte at the offsets sfmi.h documents, its packed words as literals."""
    row = bytearray(R.ROW_BYTES)
    struct.pack_into("<4I", row, 0, 0x53464C01, 2, 7, 131072)
    struct.pack_into("<4d", row, 16, 355.25, -1.5, 0.125, -0.0)                             # ship_pos, ship_vel
    struct.pack_into("<4I", row, 48, 0xAB123456, 0xBEEF8001, 0x00017FFF, 0x5678FFFE)        # timers_a
    struct.pack_into("<I3i", row, 64, 0x9ABC0003, 1000, -7, 250)                            # timers_b
    struct.pack_into("<2f2I", row, 80, 1.5, -0.05, 0x7FFFF001, 0x80FFFFFE)                  # score
    struct.pack_into("<i3I", row, 96, -1000, 0x01800000, 0xFFF80001, 0xC3F55555)            # misc
    struct.pack_into("<3hBb4H", row, 112, 359, -1, -32768, 0xFF, -100, 0x0102, 0xFFFF, 0, 0x8000)  # small
    for s in range(20):
        struct.pack_into("<2d", row, 128 + 16 * s, 100.0 + s, 200.0 + s)                    # shell (x, y)
        struct.pack_into("<2d", row, 448 + 16 * s, 0.5 * s, -0.25 * s)                      # shell (vx, vy)
        struct.pack_into("<2d", row, 768 + 16 * s, 300.0 + s, 400.0 + s)                    # missile (x, y)
        struct.pack_into("<H", row, 1088 + 2 * s, 17 * s)                                   # heading
    return np.frombuffer(bytes(row), np.uint8).reshape(1, -1).copy()


def test_known_answers_worked_out_by_hand():
    row = _hand_row()
    hdr, f = R.decode(row)
    assert hdr.tolist() == [[0x53464C01, 2, 7, 131072]]
    one = lambda name: f[name][0].item()
    # timers_a.0 = 0xAB123456: prev_vlner 12 | vlner_incs 12 << 12 | big-hex deaths 8 << 24
    assert one("prev_vlner") == 0x456 and f["stats"][11, 0] == 0x123 and f["stats"][0, 0] == 0xAB
    # timers_a.4 = 0xBEEF8001: fire timer int16 | resets << 16
    assert one("fire_timer") == -32767 and f["stats"][4, 0] == 0xBEEF
    # timers_a.8 = 0x00017FFF: thrust timer | missed << 16
    assert one("thrust_timer") == 32767 and f["stats"][6, 0] == 1
    # timers_a.12 = 0x5678FFFE, timers_b.0 = 0x9ABC0003: left / right timers; ep_return = 0x9ABC5678 from halves that differ
    assert one("left_timer") == -2 and one("right_timer") == 3
    assert one("ep_return") == -0x6543A988 and (one("ep_return") & 0xFFFFFFFF) == 0x9ABC5678
    assert (one("fort_timer"), one("fort_death_timer"), one("fort_vuln_timer")) == (1000, -7, 250)
    # score.8 = 0x7FFFF001: vlner 12 | max_vlner 12 << 12 | small-hex deaths 8 << 24
    assert one("vlner") == 1 and f["stats"][12, 0] == 0xFFF and f["stats"][1, 0] == 0x7F
    # score.12 = 0x80FFFFFE: time 24 | shell deaths 8 << 24
    assert one("time") == 0xFFFFFE and f["stats"][2, 0] == 0x80
    assert f["stats"][3, 0] == 0xAB + 0x7F + 0x80  # ship deaths: the sum, stored nowhere
    # misc.4 = 0x01800000: spawn cursor 24 | destroyed 8 << 24
    assert one("spawn_cursor") == 0x800000 and f["stats"][5, 0] == 1
    # misc.8 = 0xFFF80001: missile mask 20; the twelve bits above are the tile's pool count, no field
    assert one("missile_mask") == 0x80001
    # misc.12 = 0xC3F55555: shell mask 20, four bits of nobody, ep_kills 8 << 24
    assert one("shell_mask") == 0x55555 and one("ep_kills") == 0xC3
    assert one("ship_death_timer") == -1000
    assert (one("ship_angle"), one("fort_angle"), one("fort_last_angle"), one("flags"), one("last_reward")) == (359, -1, -32768, 255, -100)
    assert f["stats"][7:11, 0].tolist() == [0x0102, 0xFFFF, 0, 0x8000]  # shots, thrusts, lefts, rights
    assert np.float32(one("points")) == np.float32(1.5) and np.float32(one("raw_points")) == np.float32(-0.05)
    assert (one("ship_x"), one("ship_y"), one("ship_vx")) == (355.25, -1.5, 0.125) and np.signbit(f["ship_vy"][0]) and one("ship_vy") == 0
    s = np.arange(20)
    assert np.array_equal(f["shell_x"][:, 0], 100.0 + s) and np.array_equal(f["shell_y"][:, 0], 200.0 + s)
    assert np.array_equal(f["shell_vx"][:, 0], 0.5 * s) and np.array_equal(f["shell_vy"][:, 0], -0.25 * s)
    assert np.array_equal(f["missile_x"][:, 0], 300.0 + s) and np.array_equal(f["missile_y"][:, 0], 400.0 + s)
    assert np.array_equal(f["missile_angle"][:, 0], 17 * s)
    # the row is not canonical (pool count, spare bits, missiles in dead slots); its canonical form keeps slots 0 and 19
    assert not R.is_canonical(row)[0]
    canon = R.encode(hdr, f)
    assert R.is_canonical(canon)[0]
    w = canon[0, 96:112].view("<u4")
    assert w[2] == 0x00080001 and w[3] == 0xC3055555
    mp = canon[0, 768:1088].view("<f8").reshape(20, 2)
    assert mp[0].tolist() == [300.0, 400.0] and mp[19].tolist() == [319.0, 419.0] and not mp[1:19].any()
    assert canon[0, 1088:1128].view("<u2").tolist() == [0] * 19 + [323]
    keep = np.ones(R.ROW_BYTES, bool)
    keep[96 + 8:96 + 16] = False
    keep[768:1128] = False
    assert np.array_equal(canon[0, keep], row[0, keep])  # every other byte as written


def test_each_way_of_not_being_canonical_is_seen():
    rows = _canonical_random_rows(np.random.default_rng(3), 5)
    rows[:, 96 + 8] &= 0xFE  # slot 0 dead everywhere
    rows = _canonicalize(rows)
    assert R.is_canonical(rows).all()
    a = rows.copy()
    a[0, 96 + 11] |= 0x10      # a pool-count bit
    a[1, 1135] = 1             # the last pad byte
    a[2, 768 + 15] = 0x80      # the sign bit of a dead slot's y
    a[3, 1088] = 1             # a dead slot's heading
    a[4, 96 + 14] |= 0x10      # a spare bit of the shell word
    assert not R.is_canonical(a).any()


def test_bit_ranges_of_every_packed_word_are_disjoint_and_complete():
    owners = []
    for key, parts in R.WORDS.items():
        seen = 0
        for owner, shift, bits, signed in parts:
            m = ((1 << bits) - 1) << shift
            assert m < (1 << 32) and not (seen & m), (key, owner)
            seen |= m
            owners.append((key, owner, shift, bits))
        assert seen == 0xFFFFFFFF, (key, hex(seen))  # with the tile's pool count and the shell word's four bits of nobody
    assert [(k, s, b) for k, o, s, b in owners if o == "pool_count"] == [(("misc", 8), 20, 12)]
    assert [(k, s, b) for k, o, s, b in owners if o == "spare"] == [(("misc", 12), 20, 4)]
    # every stats row but the sum has exactly one home: nine bit fields and the four uint16 key counters
    rows = sorted(o[1] for k, o, s, b in owners if isinstance(o, tuple) and o[0] == "stats")
    assert rows == [0, 1, 2, 4, 5, 6, 11, 12]
    assert sorted(rows + [3] + list(range(R.ST_SHOTS, R.ST_RIGHTS + 1))) == list(range(R.NSTAT))
    # and the widths are the maxima sf_check_state's text names
    for k, o, s, b in owners:
        if isinstance(o, tuple) and o[0] == "stats":
            assert (1 << b) - 1 == R.STAT_MAX[o[1]], o
    # the plain fields and the packed words share no byte of the seven chunks, and together they fill them
    used = np.zeros(16 + 7 * 16, int)
    for name, (chunk, byte) in R.PLAIN.items():
        used[R.CHUNK_AT[chunk] + byte:R.CHUNK_AT[chunk] + byte + R.FIELD_DTYPE[name].itemsize] += 1
    for chunk, byte in R.WORDS:
        used[R.CHUNK_AT[chunk] + byte:R.CHUNK_AT[chunk] + byte + 4] += 1
    used[R.CHUNK_AT["small"] + R.KEYCOUNT_AT:R.CHUNK_AT["small"] + 16] += 1
    assert (used[16:] == 1).all(), np.flatnonzero(used[16:] != 1) + 16


def test_encode_refuses_what_a_field_cannot_hold():
    f = R.random_fields(np.random.default_rng(4), 4)
    hdr = R.header(0, 1, 65536)
    for name, bad in (("vlner", 4096), ("prev_vlner", -1), ("fire_timer", 32768), ("right_timer", -32769), ("time", 1 << 24),
                      ("ep_kills", 256), ("missile_mask", 1 << 20), ("shell_mask", 1 << 20), ("spawn_cursor", 1 << 24)):
        g = dict(f)
        g[name] = f[name].astype(np.int64)
        g[name][2] = bad
        with pytest.raises(ValueError):
            R.encode(hdr, g)
    for row, bad in ((0, 256), (4, 65536), (11, 4096), (7, -1)):
        g = dict(f)
        g["stats"] = f["stats"].copy()
        g["stats"][row, 1] = bad
        g["stats"][3] = g["stats"][:3].sum(0)
        with pytest.raises(ValueError):
            R.encode(hdr, g)
    g = dict(f)
    g["stats"] = f["stats"].copy()
    g["stats"][3, 0] += 1
    with pytest.raises(ValueError):
        R.encode(hdr, g)
    for bad in (-1, 512):
        g = dict(f)
        g["missile_angle"] = f["missile_angle"].copy()
        g["missile_angle"][5, 3] = bad
        with pytest.raises(ValueError):
            R.encode(hdr, g)


def test_the_field_list_is_the_librarys():
    """sf_n_fields / sf_field_info (host only): name, element size, count and float flag, in the library's order."""
    from spacefortress_amd import build as sfbuild
    from spacefortress_amd import _lib

    sfbuild.build()
    L = _lib.lib()
    d = _lib.FieldDesc()
    got = []
    for i in range(L.sf_n_fields()):
        assert L.sf_field_info(i, C.byref(d)) == 0
        got.append((d.name.decode(), d.elem_size, d.count, d.is_float))
    assert len(got) == len(R.FIELDS) == 35
    assert got == [(name, np.dtype(dt).itemsize, count, isf) for name, dt, count, isf in R.FIELDS]
    assert L.sf_lane_state_bytes() == R.ROW_BYTES
    assert (_lib.LANE_STATE_MAGIC, _lib.LANE_STATE_VERSION) == (R.MAGIC, R.VERSION)


def test_the_model_follows_the_layout_header(tmp_path):
    """Drift guard: sf_layout.h's own tables, printed by a native program, against the codec's.  The hand-made words above pin
    the meaning; this ties model, header and comment together when the layout changes."""
    exe = str(tmp_path / "layout_dump")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "spacefortress_amd", "csrc"),
                           os.path.join(ROOT, "tests", "native", "layout_dump.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    rec = [line.split() for line in out.stdout.splitlines()]
    groups = [(r[1], int(r[2]), int(r[3]), int(r[4])) for r in rec if r[0] == "group"]
    fields = [(r[1], int(r[2]), int(r[3]), int(r[4]), r[5], int(r[6]), int(r[7])) for r in rec if r[0] == "field"]
    bits = {r[1]: (int(r[2]), int(r[3]), int(r[4])) for r in rec if r[0] == "bits"}
    const = {r[1]: int(r[2]) for r in rec if r[0] == "const"}
    PLAIN_K, BITS_K, STATS_K, EPRET_K, MPOOL_K = range(5)
    # the row's chunks are the first seven groups, one 16-byte chunk per lane each, 1 KiB apart in a tile
    assert [g[0] for g in groups[:7]] == list(R.CHUNKS)
    assert all(g[1:] == (16, 1, 1024 * i) for i, g in enumerate(groups[:7]))
    by_name = {g[0]: g for g in groups}
    assert by_name["shell_pos"][1:3] == (16, 20) and by_name["shell_vel"][1:3] == (16, 20)
    assert by_name["missile_pos"][1:3] == (16, 20) and by_name["missile_meta"][1:3] == (4, 20)
    assert [(f[0], f[1], f[2], f[3]) for f in fields] == [(n, np.dtype(dt).itemsize, c, isf) for n, dt, c, isf in R.FIELDS]
    # where every field lives
    assert bits == R.BITFIELDS
    for name, size, count, isf, group, byte, kind in fields:
        if kind == PLAIN_K and count == 1:
            assert R.PLAIN[name] == (group, byte), name
        elif kind == PLAIN_K:
            assert (group, byte) == {"shell_x": ("shell_pos", 0), "shell_y": ("shell_pos", 8), "shell_vx": ("shell_vel", 0),
                                     "shell_vy": ("shell_vel", 8)}[name]
        elif kind == BITS_K:
            parts = {p[0]: p[1:] for p in R.WORDS[(group, byte)]}
            assert parts[name] == bits[name], name
        elif kind == STATS_K:
            assert name == "stats" and count == R.NSTAT
        elif kind == EPRET_K:
            assert name == "ep_return" and (group, byte) == ("timers_a", 12)  # the low half's word
        else:
            assert kind == MPOOL_K and name in ("missile_x", "missile_y", "missile_angle") and count == R.NSLOT
    assert sorted(f[0] for f in fields if f[6] == PLAIN_K and f[2] == 1) == sorted(R.PLAIN)
    assert const["nslot"] == R.NSLOT and const["nstat"] == R.NSTAT and const["keycount_byte"] == R.KEYCOUNT_AT
    assert (const["key_first"], const["key_count"]) == (R.ST_SHOTS, R.ST_RIGHTS - R.ST_SHOTS + 1)
    assert const["mask_bits"] == 20 and const["mask_low"] == 0xFFFFF and const["mpool_shift"] == 20 and const["kills_shift"] == 24
    assert const["mm_angle_max"] == (1 << R.HEADING_BITS) - 1
    # a lane's share of a tile: the seven chunks, 40 shell pieces, 20 pool positions and 20 meta words = the row less its
    # header and the 8 + 40 bytes by which uint16 headings and padding differ from 4-byte meta words
    assert const["bytes_per_lane"] == 7 * 16 + 40 * 16 + 20 * 16 + 20 * 4 == R.ROW_BYTES - 16 - 8 + 40
