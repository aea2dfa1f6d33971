"""The numpy model of the draw record (tests/drawrec_np.py) held to account without a GPU:

  * its header words against words worked out by hand from the documented meaning of sf_drawrec.h -- every flag bit and
    every field at least once set and once clear;
  * its codec against itself and against byte offsets written out;
  * the EXTENTS the decisions use against the renderer model (oracle/render_np.py): each object drawn alone on a black
    surface lights no pixel outside the box the decisions use for it, and at its worst heading comes within 2 px of every
    side of that box -- a box loosened by a typo would otherwise pass forever.

What a pixel of the 84x84 image reads beyond its own source pixel (kReachX, kReachY) is held by
tests/test_image_host.py::test_dirty_boxes_of_the_resampling_are_exact and not repeated here.
tests/test_gpu_drawrec_edges.py then holds the kernels to this model at the edges of every decision."""
import numpy as np
import pytest

import drawrec_np as D


def quiet(n=1, **kw):
    """n envs in which nothing is near anything: the live ship right of the fortress, the fortress at heading 0, no points, an
    empty bar, no projectiles.  Keyword arguments replace fields (scalars, or arrays of n; projectile fields [n, 20])."""
    s = dict(ship_alive=np.ones(n, np.int32), ship_x=np.full(n, 455.0), ship_y=np.full(n, 315.0), ship_angle=np.zeros(n),
             fort_alive=np.ones(n, np.int32), fort_angle=np.zeros(n), points=np.zeros(n, np.float32), vlner=np.zeros(n, np.int32),
             fort_vuln_timer=np.zeros(n, np.int32), time=np.zeros(n, np.int32))
    for k in ("missile", "shell"):
        s[k + "_alive"] = np.zeros((n, 20), np.int32)
        s[k + "_x"], s[k + "_y"] = np.full((n, 20), 555.0), np.full((n, 20), 315.0)
        s[k + "_angle"] = np.zeros((n, 20))
    for k, v in kw.items():
        s[k] = np.broadcast_to(np.asarray(v, s[k].dtype), s[k].shape).copy()
    return s


def with_projectile(kind, slot, x, y, **kw):
    s = quiet(**kw)
    s[kind + "_alive"][0, slot] = 1
    s[kind + "_x"][0, slot], s[kind + "_y"][0, slot] = x, y
    return s


def words(s, pics=True):
    return [int(w) for w in D.header(s, pics)[0][0]]


# pixels of a position: gx = (x - 130) / 5, gy = (y - 80) / 5.  The boxes, [x0, x1) x [y0, y1):
#   text 31..59 x 1..6, widened by the reach (1, 2): 30..60 x -1..8;  bar 25..65 x 88..91, widened 24..66 x 86..93
#   the fortress's picture 37..53 x 39..55, widened 36..54 x 37..57
#   the fortress's explosion 45 +- 12.9, 47 +- 12.9 -> 32..58 x 34..60, widened 31..59 x 32..62
# flags: 0x1000 ship alive, 0x2000 fortress alive, 0x4000 near text, 0x8000 near bar, 0x10000 explosion on text, 0x20000 on bar,
#   0x40000 other on text, 0x80000 on bar, 0x100000 fortress explosion restored, 0x200000 in place, 0x400000 baked text,
#   0x800000 baked bar, 0x1000000 shells merged, 0x2000000 missile 19


def test_quiet_env_all_eight_words():
    # ship (455, 315) -> (65, 47) +- 5.4 = 59.6..70.4 x 41.6..52.4: left of nothing, above nothing; 59.6 >= 54: clear of the picture
    # heading 180 -> sector 18: background 4 * 19 + 3 (text and bar baked) = 79 = 0x4F
    w = words(quiet(ship_angle=90, fort_angle=180, time=3400))
    assert w == [0x43E38000,  # 455.0f = 1.77734375 * 2^8: exponent 135, mantissa 0x638000
                 0x439D8000,  # 315.0f = 1.23046875 * 2^8: mantissa 0x1D8000
                 0, 1, 0,
                 0x4F | 0x1000 | 0x2000 | 0x400000 | 0x800000,
                 3400, 90 | 180 << 16]
    assert w[5] == 0xC0304F and w[7] == 0x00B4005A
    assert words(quiet()) == [0x43E38000, 0x439D8000, 0, 1, 0, 0xC03007, 0, 0]
    assert words(quiet(ship_angle=359, fort_angle=350))[7] == 0x015E0167
    # a negative heading keeps its low 16 bits: -1 -> 0xFFFF; the fortress's -10 -> 0xFFF6, outside 0..359: strokes, no picture
    w = words(quiet(ship_angle=-1, fort_angle=-10))
    assert (w[3], w[5], w[7]) == (3, 0xC03003, 0xFFF6FFFF)


def test_a_missile_on_within_reach_of_and_clear_of_the_score():
    # (355, 97.5) -> (45, 3.5) +- 5.31 = 39.69..50.31 x -1.81..8.81 -> 39..51 x -2..9: on the text box
    # not baked, background 4 + 2; object mask: ship | slot 3 << 2
    w = words(with_projectile("missile", 3, 355.0, 97.5))
    assert (w[3], w[5]) == (0x21, 0x847006)  # 6 | 0x3000 | 0x4000 | 0x40000 | 0x800000
    # (355, 142.5) -> gy 12.5, top edge 7.19 -> row 7: not < 6, but < 8: within reach only, the text stays baked
    w = words(with_projectile("missile", 3, 355.0, 142.5))
    assert (w[3], w[5]) == (0x21, 0xC43007)  # 7 | 0x3000 | 0x40000 | 0xC00000
    # (355, 147.5) -> gy 13.5, top edge 8.19 -> row 8: clear
    w = words(with_projectile("missile", 3, 355.0, 147.5))
    assert (w[3], w[5]) == (0x21, 0xC03007)
    # beside the box: (205, 97.5) -> gx 15, right edge 20.31 -> x1 21 <= 30
    assert words(with_projectile("missile", 3, 205.0, 97.5))[5] == 0xC03007
    # a dead slot at the same place says nothing
    s = with_projectile("missile", 3, 355.0, 97.5)
    s["missile_alive"][0, 3] = 0
    assert words(s)[3:6] == [1, 0, 0xC03007]


def test_a_shell_on_within_reach_of_and_clear_of_the_bar():
    # (355, 525) -> (45, 89) +- 3.51 = 41.49..48.51 x 85.49..92.51: on the bar.  Slot 2 alone: 1 + highest = 3 <= 8 and no
    # missiles: merged, first lane 64 - 12 = 52 = 0x34
    w = words(with_projectile("shell", 2, 355.0, 525.0))
    assert (w[3], w[4], w[5]) == (1, 0x34000004, 0x148B005)  # 5 | 0x3000 | 0x8000 | 0x80000 | 0x400000 | 0x1000000
    # (355, 495) -> gy 83, bottom edge 86.51 -> y1 87: not > 88, but > 86: within reach only
    w = words(with_projectile("shell", 2, 355.0, 495.0))
    assert (w[4], w[5]) == (0x34000004, 0x1C83007)  # 7 | 0x3000 | 0x80000 | 0xC00000 | 0x1000000
    # (355, 490) -> gy 82, bottom edge 85.51 -> y1 86: clear
    assert words(with_projectile("shell", 2, 355.0, 490.0))[5] == 0x1C03007
    # a shell on the score: (355, 97.5) -> 41.49..48.51 x -0.01..7.01
    assert words(with_projectile("shell", 2, 355.0, 97.5))[5] == 0x1847006
    # a missile on the bar: (355, 525) -> 85.69..94.31
    assert words(with_projectile("missile", 0, 355.0, 525.0))[5] == 0x48B005


def test_the_live_ship_on_and_near_the_score():
    # (355, 105) -> (45, 5) +- 5.4 = 39.6..50.4 x -0.4..10.4: on the text box; 10.4 < 37: clear of the picture
    assert words(quiet(ship_x=355.0, ship_y=105.0))[5] == 0x847006
    # (355, 140) -> gy 12, top edge 6.6 -> row 6: not < 6, < 8: within reach
    assert words(quiet(ship_x=355.0, ship_y=140.0))[5] == 0xC43007
    # on the bar: (355, 525) -> 83.6..94.4
    assert words(quiet(ship_x=355.0, ship_y=525.0))[5] == 0x48B005


def test_the_dead_ships_explosion():
    # (355, 150) -> (45, 14) +- 12.9 = 32.1..57.9 x 1.1..26.9: meets the widened text box; 26.9 < 37: clear of the picture
    w = words(quiet(ship_alive=0, ship_x=355.0, ship_y=150.0))
    assert (w[3], w[5]) == (0, 0x816006)  # 6 | 0x2000 | 0x4000 | 0x10000 | 0x800000
    # ... with 5 points and 3 tenths on the bar: nothing baked, background 4, bar state 3
    w = words(quiet(ship_alive=0, ship_x=355.0, ship_y=150.0, points=5, vlner=3))
    assert (w[2], w[5]) == (5, 0x16304)  # 4 | 0x300 | 0x2000 | 0x4000 | 0x10000
    # (355, 480) -> gy 80: 67.1..92.9 meets the widened bar box, 67.1 >= 57: clear of the picture
    assert words(quiet(ship_alive=0, ship_x=355.0, ship_y=480.0))[5] == 0x42A005  # 5 | 0x2000 | 0x8000 | 0x20000 | 0x400000
    # (455, 315) -> 52.1..77.9 x 34.1..59.9: 52.1 < 54: on the fortress's picture -> the fortress's strokes in place, background 3
    w = words(quiet(ship_alive=0))
    assert (w[3], w[5]) == (2, 0xC02003)
    # its box is clamped to the surface: at (140, 100) -> (2, 4): -10.9.. -> 0..15 x 0..17, nothing met
    assert D.explosion_box(140.0, 100.0) == (0, 0, 15, 17)
    assert words(quiet(ship_alive=0, ship_x=140.0, ship_y=100.0))[5] == 0xC02007


def test_the_fortress_picture_strokes_and_explosion():
    # live ship at (420, 315) -> gx 58, left edge 52.6 -> 52 < 54: on the picture: strokes (object bit 1), background = variant
    w = words(quiet(ship_x=420.0))
    assert (w[3], w[5]) == (3, 0xC03003)
    # (430, 315) -> gx 60, left edge 54.6 -> 54: clear
    assert words(quiet(ship_x=430.0))[3:6] == [1, 0, 0xC03007]
    # a heading between two pictures, or outside 0..359: strokes
    assert words(quiet(fort_angle=45))[3:6] == [3, 0, 0xC03003]
    assert words(quiet(fort_angle=360))[3:6] == [3, 0, 0xC03003]
    # heading 350: sector 35, background 4 * 36 + 3 = 147 = 0x93
    assert words(quiet(fort_angle=350))[5] == 0xC03093
    # a batch without pictures
    assert words(quiet(), pics=False)[3:6] == [3, 0, 0xC03003]
    # destroyed: restored from its picture while the ship is clear of 31..59 x 32..62 (quiet ship: left edge 59.6)
    assert words(quiet(fort_alive=0))[3:6] == [1, 0, 0xD01003]  # 3 | 0x1000 | 0x100000 | 0xC00000
    # (450, 315) -> gx 64, left edge 58.6 -> 58 < 59: drawn in place
    assert words(quiet(fort_alive=0, ship_x=450.0))[3:6] == [1, 0, 0xE01003]
    assert words(quiet(fort_alive=0), pics=False)[3:6] == [1, 0, 0xE01003]


def test_bar_states_and_points():
    assert words(quiet(vlner=4))[5] == 0x403405      # 5 | 0x400 | 0x3000 | 0x400000
    assert words(quiet(vlner=10, fort_vuln_timer=0))[5] == 0x403A05
    assert words(quiet(vlner=11, fort_vuln_timer=249))[5] == 0x403B05  # kill-ready
    assert words(quiet(vlner=11, fort_vuln_timer=250))[5] == 0x403A05
    assert words(quiet(vlner=15, fort_vuln_timer=4000))[5] == 0x403A05
    # the points are the float's truncation toward zero
    for p, w2, w5 in ((0.95, 0, 0xC03007), (-0.95, 0, 0xC03007), (1.000001, 1, 0x803006), (-1, 0xFFFFFFFF, 0x803006),
                      (-513, 0xFFFFFDFF, 0x803006), (512, 512, 0x803006)):
        w = words(quiet(points=p))
        assert (w[2], w[5]) == (w2, w5), p


def test_merged_shells_and_the_twentieth_missile():
    far = dict(kind="shell", x=555.0, y=315.0)

    def both(shell_slot, missile_slot):
        s = with_projectile(far["kind"], shell_slot, far["x"], far["y"])
        if missile_slot is not None:
            s["missile_alive"][0, missile_slot] = 1
        return words(s)

    # slot 7: 1 + 7 = 8 slots of four lanes: lanes 32..63.  Missile slot m has lanes 7 + 3 m .. 9 + 3 m: slot 7 ends at 30, slot 8
    # (31..33) reaches in
    assert both(7, None)[3:6] == [1, 0x20000080, 0x1C03007]
    assert both(7, 7)[3:6] == [1 | 1 << 9, 0x20000080, 0x1C03007]
    assert both(7, 8)[3:6] == [1 | 1 << 10, 0x80, 0xC03007]
    assert both(8, None)[3:6] == [1, 0x100, 0xC03007]  # nine slots do not fit
    # slot 0: lanes 60..63; missile slot 16 ends at 57, slot 17 (58..60) reaches in
    assert both(0, 16)[4] == 0x3C000001
    assert both(0, 17)[4] == 1
    assert both(19, None)[4] == 0x80000
    # the twentieth missile
    assert both(0, 19)[3:6] == [1 | 1 << 21, 1, 0x2C03007]
    s = quiet()
    s["missile_alive"][0, 19] = 1
    assert words(s)[3:6] == [0x200001, 0, 0x2C03007]


def test_margins_and_ties():
    # the quiet ship's left edge 59.6 against the widened text box's 60: 0.4 px; nothing else is nearer
    assert abs(D.header(quiet())[1][0] - 0.4) < 1e-9
    # (457, 315) -> left edge 65.4 - 5.4 = 60: a tie
    assert D.header(quiet(ship_x=457.0))[1][0] < D.TIE
    # a missile's top edge 7.19 against 8 and 6: 0.81 -- and the ship's 0.4 is smaller
    s = with_projectile("missile", 3, 355.0, 142.5, ship_x=555.0)  # ship (85, 47): 79.6 against 66: far
    assert abs(D.header(s)[1][0] - 0.81) < 1e-6
    # vectorised: the margins and words of three envs equal those of each alone
    three = quiet(3, ship_x=[455.0, 457.0, 355.0], ship_y=[315.0, 315.0, 105.0])
    w, m = D.header(three)
    for i, (x, y) in enumerate(((455.0, 315.0), (457.0, 315.0), (355.0, 105.0))):
        w1, m1 = D.header(quiet(ship_x=x, ship_y=y))
        assert np.array_equal(w[i], w1[0]) and m[i] == m1[0]


def test_codec():
    s = with_projectile("missile", 3, 355.25, 97.5, time=68)
    s["missile_angle"][0, 3] = 271
    rec, _ = D.record(s)
    assert rec.shape == (1, 432) and rec.dtype == np.uint8
    r = rec[0]
    assert r[:32].view("<u4").tolist() == words(s)
    assert r[32:48].view("<f8").tolist() == [455.0, 315.0]           # the ship's piece
    assert r[64 + 16 * 3:80 + 16 * 3].view("<f8").tolist() == [355.25, 97.5]  # missile slot 3
    assert r[384 + 2 * 3:386 + 2 * 3].view("<i2").tolist() == [271]
    live = D.live_bytes(rec[:, :32].view("<u4"))
    assert int(live.sum()) == 32 + 16 + 16 + 2 and live[0, 112:128].all() and live[0, 390:392].all() and not live[0, 48:64].any()
    d = D.decode(rec)
    assert np.array_equal(D.encode(d), rec)
    rng = np.random.default_rng(4)
    raw = rng.integers(0, 256, (300, 432), dtype=np.uint8)
    raw[:, 48:64] = 0
    raw[:, 424:] = 0
    assert np.array_equal(D.encode(D.decode(raw)), raw)


# ---------------------------------------------------------------- the extents against the renderer model

@pytest.fixture(scope="module")
def R():
    from oracle import render_np as R

    R.model_lib()
    return R


PHASE = (1.5, 3.5)  # user units: 0.3, 0.7 px
HEADINGS8 = (0, 45, 90, 135, 180, 225, 270, 315)


def _wireframe_cases():
    for a in range(360):
        yield (300.0 + PHASE[0], 300.0 + PHASE[1]), a
    for a in HEADINGS8:
        for i in range(4):
            for j in range(4):
                yield (300.0 + 1.25 * i, 300.0 + 1.25 * j), a + 7  # (off the 45-degree grid as well)
                yield (300.0 + 1.25 * i, 300.0 + 1.25 * j), a


@pytest.mark.parametrize("name,ext", [("SHIP_LINES", "SHIP_EXT"), ("MISSILE_LINES", "MISSILE_EXT"), ("SHELL_LINES", "SHELL_EXT")])
def test_wireframes_stay_inside_their_boxes_and_fill_them(R, name, ext):
    lines, e = getattr(R, name), getattr(D, ext)
    sl = np.array([D.wireframe_slack(R, lines, e, pos, a) for pos, a in _wireframe_cases()])
    assert sl.min() >= 0, ("ink outside the box", name, sl.min(0).tolist())
    assert (sl.min(0) <= 2).all(), ("a loose box", name, sl.min(0).tolist())


def test_an_explosion_stays_inside_its_box_and_fills_it(R):
    sl = []
    for x, y in ((300.0, 300.0), (301.5, 303.5), (302.5, 301.25), (303.75, 302.5)):
        sl.append(D.slack(R.run_script(R.s_begin() + R.s_explosion((x, y))), D.explosion_box(x, y)))
    sl = np.array(sl)
    assert sl.min() >= 0 and (sl.min(0) <= 2).all(), sl.tolist()
    # clamped at every border of the surface: the ink is clipped there too
    for x, y in ((150.0, 100.0), (560.5, 520.5), (355.0, 60.0), (355.0, 560.0), (100.0, 315.0), (600.0, 315.0)):
        b = D.explosion_box(x, y)
        assert 0 <= b[0] < b[2] <= D.IMG_W and 0 <= b[1] < b[3] <= D.IMG_H, b
        assert min(D.slack(R.run_script(R.s_begin() + R.s_explosion((x, y))), b)) >= 0, (x, y)


def test_the_fortress_stays_inside_its_picture_box_and_fills_it(R):
    sl = np.array([D.slack(R.run_script(R.s_begin() + R.s_wireframe(R.FORT_LINES, D.FORT, a)), D.FORT_PIC_BOX) for a in range(0, 360, 10)])
    assert sl.min() >= 0 and (sl.min(0) <= 2).all(), sl.min(0).tolist()
    # the destroyed fortress's explosion: the box the decisions widen
    assert D.explosion_box(*D.FORT) == (32, 34, 58, 60)


def test_the_score_stays_inside_the_text_box_and_fills_it(R):
    A = R.load_glyphs(0)
    black = np.zeros((D.IMG_H, D.IMG_W), np.uint8)
    sl = np.array([D.slack(R.score_text_atlas(black, p, A), D.TEXT_BOX) for p in (0, -8888888, 8888888, 9999999)])
    assert sl.min() >= 0 and (sl.min(0) <= 2).all(), sl.tolist()


def test_the_bar_stays_inside_the_bar_box_and_fills_it(R):
    black = np.zeros((D.IMG_H, D.IMG_W), np.uint8)
    sl = np.array([D.slack(R.bar_frame(black, v, kill), D.BAR_BOX) for v, kill in [(v, False) for v in range(11)] + [(11, True)]])
    assert sl.min() >= 0 and (sl.min(0) <= 2).all(), sl.tolist()
