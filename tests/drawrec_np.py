"""An independent model of the DRAW RECORD (spacefortress_amd/csrc/sf_drawrec.h), in plain numpy, vectorised over envs.

Written from the header's documented meaning, in the slow form: every object gets an integer pixel box by floor / ceil, the
explosion's box is clamped to the surface, and two boxes meet by `Box.meets` -- none of the kernel's float-edge shortcut
(`FBox`).  Positions are rounded to float32 first, as the record documents; the geometry is then evaluated in float64.

  decode / encode / live_bytes   the 432-byte record: eight header words, the ship's piece, 20 missile pieces, 20 headings
  header(snap, pics)             the eight words of oracle snapshots (a structured array or a dict of arrays), and the env's
                                 MARGIN: the smallest distance in pixels between a compared box edge and the integer it is
                                 compared with, over all decisions of that env
  record(snap, pics)             the whole record of a snapshot
  slack / wireframe_slack        what an object alone lights up, against the box the decisions use for it (oracle/render_np.py)

The kernels evaluate in float32 and the compiler may contract to fma: with |coordinate| < 128 px a float32 ulp is 2^-17 px, so
an env whose margin is under TIE (1e-4 px) is a tie, and its decision bits are nobody's to state."""
import numpy as np

NSLOT = 20
REC_BYTES, HDR_BYTES, PIECE = 432, 32, 16
SHIP_OFF, FORT_OFF, MISSILE_OFF, ANGLES_OFF = 32, 48, 64, 384

# header words
W_SHIP_X, W_SHIP_Y, W_POINTS, W_OBJMASK, W_SHELLS, W_FLAGS, W_SERIAL, W_ANGLES = range(8)
# flag bits of word 5 (bits 0..7: background index, 8..11: the bar's state)
F_SHIP_ALIVE, F_FORT_ALIVE, F_NEAR_TEXT, F_NEAR_BAR, F_EX_TEXT, F_EX_BAR, F_OTHER_TEXT, F_OTHER_BAR = (1 << b for b in range(12, 20))
F_FORT_EX_PATCH, F_FORT_EX_PLACE, F_BAKED_TEXT, F_BAKED_BAR, F_MERGE_SHELLS, F_MISSILE19 = (1 << b for b in range(20, 26))

# the surface and its user-unit window (sf_raster.h)
IMG_W, IMG_H, VP_X, VP_Y, SCALE = 90, 92, 130.0, 80.0, 0.2
TEXT_BOX = (31, 1, 59, 6)   # x0, y0, x1, y1: pixels [x0, x1) x [y0, y1)
BAR_BOX = (25, 88, 65, 91)
FORT_PIC_BOX = (37, 39, 53, 55)
REACH_X, REACH_Y = 1, 2     # what a pixel of the 84x84 image reads beyond its own source pixel
FORT = (355.0, 315.0)
# half-extents in pixels: the live ship, a missile, a shell, an explosion
SHIP_EXT = 27 * .2
MISSILE_EXT = 26.5 * .2 + 0.01
SHELL_EXT = 17.5 * .2 + 0.01
EXPLOSION_EXT = 64.5 * .2
VULN_TIME = 250
FIRST_MISSILE_LANE, LANES = 7, 64  # the frame kernel's stroke lanes: 0..2 ship, 3..6 fortress, then three per missile slot

TIE = 1e-4
# The same extents and the same conversion as the library evaluates them, operation by operation in float32: what a TIE's
# decision bits are held to.  This leans on the library's build flags (spacefortress_amd/build.py: -ffp-contract=off
# -fno-fast-math): with contraction on, (x - 130) * .2 -+ ext may fuse and a tie's bits are no longer these -- whoever changes
# those flags drops the float32 comparison of the ties (test_gpu_drawrec_edges.check_records), not the model
_F = np.float32
EXT32 = {SHIP_EXT: _F(27) * _F(.2), MISSILE_EXT: _F(26.5) * _F(.2) + _F(.01), SHELL_EXT: _F(17.5) * _F(.2) + _F(.01),
         EXPLOSION_EXT: _F(64.5) * _F(.2)}


# ---------------------------------------------------------------- codec

def decode(rec):
    """uint8 [N, 432] -> dict(words uint32 [N, 8], ship float64 [N, 2], missiles float64 [N, 20, 2], angles int16 [N, 20])."""
    rec = np.ascontiguousarray(rec, np.uint8)
    n = rec.shape[0]
    assert rec.shape == (n, REC_BYTES), rec.shape
    return dict(words=rec[:, :HDR_BYTES].copy().view("<u4"),
                ship=rec[:, SHIP_OFF:SHIP_OFF + PIECE].copy().view("<f8"),
                missiles=rec[:, MISSILE_OFF:MISSILE_OFF + NSLOT * PIECE].copy().view("<f8").reshape(n, NSLOT, 2),
                angles=rec[:, ANGLES_OFF:ANGLES_OFF + 2 * NSLOT].copy().view("<i2"))


def encode(d):
    """The inverse of decode; the fortress's piece and the bytes behind the twentieth heading are zero."""
    n = len(d["words"])
    rec = np.zeros((n, REC_BYTES), np.uint8)
    rec[:, :HDR_BYTES] = np.ascontiguousarray(d["words"], "<u4").view(np.uint8).reshape(n, HDR_BYTES)
    rec[:, SHIP_OFF:SHIP_OFF + PIECE] = np.ascontiguousarray(d["ship"], "<f8").view(np.uint8).reshape(n, PIECE)
    rec[:, MISSILE_OFF:MISSILE_OFF + NSLOT * PIECE] = np.ascontiguousarray(d["missiles"], "<f8").view(np.uint8).reshape(n, NSLOT * PIECE)
    rec[:, ANGLES_OFF:ANGLES_OFF + 2 * NSLOT] = np.ascontiguousarray(d["angles"], "<i2").view(np.uint8).reshape(n, 2 * NSLOT)
    return rec


def live_bytes(words):
    """bool [N, 432]: the bytes that mean something -- the header, the ship's piece, the pieces and headings of the LIVE
    missile slots (object-mask bits 2..21).  A dead slot keeps whatever was there; the fortress's piece is unused."""
    words = np.asarray(words)
    n = len(words)
    live = np.zeros((n, REC_BYTES), bool)
    live[:, :HDR_BYTES] = True
    live[:, SHIP_OFF:SHIP_OFF + PIECE] = True
    for s in range(NSLOT):
        on = ((words[:, W_OBJMASK] >> np.uint32(2 + s)) & 1).astype(bool)[:, None]
        live[:, MISSILE_OFF + PIECE * s:MISSILE_OFF + PIECE * (s + 1)] = on
        live[:, ANGLES_OFF + 2 * s:ANGLES_OFF + 2 * s + 2] = on
    return live


# ---------------------------------------------------------------- boxes

def widened(b):
    return (b[0] - REACH_X, b[1] - REACH_Y, b[2] + REACH_X, b[3] + REACH_Y)


def pixel(x, y):
    """User units, rounded to float32 as the record documents, to surface pixels in float64."""
    x = np.asarray(x, np.float64).astype(np.float32).astype(np.float64)
    y = np.asarray(y, np.float64).astype(np.float32).astype(np.float64)
    return (x - VP_X) * SCALE, (y - VP_Y) * SCALE


class Boxes:
    """Pixel boxes [x0, x1) x [y0, y1) of objects at (x, y) with half-extent ext: integer corners by floor / ceil, and the
    float edges they came from (for the margin)."""

    def __init__(self, x, y, ext, clamp=False, f32=False):
        if f32:  # (x - 130.f) * .2f, then -+ the float32 extent: float32 throughout
            gx = (np.asarray(x, np.float64).astype(_F) - _F(VP_X)) * _F(SCALE)
            gy = (np.asarray(y, np.float64).astype(_F) - _F(VP_Y)) * _F(SCALE)
            ext = np.asarray(ext, np.float64)
            e32 = np.zeros(ext.shape, _F)
            for k, v in EXT32.items():
                e32 = np.where(ext == k, v, e32).astype(_F)
            ext = np.broadcast_to(e32, gx.shape)
            assert (ext > 0).all() and gx.dtype == _F and (gx - ext).dtype == _F
        else:
            gx, gy = pixel(x, y)
            ext = np.broadcast_to(np.asarray(ext, np.float64), gx.shape)
        self.edges = (gx - ext, gy - ext, gx + ext, gy + ext)
        self.x0, self.y0 = np.floor(self.edges[0]).astype(np.int64), np.floor(self.edges[1]).astype(np.int64)
        self.x1, self.y1 = np.ceil(self.edges[2]).astype(np.int64), np.ceil(self.edges[3]).astype(np.int64)
        c = np.broadcast_to(np.asarray(clamp, bool), gx.shape)  # explosion_box: clamped to the surface
        self.x0, self.y0 = np.where(c, np.maximum(self.x0, 0), self.x0), np.where(c, np.maximum(self.y0, 0), self.y0)
        self.x1, self.y1 = np.where(c, np.minimum(self.x1, IMG_W), self.x1), np.where(c, np.minimum(self.y1, IMG_H), self.y1)

    def meets(self, o):
        """Box.meets against the constant box o"""
        return (self.x0 < o[2]) & (o[0] < self.x1) & (self.y0 < o[3]) & (o[1] < self.y1)

    def margin(self, o):
        """the smallest distance of a float edge to the integer it is compared with in meets(o)"""
        e = self.edges
        return np.minimum(np.minimum(np.abs(e[0] - o[2]), np.abs(e[2] - o[0])), np.minimum(np.abs(e[1] - o[3]), np.abs(e[3] - o[1])))

    def at(self, i=0):
        return (int(self.x0[i]), int(self.y0[i]), int(self.x1[i]), int(self.y1[i]))


def around(x, y, ext):
    """The integer box of one object, as a tuple"""
    return Boxes(np.array([x]), np.array([y]), ext).at()


def explosion_box(x, y):
    """The clamped integer box of one explosion, as a tuple"""
    return Boxes(np.array([x]), np.array([y]), EXPLOSION_EXT, clamp=True).at()


def bar_state(vlner, fort_vuln_timer):
    """drawVlner's state: 0..10 tenths, 11 = full and white (kill-ready)"""
    vlner, t = np.asarray(vlner, np.int64), np.asarray(fort_vuln_timer, np.int64)
    return np.where((vlner > 10) & (t < VULN_TIME), 11, np.minimum(vlner, 10))


def hud_flags(x, y, ext, live, f32=False):
    """Per projectile [N, 20]: bit 0 on the score's box, 1 on the bar's, 2 / 3 within reach of them; and the margins."""
    b = Boxes(x, y, ext, f32=f32)
    bits = np.zeros(b.x0.shape, np.uint32)
    margin = np.full(b.x0.shape, np.inf)
    for k, t in enumerate((TEXT_BOX, BAR_BOX, widened(TEXT_BOX), widened(BAR_BOX))):
        bits |= np.where(b.meets(t), 1 << k, 0).astype(np.uint32)
        margin = np.minimum(margin, b.margin(t))
    live = np.asarray(live, bool)
    return np.where(live, bits, 0).astype(np.uint32), np.where(live, margin, np.inf)


# ---------------------------------------------------------------- the header

def _f(snap, k):
    return np.asarray(snap[k])


def masks(snap):
    w = np.uint32(1) << np.arange(NSLOT, dtype=np.uint32)
    mm = ((_f(snap, "missile_alive") != 0) * w[None, :]).sum(1).astype(np.uint32)
    sm = ((_f(snap, "shell_alive") != 0) * w[None, :]).sum(1).astype(np.uint32)
    return mm, sm


def header(snap, pics=True, f32=False):
    """(words uint32 [N, 8], margin float64 [N]) of oracle snapshots.  pics: the batch has its pictures (False for a batch
    that draws everything in place).  f32: the geometry in the library's float32 operations instead of float64 (for ties; the
    margin returned means nothing then)."""
    n = len(_f(snap, "ship_x"))
    ship_alive, fort_alive = _f(snap, "ship_alive") != 0, _f(snap, "fort_alive") != 0
    sx32, sy32 = _f(snap, "ship_x").astype(np.float32), _f(snap, "ship_y").astype(np.float32)
    ship_angle, fort_angle = _f(snap, "ship_angle").astype(np.int64), _f(snap, "fort_angle").astype(np.int64)
    vlner, fvt = _f(snap, "vlner").astype(np.int64), _f(snap, "fort_vuln_timer").astype(np.int64)
    pnts = np.trunc(_f(snap, "points").astype(np.float32).astype(np.float64)).astype(np.int64)  # drawScore takes an int
    mmask, smask = masks(snap)
    m_live, s_live = _f(snap, "missile_alive") != 0, _f(snap, "shell_alive") != 0

    # the projectiles: OR over live missiles and live shells
    mf, mm = hud_flags(_f(snap, "missile_x"), _f(snap, "missile_y"), MISSILE_EXT, m_live, f32)
    sf, sm = hud_flags(_f(snap, "shell_x"), _f(snap, "shell_y"), SHELL_EXT, s_live, f32)
    proj = np.bitwise_or.reduce(mf, axis=1) | np.bitwise_or.reduce(sf, axis=1)
    margin = np.minimum(mm.min(1), sm.min(1))

    # what the ship drew: its strokes, or the dead one's explosion (clamped to the surface)
    sb = Boxes(sx32, sy32, np.where(ship_alive, SHIP_EXT, EXPLOSION_EXT), clamp=~ship_alive, f32=f32)
    wt, wb = widened(TEXT_BOX), widened(BAR_BOX)
    mt, mb = sb.meets(wt), sb.meets(wb)
    margin = np.minimum(margin, np.minimum(sb.margin(wt), sb.margin(wb)))
    on_t, on_b = sb.meets(TEXT_BOX), sb.meets(BAR_BOX)
    margin = np.where(ship_alive, np.minimum(margin, np.minimum(sb.margin(TEXT_BOX), sb.margin(BAR_BOX))), margin)

    ex_text, ex_bar = ~ship_alive & mt, ~ship_alive & mb
    other_text, other_bar = (ship_alive & mt) | ((proj & 4) != 0), (ship_alive & mb) | ((proj & 8) != 0)
    near_text = ex_text | ((proj & 1) != 0) | (ship_alive & on_t)
    near_bar = ex_bar | ((proj & 2) != 0) | (ship_alive & on_b)
    baked_text, baked_bar = (pnts == 0) & ~near_text, (vlner == 0) & ~near_bar
    variant = baked_text.astype(np.int64) + 2 * baked_bar.astype(np.int64)

    # the fortress: its picture is in the background when its heading has one and the ship's box stays out of reach of it
    wfp = widened(FORT_PIC_BOX)
    has_pic = pics & fort_alive & (fort_angle >= 0) & (fort_angle < 360) & (fort_angle % 10 == 0)
    fort_pic = has_pic & ~sb.meets(wfp)
    margin = np.where(has_pic, np.minimum(margin, sb.margin(wfp)), margin)
    bg = np.where(fort_pic, 4 * (1 + fort_angle // 10), 0) + variant
    wfe = widened(explosion_box(*FORT))
    fe_patch = ~fort_alive & pics & ~sb.meets(wfe)
    fe_place = ~fort_alive & ~fe_patch
    margin = np.where(~fort_alive & pics, np.minimum(margin, sb.margin(wfe)), margin)

    # shells ride in the top lanes of the missiles' range when they fit there (four lanes per slot, 1 + highest live slot
    # <= 8) and no live missile slot from the first one whose three lanes reach into theirs upward
    sh_hi = np.where(s_live, np.arange(1, NSLOT + 1), 0).max(1).astype(np.int64)
    sh_base = LANES - 4 * sh_hi
    touched = np.array([min(m for m in range(NSLOT + 1) if FIRST_MISSILE_LANE + 3 * m + 2 >= LANES - 4 * h or m == NSLOT)
                        for h in range(NSLOT + 1)], np.int64)  # by 1 + highest live shell slot
    first_touched = touched[sh_hi]
    merge = (smask != 0) & (sh_hi <= 8) & ((mmask.astype(np.int64) >> first_touched) == 0)

    words = np.zeros((n, 8), np.uint32)
    words[:, W_SHIP_X], words[:, W_SHIP_Y] = sx32.view(np.uint32), sy32.view(np.uint32)
    words[:, W_POINTS] = (pnts & 0xFFFFFFFF).astype(np.uint32)
    words[:, W_OBJMASK] = ship_alive.astype(np.uint32) | ((fort_alive & ~fort_pic).astype(np.uint32) << 1) | (mmask << 2)
    words[:, W_SHELLS] = smask | np.where(merge, sh_base << 24, 0).astype(np.uint32)
    fl = bg | (bar_state(vlner, fvt) << 8)
    for bit, on in ((F_SHIP_ALIVE, ship_alive), (F_FORT_ALIVE, fort_alive), (F_NEAR_TEXT, near_text), (F_NEAR_BAR, near_bar),
                    (F_EX_TEXT, ex_text), (F_EX_BAR, ex_bar), (F_OTHER_TEXT, other_text), (F_OTHER_BAR, other_bar),
                    (F_FORT_EX_PATCH, fe_patch), (F_FORT_EX_PLACE, fe_place), (F_BAKED_TEXT, baked_text), (F_BAKED_BAR, baked_bar),
                    (F_MERGE_SHELLS, merge), (F_MISSILE19, m_live[:, 19])):
        fl = fl | np.where(on, bit, 0)
    words[:, W_FLAGS] = fl.astype(np.uint32)
    words[:, W_SERIAL] = _f(snap, "time").astype(np.int64).astype(np.uint32)
    words[:, W_ANGLES] = ((ship_angle & 0xFFFF) | ((fort_angle << 16) & 0xFFFF0000)).astype(np.uint32)
    return words, margin


def record(snap, pics=True, f32=False):
    """(uint8 [N, 432], margin): the record of oracle snapshots; dead missile slots carry the snapshot's values too (mask
    them with live_bytes)."""
    words, margin = header(snap, pics, f32)
    d = dict(words=words, ship=np.stack([_f(snap, "ship_x"), _f(snap, "ship_y")], 1).astype(np.float64),
             missiles=np.stack([_f(snap, "missile_x"), _f(snap, "missile_y")], 2).astype(np.float64),
             angles=_f(snap, "missile_angle").astype(np.int16))
    return encode(d), margin


# ---------------------------------------------------------------- ink against boxes (oracle/render_np.py)

def lit_box(frame):
    """(x0, y0, x1, y1) of the pixels of a frame that are not black, or None"""
    ys, xs = np.nonzero(frame)
    return None if len(xs) == 0 else (int(xs.min()), int(ys.min()), int(xs.max()) + 1, int(ys.max()) + 1)


def slack(frame, box):
    """How far the ink of `frame` stays inside `box` on its (left, top, right, bottom) side, in pixels: negative where ink
    lies outside."""
    l = lit_box(frame)
    assert l is not None, "nothing drawn"
    return (l[0] - box[0], l[1] - box[1], box[2] - l[2], box[3] - l[3])


def worst_headings(R, lines, pos=(301.5, 303.5)):
    """For each side (left, top, right, bottom): the whole-degree heading at which a wireframe at `pos` puts its ink farthest
    toward that side (the first such heading), from 360 renders."""
    gx, gy = pixel(pos[0], pos[1])
    reach = np.zeros((360, 4))
    for a in range(360):
        l = lit_box(R.run_script(R.s_begin() + R.s_wireframe(lines, pos, a)))
        reach[a] = (gx - l[0], gy - l[1], l[2] - gx, l[3] - gy)
    return [int(h) for h in reach.argmax(0)]


def wireframe_slack(R, lines, ext, pos, angle):
    """One wireframe alone on black at `pos` (user units) and a whole-degree heading: its slack in around(pos, ext)"""
    frame = R.run_script(R.s_begin() + R.s_wireframe(lines, pos, angle))
    return slack(frame, around(pos[0], pos[1], ext))
