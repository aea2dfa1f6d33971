"""Placements for the run-time-geometry frame kernels (sf_render_view.hip, sf_render_generic.hip): oracle snapshot records, one
per lane, each a quiet base state plus ONE object under test, aimed at what play almost never lands on -- the seams between a
view's bands of rows, the margins its painter culls strokes by, the four sides and corners of the surface, and the decisions
of the draw order (the shell's d > 21, the bar's states, the score's digits).  No GPU: the states are numpy records, the
extents an object is aimed by are MEASURED on the CPU model's own drawing of it (oracle/render_np.py over cairo_model.c), never
taken from the kernel's constants.

A view is (W, H, viewport, lw, grey).  `band_h` restates sf_view_host.cpp's rule in Python; it only AIMS placements at seams
(tests/test_view_edges_model.py holds it to the host code; dense() does not depend on it at all).

Kinds that move with the state: ship, dead_ship (its explosion), missile, shell.  Kinds whose place is the reference's -- the
live fortress at a heading (fort), its explosion (dead_fort), the bar, the score -- cannot be carried to a seam; for them the
tests choose viewports that lay a seam or an edge across them (fort_decisions, bar_decisions, score_decisions with
SCORE_VIEW, BAR_SEAM_VIEW, BAR_CUT_VIEW)."""
import math
import os
from collections import namedtuple

import numpy as np

from oracle import render_np as R

View = namedtuple("View", "W H viewport lw grey")
# what a placement is: the lane's index into the records, its object kind, heading (None: the kind has none), where it was
# aimed ("seam 32", "top", "corner tl", "dense", a decision's name), from which side ("above", "below", "on", "out-in"), the
# offset of the sweep in pixels, the centre in device pixels, and what the model must show of it against the base frame:
# "ink" (differs), "none" (equal), "either"; nudge: (nx, ny) in {-1, 0, 1} -- the centre's user coordinate is the double next
# to the one (cx, cy) maps to, that way (one ulp either side of a whole pixel, taken where the state can express it)
Place = namedtuple("Place", "kind heading where side off cx cy expect nudge", defaults=((0, 0),))

MOVERS = ("ship", "dead_ship", "missile", "shell")
RECTILINEAR = (0, 90, 180, 270)
OBLIQUE = (33, 127, 211, 305)
HEADINGS = RECTILINEAR + OBLIQUE
PARK = (-400.0, -400.0)  # the base state's ship: off every surface the tests use (asserted per view in base())
FORT = (355.0, 315.0)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MISSILE_SLOT, SHELL_SLOT = 5, 7
SHELL_SPEED = 6.0
BAND_BYTES = 49152
BAR_MAX = 13  # (vlner is drawn as min(vlner, 10); the engine's own counter goes a little past 10)


def band_h(W, planes):
    """sf_view_host.cpp:116-124 restated: rows per workgroup."""
    m = next((c for c in (1, 2, 4, 8, 16) if (W * c) % 16 == 0), 16)
    bh = min(BAND_BYTES // (planes * W), 32)
    bh -= bh % m
    return max(bh, m)


def seams(view):
    bh = band_h(view.W, 1 if view.grey else 3)
    return list(range(bh, view.H, bh))


def scales(view):
    return view.W / float(view.viewport[2]), view.H / float(view.viewport[3])


def to_user(view, cx, cy):
    sx, sy = scales(view)
    return view.viewport[0] + cx / sx, view.viewport[1] + cy / sy


def shell_velocity(heading):
    """A shell's heading is what its velocity says; half a degree off the whole one, so that its truncation is not in question."""
    a = math.radians(heading + 0.5)
    return SHELL_SPEED * math.cos(a), SHELL_SPEED * math.sin(a), heading + 0.5


# ---------------------------------------------------------------- the model's drawing of one object: its extent
def _object_script(kind, x, y, heading):
    if kind in ("dead_ship", "dead_fort"):
        return R.s_explosion((x, y))
    lines = {"ship": R.SHIP_LINES, "fort": R.FORT_LINES, "missile": R.MISSILE_LINES, "shell": R.SHELL_LINES}[kind]
    return R.s_wireframe(lines, (x, y), heading)


_extents = {}


def extent(view, kind, heading):
    """(left, up, right, down) in whole pixels: how far the model's ink of the object reaches from its centre at this view's
    scales and line width, the centre on a whole pixel corner of a scratch surface."""
    sx, sy = scales(view)
    key = (sx, sy, view.lw, kind, heading)
    if key not in _extents:
        import viewmodel as V
        n, c = 256, 128
        saved = (R.W, R.H, R.VP_X, R.VP_Y, R.VP_W, R.VP_H, R.SX, R.SY, R.LINE_W, R.SCALE)
        V.set_view(n, n, (1000.0 - c / sx, 1000.0 - c / sy, n / sx, n / sy), view.lw)
        try:
            fb = R.run_script(R.s_begin() + _object_script(kind, 1000.0, 1000.0, heading or 0))
        finally:
            R.W, R.H, R.VP_X, R.VP_Y, R.VP_W, R.VP_H, R.SX, R.SY, R.LINE_W, R.SCALE = saved
        rows, cols = np.flatnonzero(fb.any(1)), np.flatnonzero(fb.any(0))
        assert len(rows) and rows[0] > 0 and rows[-1] < n - 1 and cols[0] > 0 and cols[-1] < n - 1, (kind, heading)
        _extents[key] = (c - int(cols[0]), c - int(rows[0]), int(cols[-1]) + 1 - c, int(rows[-1]) + 1 - c)
    return _extents[key]


# ---------------------------------------------------------------- records
def base(O, view, n):
    """n quiet records: the ship alive and parked off the surface, the fortress alive at heading 0, nothing in flight, zero
    points, an empty bar."""
    s = np.zeros(n, O.SNAPSHOT_DTYPE)
    s["ship_alive"], s["fort_alive"] = 1, 1
    s["ship_x"], s["ship_y"] = PARK
    sx, sy = scales(view)
    px, py = (PARK[0] - view.viewport[0]) * sx, (PARK[1] - view.viewport[1]) * sy
    assert px < -64 and py < -64, ("the parked ship is not off this view", view)
    return s


def put(s, i, kind, x, y, heading):
    """The object under test into record i."""
    if kind in ("ship", "dead_ship"):
        s["ship_x"][i], s["ship_y"][i], s["ship_angle"][i] = x, y, heading or 0
        s["ship_alive"][i] = kind == "ship"
        s["ship_death_timer"][i] = 0 if kind == "ship" else 100
    elif kind == "missile":
        s["missile_alive"][i, MISSILE_SLOT] = 1
        s["missile_x"][i, MISSILE_SLOT], s["missile_y"][i, MISSILE_SLOT], s["missile_angle"][i, MISSILE_SLOT] = x, y, heading
    elif kind == "shell":
        vx, vy, a = shell_velocity(heading)
        s["shell_alive"][i, SHELL_SLOT] = 1
        s["shell_x"][i, SHELL_SLOT], s["shell_y"][i, SHELL_SLOT] = x, y
        s["shell_vx"][i, SHELL_SLOT], s["shell_vy"][i, SHELL_SLOT], s["shell_angle"][i, SHELL_SLOT] = vx, vy, a
    elif kind == "fort":
        s["fort_angle"][i] = s["fort_last_angle"][i] = heading
    elif kind == "dead_fort":
        s["fort_alive"][i], s["fort_death_timer"][i] = 0, 100
    else:
        raise ValueError(kind)


class _Geometry:
    """render_np's module geometry set to a view's for a while."""

    def __init__(self, view):
        self.view = view

    def __enter__(self):
        import viewmodel as V
        self.saved = (R.W, R.H, R.VP_X, R.VP_Y, R.VP_W, R.VP_H, R.SX, R.SY, R.LINE_W, R.SCALE)
        V.set_view(self.view.W, self.view.H, self.view.viewport, self.view.lw)

    def __exit__(self, *exc):
        R.W, R.H, R.VP_X, R.VP_Y, R.VP_W, R.VP_H, R.SX, R.SY, R.LINE_W, R.SCALE = self.saved


def alone(view, kind, x, y, heading):
    """The model's drawing of ONE object by itself on black in the view, grey: straight from the placement's coordinates, not
    through a state record -- what a placement's frame is expected to show is decided by this, so a record that fails to
    carry its object (a flag not set, a slot not filled) cannot go unnoticed."""
    with _Geometry(view):
        return R.run_script(R.s_begin() + _object_script(kind, x, y, int(heading or 0)))


def _text_box(view):
    """The surface's pixels the score text can touch, generously: user x 285 .. 425 (seven cells of 18 about 355), y 75 .. 113."""
    sx, sy = scales(view)
    x0, x1 = int(math.floor((285 - view.viewport[0]) * sx)), int(math.ceil((425 - view.viewport[0]) * sx))
    y0, y1 = int(math.floor((75 - view.viewport[1]) * sy)), int(math.ceil((113 - view.viewport[1]) * sy))
    return slice(max(y0, 0), max(y1, 0)), slice(max(x0, 0), max(x1, 0))


_blank = {}


def blank(view):
    """Where the base frame is black and no text can come: there whatever an object inks shows in the frame as it is."""
    key = tuple(view)
    if key not in _blank:
        import viewmodel as V
        hp = np.load(os.path.join(GOLDEN, "tables.npz"))["hex_points"]
        s = np.zeros(1, _record_dtype())
        s["ship_alive"], s["fort_alive"] = 1, 1
        s["ship_x"], s["ship_y"] = PARK
        b = V.frame(s[0], hp, view.W, view.H, view.viewport, view.lw, True)[..., 0] == 0
        b[_text_box(view)] = False
        _blank[key] = b
    return _blank[key]


def _record_dtype():
    from oracle import oracle as O
    return O.SNAPSHOT_DTYPE


def _expect(view, kind, heading, x, y):
    """What the model's frame must show of a mover at user (x, y) against the base frame: "ink" where the object drawn alone
    inks a pixel that is black in the base frame (the frame then has that ink there), "none" where it inks no pixel of the
    surface or is a shell within 21 of the fortress, "either" in the rare rest: all its ink on the surface lies on something
    the base frame draws (a sliver on a hexagon's line), where equal greys can hide it."""
    if kind == "shell" and _dist(x, y) <= 21:
        return "none"
    a = alone(view, kind, x, y, heading)
    if not a.any():
        return "none"
    return "ink" if (a[blank(view)] > 0).any() else "either"


def _expect_fortress(view, kind, heading):
    """The fortress is the base frame's own object: its frame differs from the base frame where its drawing alone differs from
    the drawing alone of the fortress at heading 0 in a pixel nothing else of the base frame touches."""
    d = alone(view, kind, FORT[0], FORT[1], heading) != alone(view, "fort", FORT[0], FORT[1], 0)
    if not d.any():
        return "none"
    with _Geometry(view):
        hp = np.load(os.path.join(GOLDEN, "tables.npz"))["hex_points"]
        rest = R.bar_frame(R.run_script(R.s_begin() + R.s_hexagon(hp[:12]) + R.s_hexagon(hp[12:])), 0, False)
    rest[_text_box(view)] = 255
    return "ink" if (d & (rest == 0)).any() else "either"


def _expect_bar(view, vlner, timer):
    with _Geometry(view):
        z = np.zeros((view.H, view.W), np.uint8)
        return "ink" if not np.array_equal(R.bar_frame(z, vlner, vlner > 10 and timer < 250), R.bar_frame(z, 0, False)) else "none"


def fine_offsets():
    """Pixels around an aimed point: k / 16 over [-2, 2] (_coords adds one ulp either side of every whole pixel in it)."""
    return [k / 16.0 for k in range(-32, 33)]


def _coords(base_px):
    """(offset, coordinate, nudge): base_px + every fine offset, and each whole pixel within the range nudged either way."""
    out = [(o, base_px + o, 0) for o in fine_offsets()]
    for w in range(int(math.ceil(base_px - 2)), int(math.floor(base_px + 2)) + 1):
        out += [(w - base_px, float(w), -1), (w - base_px, float(w), 1)]
    return out


def _coarse(a, b, frac=0.37):
    """Whole pixels + frac from a to b (a < b), at most about 24 of them."""
    step = max(1, int(math.ceil((b - a) / 24.0)))
    return [math.floor(a) + k * step + frac for k in range(int((b - a) // step) + 2)]


class Batch:
    """Placements gathered into records."""

    def __init__(self, O, view):
        self.O, self.view, self.places, self._rows = O, view, [], []

    def add(self, kind, heading, where, side, off, cx, cy, expect=None, nudge=(0, 0), **fields):
        s = base(self.O, self.view, 1)
        if kind in MOVERS:
            x, y = to_user(self.view, cx, cy)
            x = float(np.nextafter(x, nudge[0] * np.inf)) if nudge[0] else x
            y = float(np.nextafter(y, nudge[1] * np.inf)) if nudge[1] else y
            put(s, 0, kind, x, y, heading)
            expect = expect or _expect(self.view, kind, heading, x, y)
        elif kind in ("fort", "dead_fort"):
            put(s, 0, kind, FORT[0], FORT[1], heading)
            expect = expect or _expect_fortress(self.view, kind, heading)
        for k, v in fields.items():
            s[k][0] = v
        self._rows.append(s)
        self.places.append(Place(kind, heading, where, side, off, cx, cy, expect or "either", tuple(nudge)))

    def done(self):
        snaps = np.concatenate(self._rows) if self._rows else np.zeros(0, self.O.SNAPSHOT_DTYPE)
        return snaps, self.places


def _headings(kind):
    return (None,) if kind == "dead_ship" else HEADINGS


def seam_sweeps(O, view, kinds=MOVERS):
    """(a): for every seam row r and every mover, the centre set so that the object's outermost ink (extent()) just reaches r
    from above and from below, stepped through fine offsets in device y; and the centre on the seam.  Headings rotate along
    the offsets, every heading starting a sweep in turn; the column rotates over three places of the surface's width."""
    B = Batch(O, view)
    g = 0
    for r in seams(view):
        for kind in kinds:
            hs = _headings(kind)
            for side in ("above", "below"):
                for j, (off, _, nudge) in enumerate(_coords(0.0)):
                    h = hs[(j + g) % len(hs)]
                    L, U, Rt, D = extent(view, kind, h)
                    aim = r - D if side == "above" else r + U
                    cy = _coords(aim)[j][1]
                    cx = view.W * (0.25, 0.5, 0.75)[(j + g) % 3] + 0.29
                    B.add(kind, h, "seam %d" % r, side, off, cx, cy, nudge=(0, nudge))
                g += 1
            for h in hs:
                for cy, nudge in ((float(r), 0), (float(r), -1), (r + 0.5, 0)):
                    B.add(kind, h, "seam %d" % r, "on", cy - r, view.W * 0.5 + 0.29, cy, nudge=(0, nudge))
    return B.done()


SIDES = ("top", "bottom", "left", "right")
CORNERS = ("tl", "tr", "bl", "br")


def edge_sweeps(O, view, kinds=MOVERS):
    """(b): across each side and corner of the surface, from wholly outside (further than the extent) to wholly inside (or the
    surface's middle where the object is larger than the surface): fine offsets around the point where the first ink enters
    and around the centre on the edge, whole pixels + .37 between.  Centres go negative and past W, H."""
    B = Batch(O, view)
    g = 0
    n_f = len(_coords(0.0))

    def along(edge, sign, reach, depth, span, j):
        """Entry j of the sweep along one axis: (side, offset, coordinate, nudge) or None past its end.  edge: the edge's coordinate,
        sign: +1 where inside is the larger coordinate."""
        if j < n_f:
            off, c, nudge = _coords(edge - sign * float(reach))[j]
            return "enters", off, c, nudge
        if j < 2 * n_f:
            off, c, nudge = _coords(float(edge))[j - n_f]
            return "on", off, c, nudge
        cs = _coarse(-reach - 3.0, min(depth + 3.0, span / 2.0))
        if j - 2 * n_f >= len(cs):
            return None
        t = cs[j - 2 * n_f]
        return "out-in", t, edge + sign * t, 0

    for kind in kinds:
        hs = _headings(kind)
        for where in SIDES + tuple("corner " + c for c in CORNERS):
            g += 1
            for j in range(2 * n_f + 27):
                h = hs[(j + g) % len(hs)]
                L, U, Rt, D = extent(view, kind, h)
                mid_x, mid_y = view.W * 0.5 + 0.29, view.H * 0.5 + 0.29
                if where == "top":
                    e, cx = along(0, 1, D, U, view.H, j), mid_x
                elif where == "bottom":
                    e, cx = along(view.H, -1, U, D, view.H, j), mid_x
                elif where == "left":
                    e, cy = along(0, 1, Rt, L, view.W, j), mid_y
                elif where == "right":
                    e, cy = along(view.W, -1, L, Rt, view.W, j), mid_y
                else:  # a corner: both axes at once, each by its own extent
                    c, span = where[-2:], min(view.W, view.H)
                    ey = along(0, 1, D, U, span, j) if c[0] == "t" else along(view.H, -1, U, D, span, j)
                    ex = along(0, 1, Rt, L, span, j) if c[1] == "l" else along(view.W, -1, L, Rt, span, j)
                    if ex is None or ey is None:
                        continue
                    B.add(kind, h, where, ey[0], ey[1], ex[2], ey[2], nudge=(ex[3], ey[3]))
                    continue
                if e is None:
                    continue
                if where in ("top", "bottom"):
                    cy = e[2]
                else:
                    cx = e[2]
                B.add(kind, h, where, e[0], e[1], cx, cy, nudge=(0, e[3]) if where in ("top", "bottom") else (e[3], 0))
    return B.done()


def dense(O, view, kinds=MOVERS, frac=0.43):
    """(c): every mover's centre on every whole row of the surface (and two rows either side of it) + frac, the heading and
    the column rotating.  Nothing here knows band_h."""
    B = Batch(O, view)
    for ki, kind in enumerate(kinds):
        hs = _headings(kind)
        for row in range(-2, view.H + 2):
            h = hs[(row + ki) % len(hs)]
            B.add(kind, h, "dense", "row", float(row), view.W * (0.3, 0.5, 0.7)[(row + ki) % 3] + 0.19, row + frac)
    return B.done()


def _dist(x, y):
    return math.sqrt((x - FORT[0]) ** 2 + (y - FORT[1]) ** 2)  # (the model's and the kernel's own expression)


def shell_decisions(O, view):
    """(d): a shell at distance 21 from the fortress on both axes (either way) and on two diagonals: the nominal point; the
    outermost double along the ray whose computed distance is still <= 21 ("inside": draws nothing, d > 21 at
    SRC/draw.cpp:248-253) and the very next double ("outside": drawn) -- one ulp of the POSITION apart, which near 376 is
    sixteen ulps of 21 --; and a unit either way."""
    B = Batch(O, view)
    sx, sy = scales(view)
    for name, (ux, uy) in (("+x", (1, 0)), ("-x", (-1, 0)), ("+y", (0, 1)), ("-y", (0, -1)), ("diag", (0.6, 0.8)), ("diag-", (-0.8, -0.6))):
        x0, y0 = FORT[0] + ux * 21.0, FORT[1] + uy * 21.0
        along_x = abs(ux) >= abs(uy)
        far = math.copysign(1e9, ux if along_x else uy)

        def moved(t, k):
            """k doubles outward (k < 0: inward) from t"""
            for _ in range(abs(k)):
                t = float(np.nextafter(t, far if k > 0 else -far))
            return t

        k = 0
        pos = lambda k: (moved(x0, k), y0) if along_x else (x0, moved(y0, k))  # noqa: E731
        while _dist(*pos(k)) > 21:
            k -= 1
        while _dist(*pos(k + 1)) <= 21:
            k += 1
        for side, (x, y) in (("at", (x0, y0)), ("inside", pos(k)), ("outside", pos(k + 1)),
                             ("well inside", (FORT[0] + ux * 20.0, FORT[1] + uy * 20.0)), ("well outside", (FORT[0] + ux * 22.0, FORT[1] + uy * 22.0))):
            s = base(O, view, 1)
            put(s, 0, "shell", x, y, 45)
            B._rows.append(s)
            cx, cy = (x - view.viewport[0]) * sx, (y - view.viewport[1]) * sy
            B.places.append(Place("shell", 45, "d21 " + name, side, _dist(x, y) - 21.0, cx, cy, _expect(view, "shell", 45, x, y)))
    return B.done()


def bar_decisions(O, view):
    """(d): vlner 0, 10, 11 and the largest, the vulnerability timer either side of 250."""
    B = Batch(O, view)
    for vl in (0, 1, 10, 11, BAR_MAX):
        for timer in (249, 250, 251):
            B.add("bar", None, "bar", "vlner %d timer %d" % (vl, timer), 0.0, 0.0, 0.0, _expect_bar(view, vl, timer),
                  vlner=vl, fort_vuln_timer=timer)
    return B.done()


SCORES = (0, -1, 9, -9999999, 9999999, 511, 512)


def score_decisions(O, view):
    """(d): the points whose text has every length and sign."""
    B = Batch(O, view)
    for p in SCORES:
        B.add("score", None, "score", "points %d" % p, 0.0, 0.0, 0.0, "none" if p == 0 else "either", points=p, raw_points=p)
    return B.done()


def fort_decisions(O, view):
    """The fortress, alive at the rectilinear and the oblique headings (heading 0 is the base frame itself), and destroyed."""
    B = Batch(O, view)
    cx, cy = (FORT[0] - view.viewport[0]) * scales(view)[0], (FORT[1] - view.viewport[1]) * scales(view)[1]
    for h in HEADINGS:
        B.add("fort", h, "fort", "heading %d" % h, 0.0, cx, cy)
    B.add("dead_fort", None, "fort", "destroyed", 0.0, cx, cy)
    return B.done()


def keys(snaps):
    """One bytes key per record, of its fields only (the aligned record type has padding, which numpy does not define)."""
    packed = np.dtype([(n, snaps.dtype[n]) for n in snaps.dtype.names])
    flat = np.ascontiguousarray(snaps.astype(packed)).view(np.uint8).reshape(len(snaps), packed.itemsize)
    return [r.tobytes() for r in flat]


def named(O, view, where, items):
    """Placements given by hand: items of (kind, heading, user x, user y) -- the findings kept as cases."""
    B = Batch(O, view)
    sx, sy = scales(view)
    for kind, heading, x, y in items:
        s = base(O, view, 1)
        put(s, 0, kind, x, y, heading)
        B._rows.append(s)
        B.places.append(Place(kind, heading, where, "named", 0.0, (x - view.viewport[0]) * sx, (y - view.viewport[1]) * sy, _expect(view, kind, heading, x, y)))
    return B.done()


def join(*parts):
    """The parts' records and placements in order; a record that an earlier part already has is dropped (an explosion whose
    extent equals the seam's row meets the seam and the top edge in the same place)."""
    snaps = np.concatenate([p[0] for p in parts])
    places = [q for p in parts for q in p[1]]
    seen, keep = set(), []
    for i, k in enumerate(keys(snaps)):
        if k not in seen:
            seen.add(k)
            keep.append(i)
    return snaps[keep], [places[i] for i in keep]


def label(p):
    ulp = "" if p.nudge == (0, 0) else " nudged %+d, %+d ulp" % p.nudge
    return "%s h=%s %s %s off=%.4f at (%.4f, %.4f)%s" % (p.kind, p.heading, p.where, p.side, p.off, p.cx, p.cy, ulp)


def object_rows(view, p):
    """The rows a mover's ink can touch (extent + 1), or None where it is wholly off the surface sideways."""
    L, U, Rt, D = extent(view, p.kind, p.heading)
    if p.cx + Rt + 1 < 0 or p.cx - L - 1 > view.W:
        return None
    return p.cy - U - 1, p.cy + D + 1


def assert_clear_of_rows(view, places, rows):
    """A view compared below `rows` masked rows: no placement may have any part of its object in them (zero hidden cases)."""
    for p in places:
        if p.kind in MOVERS and rows > 0:
            r = object_rows(view, p)
            assert r is None or r[0] >= rows or r[1] < 0, ("an object under test lies in the masked text rows", label(p))


# ---------------------------------------------------------------- the views and geometries of the tests
# name -> View; why each: profiles/view_edge_tests.md
VIEWS = {
    "fort112_lw1": View(112, 80, (299, 286, 112, 80), 1.0, True),      # band_h 32: bands 32 / 32 / 16; a seam 1 row inside the
    "fort112_lw2": View(112, 80, (299, 286, 112, 80), 2.0, True),      # fortress's tip at heading 90 (user y 350 | 351)
    "fort112_lw45": View(112, 80, (299, 286, 112, 80), 4.5, True),
    "gui450": View(450, 72, (130, 280, 450, 72), 2.0, False),          # m = 8, bands 32 / 32 / 8
    "wide1023": View(1023, 40, (-160, 300, 1030, 40), 2.0, False),     # m = 16, band_h 16: 16 / 16 / 8; sx = 1023 / 1030
    "wide1024": View(1024, 40, (-157, 300, 1024, 40), 2.0, True),      # band_h 32: 32 / 8
    "w700": View(700, 50, (5, 290, 700, 50), 2.0, False),              # m = 4, band_h 20: 20 / 20 / 10
    "short": View(200, 24, (255, 303, 200, 24), 2.0, True),            # H < band_h: one partial band
    "aniso": View(154, 100, (255, 215, 200, 200), 4.5, False),         # sx .77, sy .5: bands 32 / 32 / 32 / 4
}
BAND_H = {"fort112_lw1": 32, "fort112_lw2": 32, "fort112_lw45": 32, "gui450": 32, "wide1023": 16, "wide1024": 32, "w700": 20,
          "short": 32, "aniso": 32}  # (what the issue's list of views promises; test_view_edges_model holds band_h() to it)
# views for the fixed kinds: the score's glyph rows across seam 32 and cut by both sides; the bar across seam 32; the bar cut
# by the bottom edge
SCORE_VIEW = View(112, 80, (299, 65, 112, 80), 2.0, True)
BAR_SEAM_VIEW = View(300, 80, (205, 495, 300, 80), 2.0, False)
BAR_CUT_VIEW = View(112, 80, (250, 447, 112, 80), 2.0, True)
# (scale, viewport, ls, atlas of score_glyphs.npz or None) of the general renderer's tests
GEOMETRIES = {
    "quarter": (0.25, (100, 60, 500, 520), 2, 1),       # 125 x 130: the hexagons and the fortress inside
    "close-up": (0.75, (255, 215, 200, 200), 3, None),  # 150 x 150 at the renderer's largest scale: objects hang over every side
    "close-up-lw45": (0.75, (255, 215, 200, 200), 4.5, None),  # the widest line of the fixtures there: the circle's stroke is wide
}                                                              # against its radius (FOUND below)

# FOUND by these tests, kept as named cases (profiles/view_edge_tests.md):
#  * a hole in a stroke: where two strokes of one wireframe overlap inside a pixel cairo's row sums pass a full cell, its 8-bit
#    span coverage wraps from 256 to 0 and the pixel stays black; the model and the kernels clamped to 255.  The ship at
#    heading 305 in the anisotropic view (device centres below), pixel (row 20, column 112) of the first
HOLE_VIEW = "aniso"
HOLE_CENTRES = ((115.79, 18.4375), (38.79, 19.4375), (38.79, 49.4375), (115.79, 51.4375))
#  * the explosion's circle under a wide line: the rows through the top and the bottom of its stroke hold ten pieces at line
#    width 4.5 (1.0 and .75 pixels per unit); the rasteriser took a row whole only up to eight and sampled the others in
#    sub-rows, which cairo does not.  User centres: the unit view fort112_lw45 (rows 26 and 38; 58 and 70), the close-up
#  * and the other way round: cairo's inner_join puts the path's point where two of the circle's Bezier segments meet into the
#    polygon, so the row that holds it -- 7 units above or below the centre -- is no full row for cairo; the kernel took it
#    whole.  The last two centres of the unit view: row 3 with the centre above the surface; rows 33 and 47 with it inside
WIDE_CIRCLE_UNIT = ((355.29, 318.5), (355.29, 350.5), (355.29, 282.3125), (355.29, 326.43))
WIDE_CIRCLE_CLOSE_UP = ((330.37, 300.61), (331.85, 300.05), (330.70, 300.10), (331.81, 301.93))


def geometry_view(name):
    sc, vp, ls, _ = GEOMETRIES[name]
    return View(int(vp[2] * sc), int(vp[3] * sc), vp, float(ls), True)


def unit_view(view):
    vp = view.viewport
    return vp[2] == view.W and vp[3] == view.H and float(vp[0]).is_integer() and float(vp[1]).is_integer()


def masked_rows(view):
    """Rows of a view without an atlas that the score text can touch (none where the viewport starts below the text)."""
    import viewmodel as V
    return max(0, V.text_rows(view.H, view.viewport))
