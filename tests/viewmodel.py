"""The CPU model of a VIEW's frame (sf_render_view): oracle/render_np.py's draw scripts through oracle/cairo_model.c, once per
channel in colour.  Colour is the grey pipeline per channel: each stroke's coverage is the same, its source value is the
channel's byte of the reference's colour (SRC/draw.cpp, SRC/wireframe.cpp): hexagons green, ship and fortress yellow,
missiles white, shells red, explosion arcs yellow below radius 60 and red above, the closing circle yellow; the score
text and the bar are grey in both modes.  Frames are [H, W, 4] uint8 B, G, R, 255 -- the bytes of pb_pixels."""
import math

import numpy as np

from oracle import render_np as R

# (r, g, b) of the colour mode
YELLOW, RED, GREEN, WHITE = (1, 1, 0), (1, 0, 0), (0, 1, 0), (1, 1, 1)


def set_view(width, height, viewport, lw):
    """render_np's module geometry for a view of any size (set_geometry takes a scale; a view names its surface)."""
    R.VP_X, R.VP_Y, R.VP_W, R.VP_H = (float(v) for v in viewport)
    R.W, R.H = int(width), int(height)
    R.SX, R.SY = R.W / R.VP_W, R.H / R.VP_H
    R.LINE_W = float(lw)
    R.SCALE = R.SX


def text_rows(height, viewport):
    """Rows of a view that the score text can touch (the text's box ends at user y 108 + its ink)."""
    return int((112 - viewport[1]) * (height / viewport[3])) + 1


def _explosion(pos, src):
    x, y = float(pos[0]), float(pos[1])
    s = [R.LINE_WIDTH, float(np.float32(R.LINE_W))]
    for radius, a0, a1, grey in R.explosion_arcs():
        s += [R.GREY, src(YELLOW if grey == 191 else RED, .75 if grey == 191 else .5), R.ARC, x, y, float(radius), R.deg2rad(a0),
              R.deg2rad(a1), R.STROKE]
    return s + [R.GREY, src(YELLOW, .75), R.ARC, x, y, 7.0, 0.0, R.M_PI * 2, R.STROKE]


def _objects(snap, src):
    s = []
    ship = (float(snap["ship_x"]), float(snap["ship_y"]))
    s += R.s_wireframe(R.SHIP_LINES, ship, snap["ship_angle"], src(YELLOW, 1.0)) if snap["ship_alive"] else _explosion(ship, src)
    s += R.s_wireframe(R.FORT_LINES, R.FORT, snap["fort_angle"], src(YELLOW, 1.0)) if snap["fort_alive"] else _explosion(R.FORT, src)
    for i in range(len(snap["missile_alive"])):
        if snap["missile_alive"][i]:
            s += R.s_wireframe(R.MISSILE_LINES, (snap["missile_x"][i], snap["missile_y"][i]), snap["missile_angle"][i], src(WHITE, 1.0))
    for i in range(len(snap["shell_alive"])):
        d = math.sqrt((snap["shell_x"][i] - R.FORT[0]) ** 2 + (snap["shell_y"][i] - R.FORT[1]) ** 2)
        if snap["shell_alive"][i] and d > 21:
            s += R.s_wireframe(R.SHELL_LINES, (snap["shell_x"][i], snap["shell_y"][i]), snap["shell_angle"][i], src(RED, 1.0))
    return s


def frame(snap, hex_points, width, height, viewport, lw, grayscale, glyphs=None, vuln_time=250):
    """One view frame of an oracle snapshot record, [H, W, 4] B, G, R, 255.  glyphs: the view's atlas (dict alpha, layout, x0);
    None: no text at all (the caller compares the rows below it)."""
    saved = (R.W, R.H, R.VP_X, R.VP_Y, R.VP_W, R.VP_H, R.SX, R.SY, R.LINE_W, R.SCALE)
    set_view(width, height, viewport, lw)
    try:
        return _frame(snap, hex_points, grayscale, glyphs, vuln_time)
    finally:  # (render_np's geometry is module-wide: other tests draw in theirs)
        R.W, R.H, R.VP_X, R.VP_Y, R.VP_W, R.VP_H, R.SX, R.SY, R.LINE_W, R.SCALE = saved


def _frame(snap, hex_points, grayscale, glyphs, vuln_time):
    hb, hs = hex_points[:12], hex_points[12:]
    vlner = int(snap["vlner"])
    kill = vlner > 10 and int(snap["fort_vuln_timer"]) < vuln_time
    out = np.full((R.H, R.W, 4), 255, np.uint8)
    for c in range(3):  # B, G, R
        if grayscale:
            src = lambda rgb, grey: grey  # noqa: E731
        else:
            src = lambda rgb, grey, c=c: float(rgb[2 - c])  # noqa: E731
        fb = R.run_script(R.s_begin() + R.s_hexagon(hb, src(GREEN, 1.0)) + R.s_hexagon(hs, src(GREEN, 1.0)) + _objects(snap, src))
        if glyphs is not None:
            fb = R.score_text_atlas(fb, snap["points"], glyphs)
        out[:, :, c] = R.bar_frame(fb, vlner, kill)
        if grayscale:
            out[:, :, 1] = out[:, :, 2] = out[:, :, 0]
            break
    return out


def unit_glyphs(atlas, viewport):
    """The atlas of 1.0 pixel per unit (atlas_unit.npz: user coordinates) placed for a view at a whole viewport offset."""
    gw, gh, adv, y0 = (int(v) for v in atlas["layout"])
    return dict(alpha=atlas["alpha"], layout=(gw, gh, adv, y0 - int(viewport[1])), x0=atlas["x0"].astype(np.int64) - int(viewport[0]))


def fixture_glyphs(z):
    """A view fixture's own atlas (frames_<view>.npz: alpha, layout, x0), or None."""
    return dict(alpha=z["alpha"], layout=z["layout"], x0=z["x0"]) if "alpha" in z.files else None


def fixture_view(z):
    """(width, height, viewport, lw, grayscale) of a view fixture."""
    v = z["view"]
    return int(v[0]), int(v[1]), tuple(float(x) for x in v[2:6]), float(v[6]), bool(v[7])
