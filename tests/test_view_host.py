"""Views (sf_render_view) without a GPU: sf_view_check's defaults and limits, the circle's Bezier segment count against
oracle/cairo_model.c's restatement of cairo's rule, and the per-channel colour model (tests/viewmodel.py) against every
frame the reference's own renderer drew in a view (tests/golden/views, make_views_golden.py)."""
import ctypes as C
import glob
import math
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN

VIEWS = os.path.join(GOLDEN, "views")


@pytest.fixture(scope="module")
def L():
    from spacefortress_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        pytest.fail("libsfmi.so not built")
    return _lib


def check(_lib, width=-1, height=-1, viewport=(0, 0, -1, -1), lw=2.0, grayscale=0, fmt=0):
    v = _lib.View(width, height, *(float(x) for x in viewport), float(lw), grayscale, fmt)
    w, h = C.c_int32(), C.c_int32()
    rc = _lib.lib().sf_view_check(C.byref(v), C.byref(w), C.byref(h))
    return rc, (w.value, h.value)


def test_view_check_defaults(L):
    """The reference's defaulting (SRC/pymodule.cpp:345-349): viewport size -1 -> 710 x 626, surface -1 -> the viewport's."""
    assert check(L) == (0, (710, 626))
    assert check(L, viewport=(130, 80, 450, 460)) == (0, (450, 460))
    assert check(L, width=90, height=92, viewport=(130, 80, 450, 460), lw=3, grayscale=1) == (0, (90, 92))
    assert check(L, width=300, viewport=(130, 80, 450, -1)) == (0, (300, 626))
    assert check(L, viewport=(-50, 20, -1, 300)) == (0, (710, 300))


def test_view_check_limits(L):
    ARG = L.SF_ERR_ARG
    # exactly 1.0 pixel per unit either way is drawn; just above is refused
    assert check(L, width=450, height=460, viewport=(130, 80, 450, 460))[0] == 0
    assert check(L, width=1024, height=1024, viewport=(0, 0, 1024, 1024))[0] == 0
    assert check(L, width=450, height=460, viewport=(130, 80, 449.9999, 460))[0] == ARG
    assert check(L, width=450, height=460, viewport=(130, 80, 450, 459.9999))[0] == ARG
    assert "1.0 pixel per user unit" in L.last_error()
    assert check(L, width=451, viewport=(130, 80, 450, 460))[0] == ARG
    # sides
    assert check(L, width=1025, height=10, viewport=(0, 0, 2000, 2000))[0] == ARG
    assert check(L, width=10, height=1025, viewport=(0, 0, 2000, 2000))[0] == ARG
    assert check(L, width=0, height=10, viewport=(0, 0, 100, 100))[0] == ARG
    # viewport, line width
    for vp in ((0, 0, 0, 100), (0, 0, 100, 0), (0, 0, -2, 100), (0, 0, 100, -5)):
        assert check(L, width=10, height=10, viewport=vp)[0] == ARG, vp
    assert check(L, viewport=(0, 0, 100, 100), lw=0)[0] == ARG
    assert check(L, viewport=(0, 0, 100, 100), lw=-1)[0] == ARG
    assert check(L, viewport=(0, 0, 100, 100), lw=float("nan"))[0] == ARG
    # formats: grey output of a colour view, unknown formats
    assert check(L, viewport=(0, 0, 100, 100), fmt=2)[0] == ARG
    assert check(L, viewport=(0, 0, 100, 100), grayscale=1, fmt=2)[0] == 0
    assert check(L, viewport=(0, 0, 100, 100), fmt=3)[0] == ARG
    assert L.lib().sf_view_check(None, None, None) == ARG


# oracle/cairo_model.c: arc_max_angle, circle_major_axis, arc_in_direction (cairo-arc.c: _arc_segments_needed)
_TABLE = [(math.pi / 1.0, 0.0185185185185185036127), (math.pi / 2.0, 0.000272567143730179811158),
          (math.pi / 3.0, 2.38647043651461047433e-05), (math.pi / 4.0, 4.2455377443222443279e-06),
          (math.pi / 5.0, 1.11281001494389081528e-06), (math.pi / 6.0, 3.72662000942734705475e-07),
          (math.pi / 7.0, 1.47783685574284411325e-07), (math.pi / 8.0, 6.63240432022601149057e-08),
          (math.pi / 9.0, 3.2715520137536980553e-08), (math.pi / 10.0, 1.73863223499021216974e-08),
          (math.pi / 11.0, 9.81410988043554039085e-09)]


def model_segments(xx, yx, xy, yy, radius):
    i, j = xx * xx + yx * yx, xy * xy + yy * yy
    f, g, h = 0.5 * (i + j), 0.5 * (i - j), xx * xy + yx * yy
    major = radius * math.sqrt(f) if (abs(h) == 0 and abs(g) == 0) else radius * math.sqrt(f + math.hypot(g, h))
    tol = 0.1 / major
    angle = next((a for a, e in _TABLE if e < tol), math.pi / 12.0)
    return int(math.ceil(abs(math.pi) / angle))


def test_circle_segments_follow_cairos_rule(L):
    """Half of the radius-7 circle: one Bezier segment up to 5.4 device pixels (0.772 pixels per unit), two beyond -- over
    uniform, anisotropic, rotated and sheared matrices, and the view check's resolution of it."""
    f = L.lib().sf_view_circle_segments
    seen = set()
    for s in np.linspace(0.5, 1.0, 1001):
        for sx, sy in ((s, s), (s, 0.5), (0.3, s), (s, 1.0)):
            got = f(sx, 0.0, 0.0, sy, 7.0)
            assert got == model_segments(sx, 0.0, 0.0, sy, 7.0), (sx, sy)
            seen.add(got)
        c, n = math.cos(0.3), math.sin(0.3)
        m = (s * c, s * n, -0.8 * s * n, 0.8 * s * c)
        assert f(*m, 7.0) == model_segments(*m, 7.0)
        m = (s, 0.0, 0.25 * s, 0.9 * s)
        assert f(*m, 7.0) == model_segments(*m, 7.0)
    assert seen == {1, 2}
    assert f(0.77, 0, 0, 0.77, 7.0) == 1 and f(0.78, 0, 0, 0.78, 7.0) == 2 and f(1.0, 0, 0, 1.0, 7.0) == 2
    assert f(0.77, 0, 0, 0.78, 7.0) == 2  # the larger axis decides
    assert f(1.0, 0, 0, 1.0, 0.0) == L.SF_ERR_ARG


def _fixtures():
    return sorted(glob.glob(os.path.join(VIEWS, "frames_*.npz")))


def test_view_fixtures_are_small_and_complete():
    names = sorted(os.path.basename(p) for p in glob.glob(os.path.join(VIEWS, "*.npz")))
    assert names == ["atlas_unit.npz", "ext_autoturn_destroy.npz", "ext_youturn_deaths.npz", "frames_aniso.npz", "frames_game.npz",
                     "frames_gui.npz", "frames_gui_grey.npz", "frames_s077.npz", "frames_s078.npz"]
    for p in glob.glob(os.path.join(VIEWS, "*.npz")):
        assert os.path.getsize(p) <= 300 * 1024, p
    z = np.load(os.path.join(VIEWS, "frames_gui.npz"))
    f = z["frames"]
    assert f.shape[1:] == (460, 450, 4) and (f[..., 3] == 255).all()
    s = z["snaps"]  # what the states cover: both explosions, crowds, the kill bar, long and negative scores
    assert (s["ship_alive"] == 0).any() and (s["fort_alive"] == 0).any() and (s["shell_alive"].sum(1) >= 10).any()
    assert (s["vlner"] > 10).any() and (s["points"] >= 10 ** 6).any() and (s["points"] < 0).any()


@pytest.mark.parametrize("path", _fixtures(), ids=lambda p: os.path.basename(p)[7:-4])
def test_colour_model_equals_the_references_frames(path):
    """The per-channel model (tests/viewmodel.py) against every frame of a view fixture: every row where the view has a
    glyph atlas (the fixture's), the rows below the text where it has none."""
    import viewmodel as V
    hp = np.load(os.path.join(GOLDEN, "tables.npz"))["hex_points"]
    z = np.load(path)
    w, h, vp, lw, grey = V.fixture_view(z)
    A = V.fixture_glyphs(z)
    rows = 0 if A is not None else V.text_rows(h, vp)
    for i, s in enumerate(z["snaps"]):
        got = V.frame(s, hp, w, h, vp, lw, grey, glyphs=A)
        want = z["frames"][i]
        assert np.array_equal(got[rows:], want[rows:]), (os.path.basename(path), str(z["labels"][i]))


def test_built_in_unit_atlas_is_the_fixtures(L):
    """sf_glyphs.h's atlas of 1.0 pixel per unit (kUnit*) is what cairo gives in both native views: the fixtures' atlases,
    placed by the viewport's offset."""
    import viewmodel as V
    u = np.load(os.path.join(VIEWS, "atlas_unit.npz"))
    for name in ("gui", "game", "gui_grey"):
        z = np.load(os.path.join(VIEWS, "frames_%s.npz" % name))
        _, _, vp, _, _ = V.fixture_view(z)
        g = V.unit_glyphs(u, vp)
        assert np.array_equal(g["alpha"], z["alpha"]) and tuple(g["layout"]) == tuple(int(v) for v in z["layout"])
        assert np.array_equal(g["x0"], z["x0"])
    # ... and the header's table
    src = open(os.path.join(os.path.dirname(L.__file__), "csrc", "sf_glyphs.h")).read()
    body = re.sub(r"/\*.*?\*/", "", src.split("kUnitAlpha[SF_GLYPH_CHARS * kUnitW * kUnitH] = {")[1].split("};")[0])
    vals = [int(t) for t in body.split(",") if t.strip()]
    assert np.array_equal(np.array(vals, np.uint8), u["alpha"].reshape(-1))
    assert "kUnitW = %d, kUnitH = %d, kUnitAdvance = %d, kUnitY0 = %d" % tuple(int(v) for v in u["layout"]) in src
