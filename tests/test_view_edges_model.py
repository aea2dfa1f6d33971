"""tests/viewedges.py without a GPU: what the helper promises about its placements (every seam from both sides by every
mover, every side and corner, nothing twice, nothing in hidden rows), that every placement shows in the model's frame -- or
does not, where that is its point --, the Python restatement of the band rule against sf_view_host.cpp's own, and the CPU model
against the REAL cairo 1.16 at these placements: off the surface, at negative device coordinates, at the scales
tests/test_cairo_model.py has not seen (1.0, 1023 / 1030, the anisotropic .77 x .5, .75).  The last keeps the reference of
tests/test_gpu_view_edges.py honest; it is skipped where the probe library is absent, as tests/test_cairo_model.py is."""
import os
import subprocess

import numpy as np
import pytest

import viewedges as E
from conftest import GOLDEN
from test_cairo_model import both  # noqa: F401  (the fixture: the same script through the real cairo and through the model)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def O():
    from oracle import oracle as O
    return O


@pytest.fixture(scope="module")
def hp():
    return np.load(os.path.join(GOLDEN, "tables.npz"))["hex_points"]


# records of seam_sweeps + edge_sweeps + dense that repeat an earlier one, per view
DROPPED = {"fort112_lw1": 28, "fort112_lw2": 27, "fort112_lw45": 16, "gui450": 27, "wide1023": 8, "wide1024": 4, "w700": 4, "short": 0,
           "aniso": 42}


def _all_views():
    return list(E.VIEWS.items()) + [(n, E.geometry_view(n)) for n in E.GEOMETRIES]


@pytest.mark.parametrize("name", list(E.VIEWS))
def test_every_seam_side_and_corner_is_visited(O, name):
    view = E.VIEWS[name]
    bh = E.band_h(view.W, 1 if view.grey else 3)
    assert bh == E.BAND_H[name] and E.seams(view) == list(range(bh, view.H, bh))
    assert E.masked_rows(view) == 0  # (every view of the sweeps starts below the score text: no row is hidden)
    parts = [E.seam_sweeps(O, view), E.edge_sweeps(O, view), E.dense(O, view)]
    snaps, places = E.join(*parts)
    # no placement twice: the parts together hold exactly DROPPED[name] records that an earlier one has (an explosion whose
    # extent equals a seam's row meets the seam and the top edge in one place), and join drops those and nothing else
    together = [k for part in parts for k in E.keys(part[0])]
    assert len(together) - len(set(together)) == DROPPED[name]
    assert E.keys(snaps) == list(dict.fromkeys(together)) and len(places) == len(snaps)
    E.assert_clear_of_rows(view, places, E.masked_rows(view))
    for kind in E.MOVERS:
        mine = [p for p in places if p.kind == kind]
        # what each placement must show is decided from the object drawn alone (viewedges.alone): nearly none is left open
        assert sum(p.expect == "either" for p in mine) <= 0.02 * len(mine), (kind, "either")
        assert sum(p.expect == "ink" for p in mine) >= 0.4 * len(mine) and sum(p.expect == "none" for p in mine) >= 0.2 * len(mine), kind
        hs = set(p.heading for p in mine)
        assert hs == ({None} if kind == "dead_ship" else set(E.HEADINGS)), (kind, hs)
        for r in E.seams(view):
            L = [p for p in mine if p.where == "seam %d" % r]
            for side in ("above", "below"):
                S = [p for p in L if p.side == side]
                offs = sorted(set(p.off for p in S))
                assert set(k / 16.0 for k in range(-32, 33)) <= set(offs) and len(S) >= 70, (kind, r, side)
                # aimed by the model's extent: at offset 0 the object's last inked row is the seam's neighbour
                for p in S:
                    if p.off == 0.0 and float(p.cy).is_integer():
                        up, down = E.extent(view, kind, p.heading)[1], E.extent(view, kind, p.heading)[3]
                        assert (p.cy + down == r) if side == "above" else (p.cy - up == r), E.label(p)
                # one ulp either side of a whole row
                ulps = [p for p in S if p.nudge != (0, 0)]
                assert len(ulps) >= 8 and all(float(p.cy).is_integer() and p.nudge[0] == 0 for p in ulps), (kind, r, side)
                assert set(p.nudge[1] for p in ulps) == {-1, 1}
                if kind != "dead_ship":
                    assert set(p.heading for p in S) == set(E.HEADINGS)
                assert sum(p.expect == "ink" for p in S) >= 8, (kind, r, side, "too few placements that must show ink")
            assert any(p.cy == r and p.nudge == (0, 0) for p in mine), (kind, r)  # (the centre on the seam)
        for where in E.SIDES + tuple("corner " + c for c in E.CORNERS):
            S = [p for p in mine if p.where == where]
            assert set(p.side for p in S) == {"enters", "on", "out-in"}, (kind, where)
            assert any(p.expect == "none" for p in S), (kind, where, "never wholly outside")
            assert any(p.expect == "ink" for p in S), (kind, where, "never seen")
            out = [p for p in S if p.cx < 0 or p.cy < 0] if where in ("top", "left", "corner tl") else \
                  [p for p in S if p.cx >= view.W or p.cy >= view.H]
            assert out, (kind, where, "no centre beyond the surface")
            inside = [p for p in S if 0 < p.cx < view.W and 0 < p.cy < view.H]
            assert inside, (kind, where)
        rows = set(int(np.floor(p.cy)) for p in mine if p.where == "dense")
        assert rows >= set(range(view.H)), (kind, "dense")


def test_fortress_tip_crosses_a_seam_by_one_row():
    """What test_gpu_view_edges.test_fortress_headings_and_the_shells_distance relies on in the 112 x 80 views: the model's
    fortress at heading 90 inks row 64 and not row 65, row 64 starts a band, and the fortress's centre is in the band above --
    so the band that has to draw that one row sees only the end of the longest wireframe stroke there is."""
    for name in ("fort112_lw1", "fort112_lw2", "fort112_lw45"):
        view = E.VIEWS[name]
        assert 64 in E.seams(view)
        down = E.extent(view, "fort", 90)[3]
        cy = E.FORT[1] - view.viewport[1]
        assert cy + down == 65 and cy < 64, (name, cy, down)


@pytest.mark.parametrize("name", ["fort112_lw1", "aniso"])
def test_placements_show_in_the_model(O, hp, name):
    """Every placement's model frame differs from the base frame where the helper says "ink" and equals it where it says
    "none" (wholly outside; a shell within 21 of the fortress): a sweep that silently draws nothing cannot pass.  Here for two
    views without a GPU; tests/test_gpu_view_edges.py asserts the same of every placement it compares."""
    import viewmodel as V
    view = E.VIEWS[name]
    args = (view.W, view.H, view.viewport, view.lw, view.grey)
    snaps, places = E.join(E.seam_sweeps(O, view), E.edge_sweeps(O, view), E.dense(O, view), E.shell_decisions(O, view),
                           E.fort_decisions(O, view))
    base = V.frame(E.base(O, view, 1)[0], hp, *args)
    seen = {}
    for i in range(0, len(places), 2 if name == "aniso" else 1):
        p = places[i]
        differs = not np.array_equal(V.frame(snaps[i], hp, *args), base)
        assert p.expect == "either" or differs == (p.expect == "ink"), (differs, E.label(p))
        seen[(p.kind, p.expect)] = seen.get((p.kind, p.expect), 0) + 1
    for kind in E.MOVERS:
        assert seen[(kind, "ink")] > 400 and seen[(kind, "none")] > 200 and seen.get((kind, "either"), 0) < 20, (kind, seen)
    fort = {p.side: p.expect for p in places if p.where == "fort"}
    assert fort.pop("heading 0") == "none" and len(fort) == 8 and set(fort.values()) == {"ink"}, fort
    d21 = {(p.where, p.side): p.expect for p in places if p.where.startswith("d21")}
    assert len(d21) >= 24 and all(e == ("ink" if "outside" in side else "none") for (_, side), e in d21.items() if side != "at"), d21
    near = [p for p in places if p.where.startswith("d21") and abs(p.off) < 1e-9]  # (an "at" that is the "inside" is one record)
    assert sum(p.expect == "ink" for p in near) == 6 and sum(p.expect == "none" for p in near) >= 6, near


def test_band_rule_is_the_host_codes(tmp_path):
    """band_h() against sf_view_resolve itself (tests/native/view_band_dump.cpp: sf_view_host.cpp in a host program), for the
    views of the tests and for every width at both plane counts."""
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    if not os.path.exists(os.path.join(rocm, "include", "hip", "hip_runtime.h")):
        pytest.skip("no HIP headers on this box (sf_view_host.cpp includes them for their types)")
    exe = str(tmp_path / "view_band_dump")
    csrc = os.path.join(ROOT, "spacefortress_amd", "csrc")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", csrc, "-I", os.path.join(ROOT, "include"),
                           "-I", os.path.join(rocm, "include"), os.path.join(ROOT, "tests", "native", "view_band_dump.cpp"),
                           os.path.join(csrc, "sf_view_host.cpp"), "-o", exe])
    views = [v for _, v in _all_views()] + [E.SCORE_VIEW, E.BAR_SEAM_VIEW, E.BAR_CUT_VIEW]
    views += [E.View(w, 40, (0, 0, 1024, 40), 2.0, grey) for w in range(1, 1025) for grey in (True, False)]
    args = [str(x) for v in views for x in (v.W, v.H, *v.viewport, v.lw, int(v.grey))]
    out = subprocess.run([exe] + args, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    rec = [line.split() for line in out.stdout.splitlines()]
    assert len(rec) == len(views)
    for v, r in zip(views, rec):
        assert r[0] != "error", (v, r)
        assert [int(x) for x in r[:4]] == [v.W, v.H, 1 if v.grey else 3, E.band_h(v.W, 1 if v.grey else 3)], (v, r)


def test_found_a_hole_in_a_stroke(both):  # noqa: F811
    """FOUND (viewedges.py): the real cairo leaves pixel (20, 112) of this ship BLACK inside a fully covered stroke -- its span
    coverage is a uint8_t and GRID_AREA_TO_ALPHA gave 256 --; the model draws the same, and so does the kernels' formulation
    run on the host (sf_image_object_alpha), which both clamped to 255 before."""
    import ctypes as C
    import viewmodel as V
    from spacefortress_amd import _lib
    R, run = both
    view = E.VIEWS[E.HOLE_VIEW]
    saved = (R.W, R.H, R.VP_X, R.VP_Y, R.VP_W, R.VP_H, R.SX, R.SY, R.LINE_W, R.SCALE)
    V.set_view(view.W, view.H, view.viewport, view.lw)
    try:
        L = _lib.lib()
        for n, c in enumerate(E.HOLE_CENTRES):
            x, y = E.to_user(view, *c)
            got, real = run(R.s_begin() + R.s_wireframe(R.SHIP_LINES, (x, y), 305), view.W, view.H)
            assert np.array_equal(got, real), (c, np.argwhere(got != real)[:6].tolist())
            if n == 0:
                assert real[20, 112] == 0 and real[20, 111] == 163 and real[20, 113] == 255 and real[19, 112] == 255 and real[21, 112] == 255
            alpha = np.zeros((view.H, view.W), np.uint8)
            assert L.sf_image_object_alpha(0, x, y, 305, view.W, view.H, *[float(v) for v in view.viewport], view.lw,
                                           alpha.ctypes.data_as(C.c_void_p)) == 0
            assert np.array_equal(alpha, real), (c, np.argwhere(alpha != real)[:6].tolist())  # (white on black: the frame is the coverage)
    finally:
        R.W, R.H, R.VP_X, R.VP_Y, R.VP_W, R.VP_H, R.SX, R.SY, R.LINE_W, R.SCALE = saved


CAIRO_VIEWS = list(E.VIEWS) + list(E.GEOMETRIES)  # every surface the GPU tests compare on


@pytest.mark.parametrize("name", CAIRO_VIEWS)
def test_model_is_cairo_at_these_placements(both, O, hp, name):  # noqa: F811
    """One channel's draw script of a sample of every kind's placements -- hexagons and objects as the model's frame() builds
    them -- through the real cairo and through oracle/cairo_model.c: the same bytes."""
    import viewmodel as V
    R, run = both
    view = E.VIEWS[name] if name in E.VIEWS else E.geometry_view(name)
    snaps, places = E.join(E.seam_sweeps(O, view), E.edge_sweeps(O, view), E.dense(O, view), E.shell_decisions(O, view),
                           E.fort_decisions(O, view))
    saved = (R.W, R.H, R.VP_X, R.VP_Y, R.VP_W, R.VP_H, R.SX, R.SY, R.LINE_W, R.SCALE)
    V.set_view(view.W, view.H, view.viewport, view.lw)
    try:
        grey = lambda rgb, g: g  # noqa: E731
        seen = set()
        for i in list(range(0, len(places), 23)) + [i for i, p in enumerate(places) if p.kind in ("fort", "dead_fort")]:
            script = R.s_begin() + R.s_hexagon(hp[:12]) + R.s_hexagon(hp[12:]) + V._objects(snaps[i], grey)
            got, real = run(script, view.W, view.H)
            assert np.array_equal(got, real), (name, E.label(places[i]), np.argwhere(got != real)[:6].tolist())
            seen.add((places[i].kind, places[i].where.split()[0]))
        for kind in E.MOVERS:
            assert {(kind, w) for w in ("top", "bottom", "left", "right", "corner", "dense")} <= seen, (kind, seen)
        assert ("fort", "fort") in seen and ("dead_fort", "fort") in seen
    finally:
        R.W, R.H, R.VP_X, R.VP_Y, R.VP_W, R.VP_H, R.SX, R.SY, R.LINE_W, R.SCALE = saved
