"""The two run-time-geometry frame kernels (sf_render_view.hip, sf_render_generic.hip: one painter, sf_scene_dev.h) at the
places play almost never produces: every object carried in 1/16-pixel steps to every seam between a view's bands, from both
sides, to every side and corner of the surface from wholly outside to inside, onto every row of a small view; the decisions of
the draw order at their thresholds; the 84 x 84 resample across its size contract.  The placements are tests/viewedges.py's
(one object per lane on a quiet base state, so a mismatch names its object); the reference is the CPU model
(tests/viewmodel.py, oracle/render_np.py over oracle/cairo_model.c, held to the real cairo at these placements by
tests/test_view_edges_model.py).  Bar: every byte.  Every placement of a test is a lane of one batch: one or two launches, and
the model's frames (0.2 .. 0.9 ms each, profiles/view_edge_tests.md) are the cost; every placement is modelled."""
import os

import numpy as np
import pytest

import viewedges as E
from conftest import GOLDEN
from lockstep import load_state, sfa  # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

GAMETYPE = "youturn"


@pytest.fixture(scope="module")
def O():
    from oracle import oracle as O
    O.oracle_lib()
    return O


@pytest.fixture(scope="module")
def hp():
    return np.load(os.path.join(GOLDEN, "tables.npz"))["hex_points"]


@pytest.fixture(scope="module")
def atlas_unit():
    return np.load(os.path.join(GOLDEN, "views", "atlas_unit.npz"))


def _same(got, want, what):
    if not np.array_equal(got, want):
        d = np.argwhere(got != want)
        raise AssertionError((what, int((got != want).sum()), d[:6].tolist()))


def _model_glyphs(view, atlas_unit):
    """(the model's atlas, rows hidden from the comparison).  A unit view at a whole offset has the built-in atlas on the device
    and atlas_unit.npz in the model -- left out of the model where the text's box lies wholly off the surface (it then draws
    nothing; its per-pixel Python loop is most of a small frame's time); any other view draws the seven-segment fallback, which
    equals no reference pixels: its rows are hidden, and the caller sees to it that no object under test is in them."""
    import viewmodel as V
    if not E.unit_view(view):
        return None, E.masked_rows(view)
    A = V.unit_glyphs(atlas_unit, view.viewport)
    gw, gh, adv, y0 = A["layout"]
    return (A if y0 < view.H and y0 + gh > 0 else None), 0


def _check_view(sfa, O, hp, atlas_unit, view, snaps, places, what):
    """The batch's frames in the view against the model, every placement, every (unhidden) row; each placement's model frame
    against the base frame as its `expect` says; rgb and gray against the bgrx bytes."""
    import viewmodel as V
    A, rows = _model_glyphs(view, atlas_unit)
    E.assert_clear_of_rows(view, places, rows)
    env = sfa.SFVecEnv(len(snaps), gametype=GAMETYPE, obs_type="features")
    load_state(env, snaps)
    args = (view.W, view.H, view.viewport, view.lw, view.grey)
    dev = env.render_view(*args)
    assert tuple(dev.shape) == (len(snaps), view.H, view.W, 4)
    assert torch.equal(env.render_view(*args, format="rgb"), dev[..., [2, 1, 0]]), (what, "rgb")
    if view.grey:
        assert torch.equal(env.render_view(*args, format="gray"), dev[..., 0]), (what, "gray")
    got = dev.cpu().numpy()
    env.close()
    base = V.frame(E.base(O, view, 1)[0], hp, *args, glyphs=A)
    for i, p in enumerate(places):
        want = V.frame(snaps[i], hp, *args, glyphs=A)
        _same(got[i, rows:], want[rows:], (what, E.label(p)))
        differs = not np.array_equal(want, base)
        assert p.expect == "either" or differs == (p.expect == "ink"), (what, "the model shows", differs, E.label(p))


@pytest.mark.parametrize("kind", E.MOVERS)
@pytest.mark.parametrize("name", list(E.VIEWS))
def test_movers_at_seams_edges_and_every_row(sfa, O, hp, atlas_unit, name, kind):
    """(a) + (b) + (c): one mover in one view -- its seam sweeps, its edge and corner sweeps, its dense pass over the rows."""
    view = E.VIEWS[name]
    snaps, places = E.join(E.seam_sweeps(O, view, (kind,)), E.edge_sweeps(O, view, (kind,)), E.dense(O, view, (kind,)))
    _check_view(sfa, O, hp, atlas_unit, view, snaps, places, (name, kind))


@pytest.mark.parametrize("name", list(E.VIEWS))
def test_fortress_headings_and_the_shells_distance(sfa, O, hp, atlas_unit, name):
    """(d): the live fortress at every heading of the sweeps (in the 112 x 80 views its tip at heading 90 reaches one row past
    seam 64: the longest wireframe stroke there is, the one the painter's cull margin has to cover;
    test_view_edges_model.test_fortress_tip_crosses_a_seam_by_one_row), destroyed, and a shell at
    21 units from it, an ulp either side, on the axes and a diagonal."""
    view = E.VIEWS[name]
    snaps, places = E.join(E.fort_decisions(O, view), E.shell_decisions(O, view))
    _check_view(sfa, O, hp, atlas_unit, view, snaps, places, (name, "fortress"))


def test_found_a_hole_in_a_stroke_and_the_wide_circle(sfa, O, hp, atlas_unit):
    """The placements that failed when these tests were first run (viewedges.py: FOUND), by name, through the view kernel."""
    view = E.VIEWS[E.HOLE_VIEW]
    snaps, places = E.named(O, view, "hole in a stroke", [("ship", 305) + E.to_user(view, *c) for c in E.HOLE_CENTRES])
    _check_view(sfa, O, hp, atlas_unit, view, snaps, places, "hole in a stroke")
    view = E.VIEWS["fort112_lw45"]
    snaps, places = E.named(O, view, "wide circle", [("dead_ship", None) + c for c in E.WIDE_CIRCLE_UNIT])
    _check_view(sfa, O, hp, atlas_unit, view, snaps, places, "wide circle")


@pytest.mark.parametrize("which", ["score", "bar across a seam", "bar cut by the bottom edge"])
def test_score_and_bar_across_a_seam_and_an_edge(sfa, O, hp, atlas_unit, which):
    """(d): the score's seven characters at every length and sign in a unit view whose rows put the glyphs across seam 32 and
    whose sides cut the text; the bar empty, part, full and past full with the timer either side of 250, across seam 32 (in
    colour: grey in every plane) and cut by the bottom edge."""
    import viewmodel as V
    if which == "score":
        view = E.SCORE_VIEW
        snaps, places = E.score_decisions(O, view)
        A = V.unit_glyphs(atlas_unit, view.viewport)
        y0, gh = A["layout"][3], A["layout"][1]
        assert y0 < 32 < y0 + gh and A["x0"].min() < 0 and A["x0"].max() + 6 * A["layout"][2] + A["layout"][0] > view.W
    else:
        view = E.BAR_SEAM_VIEW if which == "bar across a seam" else E.BAR_CUT_VIEW
        snaps, places = E.bar_decisions(O, view)
        top, bottom = 522 - view.viewport[1], 532 - view.viewport[1]
        assert (top < 32 < bottom and 32 in E.seams(view)) if which == "bar across a seam" else top < view.H < bottom
    _check_view(sfa, O, hp, atlas_unit, view, snaps, places, which)
    # the states that must differ from each other do: every pair of distinct scores; the bar's lengths and its kill colour
    args = (view.W, view.H, view.viewport, view.lw, view.grey)
    frames = [V.frame(s, hp, *args, glyphs=V.unit_glyphs(atlas_unit, view.viewport)).tobytes() for s in snaps]
    if which == "score":
        assert len(set(frames)) == len(frames)
    else:
        by = {p.side: f for p, f in zip(places, frames)}
        assert by["vlner 10 timer 249"] == by["vlner 10 timer 251"] != by["vlner 1 timer 249"] != by["vlner 0 timer 249"]
        assert by["vlner 11 timer 249"] != by["vlner 11 timer 250"] == by["vlner 11 timer 251"] == by["vlner 10 timer 250"]
        assert by["vlner %d timer 249" % E.BAR_MAX] == by["vlner 11 timer 249"]


# ---------------------------------------------------------------- the general renderer
def _resize_batch(frames, dsize=84):
    """oracle/render_np.py's resize_area (OpenCV's INTER_AREA: the same tables, the same float32 sums in the same order) over
    a batch of frames at once.  test_general_renderer holds it to resize_area itself on a sample."""
    from oracle import render_np as R
    n, sh, sw = frames.shape
    src = frames.astype(np.float32)
    tmp = np.zeros((n, sh, dsize), np.float32)
    for dx, sx, alpha in R.area_tab(sw, dsize):
        tmp[:, :, dx] += src[:, :, sx] * alpha
    out = np.zeros((n, dsize, dsize), np.float32)
    first = set()
    for dy, sy, beta in R.area_tab(sh, dsize):
        if dy in first:
            out[:, dy] += beta * tmp[:, sy]
        else:
            out[:, dy] = beta * tmp[:, sy]
            first.add(dy)
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


@pytest.mark.parametrize("kind", E.MOVERS + ("decisions",))
@pytest.mark.parametrize("name", list(E.GEOMETRIES))
def test_general_renderer_at_edges_and_decisions(sfa, O, hp, name, kind):
    """(b) and (d) through image_geometry=: image-raw against the model and image against resize_area of the model's frame,
    every placement; and the view kernel at the same size, viewport and line width, grey, gives the device's own image-raw
    bytes (two kernels, one painter, two band arrangements)."""
    from oracle import render_np as R
    sc, vp, ls, atlas = E.GEOMETRIES[name]
    view = E.geometry_view(name)
    if kind == "decisions":
        snaps, places = E.join(E.fort_decisions(O, view), E.shell_decisions(O, view), E.bar_decisions(O, view), E.score_decisions(O, view),
                               E.named(O, view, "wide circle", [("dead_ship", None) + c for c in E.WIDE_CIRCLE_CLOSE_UP]))
    else:
        snaps, places = E.edge_sweeps(O, view, (kind,))
    A = R.load_glyphs(atlas) if atlas is not None else None
    rows = 0 if A is not None else E.masked_rows(view)
    if A is None:
        E.assert_clear_of_rows(view, places, rows)
        assert rows == 0  # (the close-up starts below the text: nothing is hidden, the score's placements draw nothing)
    env = sfa.SFVecEnv(len(snaps), gametype=GAMETYPE, obs_type="image-raw", image_geometry=(sc, vp, ls))
    assert tuple(env.obs_shape) == (view.H, view.W)
    if A is not None:
        env.set_score_glyphs(A["alpha"], A["layout"], A["x0"])
    load_state(env, snaps)
    raw = env.render("image-raw")
    small = env.render("image").cpu().numpy()[:, 0]
    via_view = env.render_view(view.W, view.H, vp, ls, grayscale=True, format="gray", glyphs=env.score_glyphs())
    assert torch.equal(via_view, raw), (name, kind, "view kernel != general renderer", torch.nonzero((via_view != raw).flatten(1).any(1))[:6].tolist())
    raw = raw.cpu().numpy()
    env.close()
    prev = R.set_geometry(sc, vp, ls)
    try:
        hb, hs = hp[:12], hp[12:]
        base = R.render_raw(E.base(O, view, 1)[0], hb, hs, text=A is not None, glyphs=A)
        want = np.stack([R.render_raw(s, hb, hs, text=A is not None, glyphs=A) for s in snaps])
    finally:
        R.set_geometry(*prev)
    for i, p in enumerate(places):
        _same(raw[i, rows:], want[i, rows:], (name, "image-raw", E.label(p)))
        differs = not np.array_equal(want[i], base)
        assert p.expect == "either" or differs == (p.expect == "ink"), (name, "the model shows", differs, E.label(p))
    want_small = _resize_batch(want)
    for i in range(0, len(want), max(1, len(want) // 3)):
        _same(want_small[i], R.resize_area(want[i]), (name, "the batched resample is not resize_area", i))
    for i, p in enumerate(places):
        _same(small[i], want_small[i], (name, "image", E.label(p)))


# (W, H) of the resample's contract -- every W, H in [84, 251] with W * H <= 49152 -- and a geometry that gives exactly it
RESAMPLE = [
    ((84, 84), (0.5, (271, 231, 168, 168), 3)),
    ((85, 251), (0.5, (270, 64, 170, 502), 3)),
    ((251, 85), (0.5, (104, 230, 502, 170), 3)),
    ((168, 126), (0.5, (187, 189, 336, 252), 3)),
    ((251, 195), (0.5, (104, 120, 502, 390), 2)),
    ((97, 101), (0.5, (258, 214, 194, 202), 3)),
    ((131, 89), (0.6, (246, 241, 219, 149), 3)),    # (sx = 131 / 219, sy = 89 / 149: not the scale itself)
    ((173, 249), (0.7, (231, 137, 248, 356), 2)),   # (int(248 * .7) = 173, int(356 * .7) = 249)
]


@pytest.mark.parametrize("size,geometry", RESAMPLE, ids=["%dx%d" % s for s, _ in RESAMPLE])
def test_resample_across_the_size_contract(sfa, O, hp, size, geometry):
    """The 84 x 84 INTER_AREA resample of the general renderer (per-batch tap tables, four pixels and one 32-bit store per
    thread) at the corners of its size contract and at odd sizes: the device's `image` frame is resize_area of the device's OWN
    image-raw frame, exactly, on busy states; and the raw frame equals the model on a sample of them."""
    from oracle import render_np as R
    sc, vp, ls = geometry
    view = E.View(int(vp[2] * sc), int(vp[3] * sc), vp, float(ls), True)
    assert (view.W, view.H) == size and 84 <= min(size) and max(size) <= 251 and size[0] * size[1] <= 49152
    snaps, places = E.join(E.fort_decisions(O, view), E.dense(O, view, ("dead_ship", "ship"), frac=0.31))
    snaps, places = snaps[::7].copy(), places[::7]
    # busy: every lane also gets a dead fortress or a full bar, points, and a second object from its neighbour
    snaps["vlner"], snaps["points"] = np.arange(len(snaps)) % 12, (np.arange(len(snaps)) * 37) % 1000
    for i in range(len(snaps)):
        if i % 3 == 0:
            E.put(snaps, i, "dead_fort", 0, 0, None)
        x, y = E.to_user(view, view.W * ((i * 0.37) % 1.0), view.H * ((i * 0.61) % 1.0))
        E.put(snaps, i, "missile", x, y, (i * 47) % 360)
        E.put(snaps, i, "shell", x + 40, y - 30, (i * 29) % 360)
    env = sfa.SFVecEnv(len(snaps), gametype=GAMETYPE, obs_type="image", image_geometry=(sc, vp, ls))
    load_state(env, snaps)
    raw = env.render("image-raw").cpu().numpy()
    small = env.render("image").cpu().numpy()[:, 0]
    env.close()
    assert raw.shape == (len(snaps), view.H, view.W) and len(set(f.tobytes() for f in raw)) == len(raw)
    want = _resize_batch(raw)
    _same(want[0], R.resize_area(raw[0]), (size, "the batched resample is not resize_area"))
    _same(want[-1], R.resize_area(raw[-1]), (size, "the batched resample is not resize_area"))
    _same(small, want, (size, "image != resize_area(image-raw)"))
    rows = E.masked_rows(view)  # (no atlas for these geometries: the fallback's rows are not the model's)
    prev = R.set_geometry(sc, vp, ls)
    try:
        for i in range(0, len(snaps), max(1, len(snaps) // 6)):
            _same(raw[i, rows:], R.render_raw(snaps[i], hp[:12], hp[12:], text=False)[rows:], (size, "image-raw", i))
    finally:
        R.set_geometry(*prev)
