#!/usr/bin/env python3
"""Frame fixtures of VIEWS (sf_render_view) from the reference's REAL renderer and its REAL Python extension.

Run in the build container only: needs the reference's sources and the image's cairo 1.16 (`make -C oracle refdraw refpy
cairoprobe`).  What is written is data -- engine states, the pixels the reference drew for them, a glyph atlas --, never
reference source; the libraries stay behind (oracle/_ref/ is git-ignored).

    python tests/golden/views/make_views_golden.py

    frames_<view>.npz  STATES drawn by Game(config, lw, grayscale, width, height, viewport).draw() (SRC/draw.cpp:256-270 through
                       oracle/_ref/libsfrefdraw.so): frames u8[n, H, W, 4], all four bytes of the RGB24 pixel (B, G, R, x) on
                       every row; view = (width, height, vp_x, vp_y, vp_w, vp_h, line width, grayscale); snaps, labels; the
                       view's glyph atlas (alpha, layout, x0) where cairo's text is an atlas there (atlas_of), else none
    atlas_unit.npz     the glyph atlas of 1.0 pixel per user unit in USER coordinates (viewport offset 0): the built-in one of
                       sf_glyphs.h (kUnit*), taken in both native views
    ext_<run>.npz      the real extension _spacefortress.Game(config, viewport=(130, 80, 450, 460), lw=2, grayscale=False)
                       replaying the keys of a recorded run as SSF_Env.step does: pb_pixels, pb_width, pb_height every EXT_EVERY
                       ticks (and the last) -- the public surface itself
"""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.dirname(HERE)
ROOT = os.path.dirname(GOLDEN)
ROOT = os.path.dirname(ROOT)
REFDIR = os.path.join(ROOT, "oracle", "_ref")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(GOLDEN, "frames"))

from oracle import oracle as O  # noqa: E402

GUI = (130, 80, 450, 460)
# name -> (width, height, viewport, line width, grayscale)
VIEWS = {
    "gui": (450, 460, GUI, 2.0, 0),             # spacefortress.game's human-play view (and its video), colour
    "game": (710, 626, (0, 0, 710, 626), 2.0, 0),  # Game(config)'s defaults
    "gui_grey": (450, 460, GUI, 2.0, 1),
    "s077": (int(450 * .77), int(460 * .77), GUI, 2.0, 0),  # the circle: one Bezier segment per half ...
    "s078": (int(450 * .78), int(460 * .78), GUI, 2.0, 0),  # ... and two
    "aniso": (300, 400, GUI, 2.0, 0),          # w / vw != h / vh
}
POSES = ["ship_explosion_3", "fort_explosion_0", "fort_explosion_1", "crowd_0", "crowd_5", "crowd_14",
         "bar_12_0", "border_1", "border_3", "fort_heading_0", "score_1234567", "score_-99999"]
SCENARIOS = 3       # youturn states of scenarios.npz, evenly spread
RUNS = ["youturn_deaths", "autoturn_destroy"]
EXT_EVERY = 61


def draw4(g, view):
    """The four bytes of every pixel of the RGB24 surface the reference's draw() leaves: [H, W, 4]."""
    w, h, vp, ls, grey = view
    out = np.zeros((4, h, w), np.uint8)
    for c in range(4):
        assert g.L.sfref_draw_geom(g.h, w, h, int(vp[0]), int(vp[1]), int(vp[2]), int(vp[3]), float(ls), int(grey), c,
                                   out[c].ctypes.data_as(ctypes.c_void_p)) == 0
    return np.ascontiguousarray(out.transpose(1, 2, 0))


def atlas(P, M, view):
    """The view's glyph atlas from the real cairo (make_score_golden.atlas_of), or None where cairo's text is no atlas there."""
    w, h, vp, ls, _ = view
    real_surface = M.surface
    M.surface = lambda geom: (w, h, w / vp[2], h / vp[3], float(vp[0]), float(vp[1]))
    try:
        return M.atlas_of(P, (None, vp, ls))
    except AssertionError:
        return None
    finally:
        M.surface = real_surface


def states():
    z = np.load(os.path.join(GOLDEN, "frames", "poses.npz"))
    labels = [str(s) for s in z["labels"]]
    snaps = [z["snaps"][labels.index(k)] for k in POSES]
    names = list(POSES)
    s = np.load(os.path.join(GOLDEN, "frames", "scenarios.npz"))
    yt = np.flatnonzero(s["gametype"] == 0)
    for i in yt[np.linspace(0, len(yt) - 1, SCENARIOS + 2).astype(int)[1:-1]]:
        snaps.append(s["snaps"][i])
        names.append(str(s["labels"][i]))
    out = np.zeros(len(snaps), O.SNAPSHOT_DTYPE)  # (field by field: the record's padding stays zero, the file reproducible)
    for i, s in enumerate(snaps):
        for f in O.SNAPSHOT_DTYPE.names:
            out[i][f] = s[f]
    return out, names


def extension_runs():
    if os.environ.get("MALLOC_PERTURB_") != "255":  # (as make_getters_golden.py: the same allocator state, the same runs)
        env = dict(os.environ, MALLOC_PERTURB_="255")
        sys.exit(subprocess.call([sys.executable, os.path.abspath(__file__), "--ext"], env=env))
    sys.path.insert(0, REFDIR)
    import _spacefortress as sf
    libc = ctypes.CDLL(None)
    libc.initstate.restype = ctypes.c_void_p
    libc.initstate.argtypes = [ctypes.c_uint, ctypes.c_char_p, ctypes.c_size_t]
    keep = []
    for name in RUNS:
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        meta = json.loads(str(z["meta"]))
        gt, youturn = meta["gametype"], meta["gametype"] in ("youturn", "test-youturn")
        rng = ctypes.create_string_buffer(128)
        keep.append(rng)
        libc.initstate(meta["seed"], rng, 128)
        kw = dict(viewport=GUI, lw=2, grayscale=False)
        for _ in range(meta["spawn_skip"]):
            sf.Game(gt, **kw)
        g = sf.Game(gt, **kw)
        frames, ticks = [], []
        T = len(z["keys"])
        for t in range(T):
            keys = int(z["keys"][t])
            (g.press_key if keys & 1 else g.release_key)(sf.FIRE_KEY)  # ENV:213-229
            (g.press_key if keys & 2 else g.release_key)(sf.THRUST_KEY)
            if youturn:
                (g.press_key if keys & 4 else g.release_key)(sf.LEFT_KEY)
                (g.press_key if keys & 8 else g.release_key)(sf.RIGHT_KEY)
            assert g.step_one_tick(34) == z["eng_reward"][t], (name, t)
            if t % EXT_EVERY == EXT_EVERY - 1 or t == T - 1:
                g.draw()
                frames.append(np.frombuffer(g.pb_pixels, np.uint8).copy())
                ticks.append(t)
            assert not g.is_game_over() or t == T - 1, (name, t)
        assert (g.pb_width, g.pb_height) == (450, 460)
        np.savez_compressed(os.path.join(HERE, "ext_%s.npz" % name), pb_pixels=np.array(frames, np.uint8), ticks=np.array(ticks, np.int64),
                            pb_width=np.int64(g.pb_width), pb_height=np.int64(g.pb_height),
                            meta=json.dumps(dict(run=name, gametype=gt, seed=meta["seed"], kwargs=dict(viewport=list(GUI), lw=2, grayscale=False),
                                                 every=EXT_EVERY)))
        print("ext_%s: %d frames" % (name, len(frames)))


def main():
    if "--ext" in sys.argv:
        extension_runs()
        return
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), "refdraw", "refpy", "cairoprobe"], stdout=subprocess.DEVNULL)
    import make_score_golden as M
    P = M.probe()
    g = O.RefDrawGame("youturn")
    snaps, names = states()
    for key, view in VIEWS.items():
        frames = []
        for s in snaps:
            g.load_snapshot(s)
            frames.append(draw4(g, view))
        out = dict(frames=np.array(frames, np.uint8), view=np.array([view[0], view[1]] + list(view[2]) + [view[3], view[4]], np.float64),
                   snaps=snaps, labels=np.array(names), meta=json.dumps(dict(cairo=g.cairo_version(), gametype="youturn")))
        A = atlas(P, M, view)
        if A is not None:
            out.update(alpha=A[0], layout=A[1], x0=A[2])
        np.savez_compressed(os.path.join(HERE, "frames_%s.npz" % key), **out)
        print("frames_%s: %d frames %s, atlas %s" % (key, len(frames), frames[0].shape, "yes" if A is not None else "none"))
    # the built-in atlas of 1.0 pixel per unit: the same bitmaps in both native views, layouts apart by the viewport's offset
    a0 = atlas(P, M, VIEWS["game"])
    a1 = atlas(P, M, VIEWS["gui"])
    assert np.array_equal(a0[0], a1[0]) and np.array_equal(a0[2] - GUI[0], a1[2]) and a0[1][3] - GUI[1] == a1[1][3]
    np.savez_compressed(os.path.join(HERE, "atlas_unit.npz"), alpha=a0[0], layout=a0[1], x0=a0[2])
    subprocess.check_call([sys.executable, os.path.abspath(__file__), "--ext"])


if __name__ == "__main__":
    main()
