"""Frames in a VIEW on the GPU (sf_render_view.hip behind SFVecEnv.render_view and spacefortress.core.Game) against the
reference: frames its own renderer drew in six views (tests/golden/views/frames_*.npz), what its real Python extension's
Game(config, viewport=(130, 80, 450, 460), lw=2, grayscale=False) left in pb_pixels while replaying recorded runs
(ext_*.npz), and the per-channel CPU model (tests/viewmodel.py, itself equal to those frames) on played batches.
Bar: every byte of every pixel -- the score text included wherever the view has a glyph atlas."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN
from lockstep import load_state as _load, sfa

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

VIEWS = os.path.join(GOLDEN, "views")
GUI = (130, 80, 450, 460)
FRAME_VIEWS = ["gui", "game", "gui_grey", "s077", "s078", "aniso"]


def _same(got, want, what):
    if not np.array_equal(got, want):
        d = np.argwhere(got != want)
        raise AssertionError((what, int((got != want).sum()), d[:6].tolist()))


def _unit_view(w, h, vp):
    return vp[2] == w and vp[3] == h and float(vp[0]).is_integer() and float(vp[1]).is_integer()


@pytest.mark.parametrize("name", FRAME_VIEWS)
def test_views_equal_the_references_frames(sfa, name):
    """Fixture states into lanes (set_field), render_view in the fixture's view: all four bytes of every pixel equal what
    SRC/draw.cpp + cairo 1.16 drew, every row -- the text from the built-in atlas at 1.0 pixel per unit, else from the fixture's
    atlas; a view without either is compared below its text rows (the seven-segment fallback equals no reference pixels).
    Every row: gui, game, gui_grey (the built-in atlas).  Below the text: s077, s078, aniso -- cairo's text is no whole-pixel
    atlas there (make_score_golden.atlas_of finds none), so the fallback and whatever lies under the text go unchecked in them."""
    import viewmodel as V
    z = np.load(os.path.join(VIEWS, "frames_%s.npz" % name))
    w, h, vp, lw, grey = V.fixture_view(z)
    want = z["frames"]
    env = sfa.SFVecEnv(len(want), gametype="youturn", obs_type="features")
    _load(env, z["snaps"])
    A = None if _unit_view(w, h, vp) else V.fixture_glyphs(z)
    rows = 0 if (A is not None or _unit_view(w, h, vp)) else V.text_rows(h, vp)
    got = env.render_view(w, h, vp, lw, grey, glyphs=A).cpu().numpy()
    assert got.shape == want.shape
    for i in range(len(want)):
        _same(got[i, rows:], want[i, rows:], (name, str(z["labels"][i])))
    rgb = env.render_view(w, h, vp, lw, grey, format="rgb", glyphs=A).cpu().numpy()
    _same(rgb, got[..., 2::-1], (name, "rgb"))
    if grey:
        _same(env.render_view(w, h, vp, lw, grey, format="gray", glyphs=A).cpu().numpy(), got[..., 0], (name, "gray"))
    env.close()


def _drive(g, keys, youturn):
    import spacefortress.core as sf
    (g.press_key if keys & 1 else g.release_key)(sf.FIRE_KEY)  # ENV:213-229
    (g.press_key if keys & 2 else g.release_key)(sf.THRUST_KEY)
    if youturn:
        (g.press_key if keys & 4 else g.release_key)(sf.LEFT_KEY)
        (g.press_key if keys & 8 else g.release_key)(sf.RIGHT_KEY)


@pytest.mark.parametrize("run", ["youturn_deaths", "autoturn_destroy"])
def test_game_view_replays_the_real_extension(sfa, run):
    """spacefortress.core.Game(config, viewport=(130, 80, 450, 460), lw=2, grayscale=False) -- the human-play front-end's
    Game -- replays a recorded run's keys; pb_pixels, pb_width and pb_height equal the real extension's at every recorded tick."""
    import spacefortress.core as sf
    e = np.load(os.path.join(VIEWS, "ext_%s.npz" % run))
    em = json.loads(str(e["meta"]))
    z = np.load(os.path.join(GOLDEN, run + ".npz"))
    meta = json.loads(str(z["meta"]))
    youturn = meta["gametype"] in ("youturn", "test-youturn")
    g = sf.Game(meta["gametype"], seed=meta["seed"], **dict(em["kwargs"], viewport=tuple(em["kwargs"]["viewport"])))
    assert (g.pb_width, g.pb_height) == (int(e["pb_width"]), int(e["pb_height"])) == (450, 460)
    ticks = [int(t) for t in e["ticks"]]
    k = 0
    for t, keys in enumerate(z["keys"]):
        _drive(g, int(keys), youturn)
        assert g.step_one_tick(34) == int(z["eng_reward"][t]), t
        if k < len(ticks) and t == ticks[k]:
            g.draw()
            px = np.frombuffer(g.pb_pixels, np.uint8)
            _same(px.reshape(460, 450, 4), e["pb_pixels"][k].reshape(460, 450, 4), (run, t))
            k += 1
    assert k == len(ticks)
    g.close()
    d = sf.Game("youturn")  # the reference's defaults: the config's 710 x 626, colour
    assert (d.pb_width, d.pb_height) == (710, 626) and len(d.pb_pixels) == 710 * 626 * 4
    px = np.frombuffer(d.pb_pixels, np.uint8).reshape(626, 710, 4)
    assert (px[..., 3] == 255).all() and px[..., 1].max() == 255 and px[..., 0].max() < 255  # green hexagons, no blue stroke
    d.close()


def _snapshots(env):
    """The batch's state as oracle snapshot records: what the model draws."""
    from oracle import oracle as O
    n = env.num_envs
    f = {k: np.asarray(env.get_field(k)) for k in ("flags", "ship_x", "ship_y", "ship_angle", "fort_angle", "points", "vlner",
                                                   "fort_vuln_timer", "missile_mask", "missile_x", "missile_y", "missile_angle",
                                                   "shell_mask", "shell_x", "shell_y", "shell_vx", "shell_vy")}
    s = np.zeros(n, O.SNAPSHOT_DTYPE)
    s["ship_alive"], s["fort_alive"] = f["flags"] & 1, (f["flags"] >> 1) & 1
    for k in ("ship_x", "ship_y", "ship_angle", "fort_angle", "points", "vlner", "fort_vuln_timer"):
        s[k] = f[k]
    bits = 1 << np.arange(20, dtype=np.uint32)
    s["missile_alive"] = (f["missile_mask"][:, None] & bits[None, :]) != 0
    s["shell_alive"] = (f["shell_mask"][:, None] & bits[None, :]) != 0
    for k in ("missile_x", "missile_y", "missile_angle", "shell_x", "shell_y"):
        s[k] = f[k].T
    ang = np.degrees(np.arctan2(f["shell_vy"], f["shell_vx"])).T  # (the kernel's heading of a shell, SRC/game.cpp:159-173)
    s["shell_angle"] = np.where(ang < 0, ang + 360.0, ang)
    return s


def test_played_batch_views_equal_the_model(sfa):
    """1 024 lanes play sampled actions for 340 steps (deaths, explosions, shells); every 17th step the GUI view's colour
    frames of all lanes are drawn, and a dozen lanes -- the dead ships, the dead fortresses, the most shells first, two more --
    equal the per-channel CPU model with the built-in atlas, every byte (the model costs 50 ms a frame: not every lane).
    Random play all but never destroys the fortress, so four lanes have theirs destroyed through set_field at step 40 (the
    engine then plays its 1 000 ms explosion and the respawn)."""
    import viewmodel as V
    hp = np.load(os.path.join(GOLDEN, "tables.npz"))["hex_points"]
    unit = V.unit_glyphs(np.load(os.path.join(VIEWS, "atlas_unit.npz")), GUI)
    N, T = 1024, 340
    env = sfa.SFVecEnv(N, gametype="youturn", obs_type="features")
    env.reset()
    env.seed_actions(20261016)
    seen_dead = seen_fort = seen_shells = 0
    for t in range(T):
        env.step_sampled()
        if t == 40:
            flags, timer = env.get_field("flags"), env.get_field("fort_death_timer")
            flags[:4] &= ~np.uint8(2)  # (FL_FORT)
            timer[:4] = 0
            env.set_field("flags", flags)
            env.set_field("fort_death_timer", timer)
        if t % 17 != 16:
            continue
        s = _snapshots(env)
        dead, fort_dead = np.flatnonzero(s["ship_alive"] == 0), np.flatnonzero(s["fort_alive"] == 0)
        shells = np.argsort(-s["shell_alive"].sum(1), kind="stable")
        lanes = list(dict.fromkeys(int(i) for i in list(dead[:4]) + list(fort_dead[:3]) + list(shells[:3]) + [t % N, (7 * t) % N]))
        frames = env.render_view(viewport=GUI)
        assert frames.shape == (N, 460, 450, 4)
        got = dict(zip(lanes, frames[lanes].cpu().numpy()))
        seen_dead += len(dead) > 0
        seen_fort += len(fort_dead) > 0
        seen_shells += int(s["shell_alive"].sum() > 0)
        for i in lanes:
            _same(got[i], V.frame(s[i], hp, 450, 460, GUI, 2.0, False, glyphs=unit), (t, int(i)))
    assert seen_dead and seen_fort and seen_shells, (seen_dead, seen_fort, seen_shells)
    env.close()


def test_grey_view_at_the_wrappers_geometry_is_its_image(sfa):
    """At SSF_Env's geometry (90 x 92 of (130, 80, 450, 460), line width 3) in grey, with the batch's atlas, render_view is the
    frame kernel's image-raw observation byte for byte, on a played batch."""
    env = sfa.SFVecEnv(128, gametype="youturn", obs_type="image-raw")
    env.reset()
    env.seed_actions(7)
    for t in range(160):
        env.step_sampled()
        if t % 40 == 39:
            want = env.render("image-raw").cpu().numpy()
            got = env.render_view(90, 92, GUI, 3.0, True, format="gray", glyphs=env.score_glyphs()).cpu().numpy()
            _same(got, want, ("ssf geometry", t))
            bgrx = env.render_view(90, 92, GUI, 3.0, True, glyphs=env.score_glyphs()).cpu().numpy()
            _same(bgrx[..., :3], np.repeat(want[..., None], 3, axis=3), ("ssf geometry, bgrx", t))
    env.close()


def _wrapper_geometries():
    """(name, (scale, vx, vy, vw, vh, ls), snaps, atlas index of score_glyphs.npz or None): the four geometries of
    geometries.npz and the close-up of zoom.npz (scale .75, 187 x 195: a wireframe larger than one accumulator window of the
    rasteriser, arcs 47 pixels out), each with the fixture's states: dead ships, dead fortresses, missiles, shells."""
    z = np.load(os.path.join(GOLDEN, "frames", "geometries.npz"))
    out = [("geometry %d" % gi, tuple(float(v) for v in g), z["snaps"], gi + 1) for gi, g in enumerate(z["geometries"])]
    q = np.load(os.path.join(GOLDEN, "frames", "zoom.npz"))
    return out + [("close-up", tuple(float(v) for v in q["geometry"]), q["snaps"], None)]


def test_grey_view_at_any_wrapper_geometry_is_its_image(sfa):
    """The general renderer and the view kernel paint with the same code (sf_scene_dev.h); here they see the same states in
    every other geometry the fixtures have: an image-raw batch in the geometry, the fixture's snapshots in lanes 60 .. of 128
    (two state tiles), and render_view at the same size, viewport and line width, grey, cut into bands of at most 32 rows, is
    render("image-raw") byte for byte -- with the geometry's atlas where score_glyphs.npz has one, and with none (both draw the
    seven-segment fallback); the BGRx form is the grey one in B, G and R with x = 255."""
    from oracle import render_np as R
    first = 60
    for name, (sc, vx, vy, vw, vh, ls), snaps, atlas in _wrapper_geometries():
        n, vp = len(snaps), (vx, vy, vw, vh)
        lanes = range(first, first + n)
        env = sfa.SFVecEnv(128, gametype="youturn", obs_type="image-raw", image_geometry=(sc, vp, ls))
        h, w = env.obs_shape
        assert h > 32  # (more than one band)
        batch = snaps[np.arange(128) % n]
        batch[first:first + n] = snaps
        _load(env, batch)
        for A in ([R.load_glyphs(atlas)] if atlas is not None else []) + [None]:
            if A is None:
                env.set_score_glyphs(None)
            else:
                env.set_score_glyphs(A["alpha"], A["layout"], A["x0"])
            assert (env.score_glyphs() is None) == (A is None)
            what = (name, "atlas" if A is not None else "fallback")
            want = env.render("image-raw").cpu().numpy()[first:first + n]
            got = env.render_view(w, h, vp, ls, grayscale=True, format="gray", lanes=lanes, glyphs=env.score_glyphs()).cpu().numpy()
            assert got.shape == want.shape == (n, h, w)
            _same(got, want, what)
            bgrx = env.render_view(w, h, vp, ls, grayscale=True, lanes=lanes, glyphs=env.score_glyphs()).cpu().numpy()
            _same(bgrx[..., :3], np.repeat(want[..., None], 3, axis=3), what + ("bgrx",))
            assert (bgrx[..., 3] == 255).all(), what
        env.close()


def test_lane_ranges_and_a_view_changes_nothing(sfa):
    """A sub-range of lanes is the same lanes of the whole batch's frames; a batch that draws views every step keeps the same
    observations and the same state as its twin that never does -- an image batch and a features batch."""
    env = sfa.SFVecEnv(200, gametype="youturn", obs_type="features")
    env.reset()
    env.seed_actions(3)
    for _ in range(120):
        env.step_sampled()
    full = env.render_view(viewport=GUI).cpu().numpy()
    _same(env.render_view(viewport=GUI, lanes=range(70, 135)).cpu().numpy(), full[70:135], "range")
    _same(env.render_view(viewport=GUI, lanes=199).cpu().numpy(), full[199:], "last lane")
    out = torch.zeros((3, 460, 450, 4), dtype=torch.uint8, device=env.device)
    env.render_view(viewport=GUI, lanes=range(0, 3), out=out)
    _same(out.cpu().numpy(), full[:3], "out")
    env.close()
    for obs_type in ("image-raw", "features"):
        a = sfa.SFVecEnv(96, gametype="youturn", obs_type=obs_type)
        b = sfa.SFVecEnv(96, gametype="youturn", obs_type=obs_type)
        a.reset(), b.reset()
        a.seed_actions(11), b.seed_actions(11)
        for t in range(150):
            oa = a.step_sampled()[0].cpu().numpy()
            a.render_view(viewport=GUI, grayscale=t % 2 == 0, format="rgb")
            ob = b.step_sampled()[0].cpu().numpy()
            _same(oa, ob, (obs_type, t))
        sa, sb = a.state_dict(), b.state_dict()
        for k in sa:
            assert np.asarray(sa[k]).tobytes() == np.asarray(sb[k]).tobytes(), (obs_type, k)
        a.close(), b.close()


def test_refusals_are_errors_not_faults(sfa):
    env = sfa.SFVecEnv(64, gametype="youturn", obs_type="features")
    env.reset()
    with pytest.raises(ValueError, match="1.0 pixel"):
        env.render_view(451, 460, GUI)
    with pytest.raises(ValueError):
        env.render_view(2000, 10, (0, 0, 4000, 4000))
    with pytest.raises(ValueError):
        env.render_view(viewport=(0, 0, 0, 100))
    with pytest.raises(ValueError):
        env.render_view(viewport=GUI, lw=0)
    with pytest.raises(ValueError):
        env.render_view(viewport=GUI, format="gray")
    with pytest.raises(ValueError):
        env.render_view(viewport=GUI, lanes=range(60, 70))
    with pytest.raises(ValueError):
        env.render_view(viewport=GUI, lanes=64)
    with pytest.raises(ValueError):
        env.render_view(viewport=GUI, out=torch.zeros((64, 460, 450, 3), dtype=torch.uint8, device=env.device))
    f = env.render_view(viewport=GUI, lanes=range(0, 2)).cpu().numpy()  # the device is fine
    torch.cuda.synchronize()
    assert f.shape == (2, 460, 450, 4) and (f[..., 3] == 255).all()
    env.close()
