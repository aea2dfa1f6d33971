"""The draw record's decisions (sf_drawrec.h: make_header, hud_flags_near, hud_rows_near; the step kernel's three routes to
the projectile flags) held to the independent model of tests/drawrec_np.py AT THEIR EDGES, on image batches.

Every directed sweep targets one decision: one mover (a live ship, a dead ship's explosion, a missile, a shell), one target
box, one side of it.  192 envs stand along the side's normal at (2 k + 1) / 128 px, k = -96 .. 95, around the place where the
mover's box edge meets the target's edge as the model computes it: +- 1.5 px in steps of 1 / 64, none of them a tie.  Three
checks on every batch:
  (a) the bytes of draw_records(from_state=True) equal the model's -- header and live bytes -- for every env that is no tie;
  (b) the frames of the product batch equal, byte for byte and in both sizes, those of a batch that draws everything in place
      (SFMI_NO_EXPLOSION_CACHE, SFMI_NO_RENDER_ORDER), ties included;
  (c) the frames equal the numpy renderer's (oracle/render_np.py) at the ends of every sweep line, on both sides of every change
      of header words 3..5 along it, and on the deliberate ties (the centre of a sweep and its float32 neighbours).
Every comparison is exact.  profiles/drawrec_tests.md has the counts, the times and the mutations each test catches."""
import math

import numpy as np
import pytest

import drawrec_np as D
from lockstep import load_state, missile_table, sfa  # noqa: F401  (sfa: a fixture)
from sfcompare import compare_state, mask_bits

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GAMETYPE = "youturn"
K = np.arange(-96, 96)
OFFS = (2 * K + 1) / 128.0          # px along the normal; in user units 5 (2 k + 1) / 128, exact
NEAR = 3 / 128.0                    # "just inside" a corner, tangentially
PARK = (480.0, 300.0)               # a ship here is far from every threshold: 64.6..75.4 x 38.6..49.4 px
MAX_MODEL_FRAMES = 250
SHELL_SPEED = 6.0

TEXT, BAR = D.TEXT_BOX, D.BAR_BOX
WTEXT, WBAR, WFP = D.widened(TEXT), D.widened(BAR), D.widened(D.FORT_PIC_BOX)
WFE = D.widened(D.explosion_box(*D.FORT))
OBJ_FORT = (D.W_OBJMASK, 2)
# mover -> [(target box, its name, fortress alive, (header word, mask) of the decision)]
TARGETS = {
    "ship": [(TEXT, "text", 1, (D.W_FLAGS, D.F_NEAR_TEXT)), (WTEXT, "wtext", 1, (D.W_FLAGS, D.F_OTHER_TEXT)),
             (BAR, "bar", 1, (D.W_FLAGS, D.F_NEAR_BAR)), (WBAR, "wbar", 1, (D.W_FLAGS, D.F_OTHER_BAR)),
             (WFP, "wfp", 1, OBJ_FORT), (WFE, "wfe", 0, (D.W_FLAGS, D.F_FORT_EX_PLACE))],
    # (a dead ship's explosion is compared with the widened boxes only)
    "dead": [(WTEXT, "wtext", 1, (D.W_FLAGS, D.F_EX_TEXT)), (WBAR, "wbar", 1, (D.W_FLAGS, D.F_EX_BAR)),
             (WFP, "wfp", 1, OBJ_FORT), (WFE, "wfe", 0, (D.W_FLAGS, D.F_FORT_EX_PLACE))],
    "missile": [(TEXT, "text", 1, (D.W_FLAGS, D.F_NEAR_TEXT)), (WTEXT, "wtext", 1, (D.W_FLAGS, D.F_OTHER_TEXT)),
                (BAR, "bar", 1, (D.W_FLAGS, D.F_NEAR_BAR)), (WBAR, "wbar", 1, (D.W_FLAGS, D.F_OTHER_BAR))],
}
TARGETS["shell"] = TARGETS["missile"]
EXT = {"ship": D.SHIP_EXT, "dead": D.EXPLOSION_EXT, "missile": D.MISSILE_EXT, "shell": D.SHELL_EXT}
LINES_OF = {"ship": "SHIP_LINES", "missile": "MISSILE_LINES", "shell": "SHELL_LINES"}
HUD = ((0, 0), (37, 4), (0, 4), (37, 0))  # (points, vlner) by line: the baked route and the picture route


@pytest.fixture(scope="module")
def model():
    import os

    from conftest import GOLDEN
    from oracle import render_np as R

    z = np.load(os.path.join(GOLDEN, "tables.npz"))
    hb, hs = z["hex_points"][:12], z["hex_points"][12:]
    return R, hb, hs, R.background(hb, hs)


@pytest.fixture(scope="module")
def headings(model):
    """mover -> the heading that puts the most ink toward (left, top, right, bottom), measured on the renderer model"""
    R = model[0]
    return {m: D.worst_headings(R, getattr(R, n)) for m, n in LINES_OF.items()}


def frames_equal(got, want, what):
    if not np.array_equal(got, want):
        d = np.abs(got.astype(np.int32) - want.astype(np.int32))
        raise AssertionError((what, int(d.max()), int((d > 0).sum()), np.argwhere(d > 0)[:6].tolist()))


# ---------------------------------------------------------------- sweeps

def user(gx, gy):
    return D.VP_X + 5.0 * np.asarray(gx, np.float64), D.VP_Y + 5.0 * np.asarray(gy, np.float64)


def f32_neighbours(v):
    v32 = np.float32(v)
    return [float(np.nextafter(v32, np.float32(-np.inf))), float(v32), float(np.nextafter(v32, np.float32(np.inf)))]


def sweep_lines(mover, headings):
    """The lines of one mover: dicts of name, x / y (user units, 192 grid places), ux / uy (the three deliberate ties), heading,
    fortress alive, the targeted (word, mask)."""
    e = EXT[mover]
    lines = []
    for box, bname, fort_alive, target in TARGETS[mover]:
        x0, y0, x1, y1 = box
        # where the mover's box edge meets a side, and the inward direction: side -> (axis, centre in px, sign)
        sides = {"left": (0, x0 - e, +1), "right": (0, x1 + e, -1), "top": (1, y0 - e, +1), "bottom": (1, y1 + e, -1)}
        tang = {0: [("mid", (y0 + y1) / 2 + 1 / 128.0), ("low", y0 - e + NEAR), ("high", y1 + e - NEAR)],
                1: [("mid", (x0 + x1) / 2 + 1 / 128.0), ("low", x0 - e + NEAR), ("high", x1 + e - NEAR)]}
        todo = []
        for si, (side, (axis, c, sign)) in enumerate(sides.items()):
            for tname, t in tang[axis]:
                g = [None, None]
                g[axis], g[1 - axis] = (c, sign), (t, 0)
                todo.append(("%s/%s/%s/%s" % (mover, bname, side, tname), g, si))
        for sx, sy in (("left", "top"), ("right", "top"), ("left", "bottom"), ("right", "bottom")):  # both axes cross together
            todo.append(("%s/%s/%s-%s" % (mover, bname, sx, sy), [sides[sx][1:], sides[sy][1:]], list(sides).index(sx)))
        for name, ((cx, sgx), (cy, sgy)), si in todo:
            for flip in ((0, 180) if mover != "dead" else (0,)):
                h = (headings[mover][si] + flip) % 360 if mover != "dead" else 0
                ux0, uy0 = user(cx, cy)
                x, y = user(cx + sgx * OFFS, cy + sgy * OFFS)
                ux = f32_neighbours(ux0) if sgx else [float(np.float32(ux0))] * 3
                uy = f32_neighbours(uy0) if sgy else [float(np.float32(uy0))] * 3
                lines.append(dict(name="%s/%d" % (name, h), x=np.broadcast_to(x, K.shape), y=np.broadcast_to(y, K.shape),
                                  ux=ux, uy=uy, heading=h, fort_alive=fort_alive, target=target))
    return lines


def off_grid(v):
    """Random user units moved to 0.1 m + 0.03: with the extents 5.31 and 3.51 px no box edge of such a place is a whole pixel"""
    return np.round(np.asarray(v), 1) + 0.03


def shell_velocity(heading):
    """A shell's heading is what its velocity says; half a degree off the whole one, so that its truncation is not in question"""
    a = math.radians(heading + 0.5)
    return SHELL_SPEED * math.cos(a), SHELL_SPEED * math.sin(a), heading + 0.5


def shell_slot(li):
    return (2, 16, 19, 7)[li % 4]


def sweep_batch(O, mover, headings, rng, back_up=False, dead_ships=False):
    """Oracle snapshots of every line of a mover (192 grid envs and 3 ties each) and a few parked envs so that N is no multiple
    of 64, shuffled.  Returns (snaps, line index per env (-1: parked), place along the line (-1: a tie), lines).
    back_up: the projectiles stand one tick of motion in front of their places (for the one-tick test).
    dead_ships: every third line's parked ship is dead, with a death timer that keeps it dead through a tick."""
    from lockstep import fresh

    lines = sweep_lines(mover, headings)
    per = len(K) + 3
    n = len(lines) * per
    n += 37 - n % 64 if n % 64 <= 37 else 101 - n % 64
    assert n % 64 == 37
    s = fresh(O, GAMETYPE, n)
    s["ship_x"], s["ship_y"] = PARK
    line_of, place = np.full(n, -1), np.full(n, -1)
    tab = missile_table()
    for li, L in enumerate(lines):
        i = slice(li * per, (li + 1) * per)
        line_of[i] = li
        place[li * per:li * per + len(K)] = np.arange(len(K))
        x, y = np.concatenate([L["x"], L["ux"]]), np.concatenate([L["y"], L["uy"]])
        s["fort_alive"][i] = L["fort_alive"]
        s["fort_angle"][i] = s["fort_last_angle"][i] = 10 * (li % 36)
        s["points"][i], s["vlner"][i] = HUD[li % 4]
        s["raw_points"][i] = s["points"][i]
        if mover in ("ship", "dead"):
            s["ship_x"][i], s["ship_y"][i], s["ship_angle"][i] = x, y, L["heading"]
            s["ship_alive"][i] = mover == "ship"
        elif mover == "missile":
            slot = (5, 0, 19, 12)[li % 4]
            vx, vy = tab[L["heading"]]
            s["missile_alive"][i, slot] = 1
            s["missile_x"][i, slot], s["missile_y"][i, slot] = x - vx * back_up, y - vy * back_up
            s["missile_vx"][i, slot], s["missile_vy"][i, slot], s["missile_angle"][i, slot] = vx, vy, L["heading"]
        else:
            slot = shell_slot(li)
            vx, vy, a = shell_velocity(L["heading"])
            s["shell_alive"][i, slot] = 1
            s["shell_x"][i, slot], s["shell_y"][i, slot] = x - vx * back_up, y - vy * back_up
            s["shell_vx"][i, slot], s["shell_vy"][i, slot], s["shell_angle"][i, slot] = vx, vy, a
        if dead_ships and li % 3 == 0:
            s["ship_alive"][i], s["ship_death_timer"][i] = 0, 100
    perm = rng.permutation(n)
    return s[perm], line_of[perm], place[perm], lines


# ---------------------------------------------------------------- batches and checks

def snaps_from_state(O, sd):
    """state_dict() as oracle snapshots: what the model and the numpy renderer read"""
    n = len(sd["flags"])
    s = np.zeros(n, O.SNAPSHOT_DTYPE)
    for k in ("time", "ship_x", "ship_y", "points", "vlner", "fort_vuln_timer", "ship_angle", "fort_angle"):
        s[k] = sd[k]
    s["ship_alive"], s["fort_alive"] = sd["flags"] & 1, (sd["flags"] >> 1) & 1
    for kind in ("missile", "shell"):
        s[kind + "_alive"] = mask_bits(sd[kind + "_mask"]).T
        s[kind + "_x"], s[kind + "_y"] = sd[kind + "_x"].T, sd[kind + "_y"].T
    s["missile_angle"] = sd["missile_angle"].T
    a = np.degrees(np.arctan2(sd["shell_vy"].T, sd["shell_vx"].T))
    s["shell_angle"] = np.where(a < 0, a + 360.0, a)
    return s


def image_batch(sfa, n, snaps=None):
    env = sfa.SFVecEnv(n, gametype=GAMETYPE, obs_type="image", spawn_stride=3)
    if snaps is not None:
        load_state(env, snaps)
    return env


def in_place_batch(sfa, monkeypatch, n, snaps=None):
    """A batch that draws every frame in place, in env order"""
    monkeypatch.setenv("SFMI_NO_EXPLOSION_CACHE", "1")
    monkeypatch.setenv("SFMI_NO_RENDER_ORDER", "1")
    env = image_batch(sfa, n, snaps)
    env.render("image")  # the switches are read at create / by the first frame
    monkeypatch.delenv("SFMI_NO_EXPLOSION_CACHE")
    monkeypatch.delenv("SFMI_NO_RENDER_ORDER")
    return env


def check_records(rec, snaps, allowed_ties, what):
    """(a): header words and live bytes against the model on every env that is no tie; ties only where allowed.  A tie's bits
    are not the model's to state: they are held to the library's own float32 evaluation, operation by operation (its build
    has contraction off) -- the one place where a `<` turned `<=` shows.  Returns the device's header words."""
    want, margin = D.record(snaps, pics=True)
    tie = margin < D.TIE
    stray = np.flatnonzero(tie & ~allowed_ties)
    assert stray.size == 0, (what, "ties on the grid", stray[:8].tolist(), margin[stray[:8]].tolist())
    if tie.any():
        want[tie] = D.record(snaps[tie], pics=True, f32=True)[0]
    live = D.live_bytes(want[:, :32].copy().view("<u4"))
    bad = np.argwhere(live & (rec != want))
    if bad.size:
        i = int(bad[0][0])
        raise AssertionError((what, len(np.unique(bad[:, 0])), "envs differ; env", i, "bytes", bad[bad[:, 0] == i][:, 1][:12].tolist(),
                              "words", [hex(int(w)) for w in rec[i, :32].view("<u4")], "model", [hex(int(w)) for w in want[i, :32].view("<u4")],
                              "margin", float(margin[i])))
    return rec[:, :32].copy().view("<u4")


def check_same_frames(a, b, what):
    """(b): both sizes, byte for byte"""
    for mode in ("image", "image-raw"):
        x, y = a.render(mode), b.render(mode)
        if not torch.equal(x, y):
            raise AssertionError((what, mode, (x != y).flatten(1).any(1).nonzero().flatten()[:8].tolist()))


def check_model_frames(model, env, snaps, idx, what, small=None):
    """(c): the frames of the envs `idx` against the numpy renderer, both sizes (`small`: the 84x84 frames to compare
    instead of a fresh render, e.g. a step's observation)"""
    R, hb, hs, bg = model
    idx = np.asarray(sorted(set(int(i) for i in idx)))
    t = torch.from_numpy(idx).to(env.device)
    raw = env.render("image-raw")[t].cpu().numpy()
    small = (env.render("image") if small is None else small)[t].cpu().numpy()
    for j, i in enumerate(idx):
        want = R.render_raw(snaps[i], hb, hs, bg=bg)
        frames_equal(raw[j], want, (what, "raw", int(i)))
        frames_equal(small[j, 0], R.resize_area(want), (what, "84x84", int(i)))
    return len(idx)


def line_table(line_of, place, n_lines):
    order = np.full((n_lines, len(K)), -1)
    on = place >= 0
    order[line_of[on], place[on]] = np.flatnonzero(on)
    assert (order >= 0).all()
    return order


def check_flips(words, order, lines):
    """along each sweep both values of the targeted flag occur"""
    for li, L in enumerate(lines):
        w, m = L["target"]
        v = (words[order[li], w] & np.uint32(m)) != 0
        # (the first place lies 1.5 px outside, the last 1.5 px inside)
        assert v[-1] and not v[0], (L["name"], "the sweep never flips", bool(v[0]), bool(v[-1]))


def select_frames(words, order, line_of, place):
    """The rule of (c): per line its two ends, both sides of every change of words 3..5, its ties; if that is more than
    MAX_MODEL_FRAMES frames, every j-th LINE whole (j odd: the two headings of a line alternate).  Returns (envs, j)."""
    w = words[order][:, :, 3:6]
    change = (w[:, 1:] != w[:, :-1]).any(2)
    sel = np.zeros(order.shape, bool)
    sel[:, 0] = sel[:, -1] = True
    sel[:, :-1] |= change
    sel[:, 1:] |= change
    per_line = sel.sum(1) + 3
    j = max(1, -(-int(per_line.sum()) // MAX_MODEL_FRAMES))
    j += 1 - j % 2
    keep = np.arange(len(order))[::j]
    envs = [order[li][sel[li]] for li in keep] + [np.flatnonzero((place < 0) & np.isin(line_of, keep))]
    return np.concatenate(envs), j


@pytest.mark.parametrize("mover", ["ship", "dead", "missile", "shell"])
def test_directed_sweeps(sfa, oracle_mod, model, headings, monkeypatch, mover):
    """One mover against every side of every box its decisions compare it with, from a state loaded with set_field: the
    records sf_drawrec_kernel makes, the frames with and without every shortcut, the numpy renderer."""
    snaps, line_of, place, lines = sweep_batch(oracle_mod, mover, headings, np.random.default_rng(71))
    n = len(snaps)
    env = image_batch(sfa, n, snaps)
    words = check_records(env.draw_records(True), snaps, (place < 0) & (line_of >= 0), mover)
    order = line_table(line_of, place, len(lines))
    check_flips(words, order, lines)
    plain = in_place_batch(sfa, monkeypatch, n, snaps)
    check_same_frames(env, plain, mover)
    plain.close()
    sel, j = select_frames(words, order, line_of, place)
    shown = check_model_frames(model, env, snaps, sel, mover)
    print("sweeps of %s: %d envs, %d lines, every %d. line, %d frames against the model" % (mover, n, len(lines), j, shown))
    env.close()


def combination_snaps(O, n, rng, back_up=False):
    """Envs with a missile in slot 3 on the text box, a missile in slot 17 on the bar and a shell within reach of the text box
    only -- each of the three present or not by the env's number, so that in every tile several owners' words are ORed at
    once and every subset occurs; the rest of the 20 slots hold projectiles far from both boxes."""
    from lockstep import fresh

    tab = missile_table()
    s = fresh(O, GAMETYPE, n)
    s["ship_x"], s["ship_y"] = PARK
    i = np.arange(n)
    ang = rng.integers(0, 360, (n, 20))
    s["missile_alive"] = rng.random((n, 20)) < 0.15
    s["missile_angle"], s["missile_vx"], s["missile_vy"] = ang, tab[ang, 0], tab[ang, 1]
    s["missile_x"], s["missile_y"] = off_grid(rng.uniform(150, 560, (n, 20))), off_grid(rng.uniform(220, 420, (n, 20)))
    s["shell_alive"] = rng.random((n, 20)) < 0.1
    sa = rng.integers(0, 360, (n, 20)) + 0.5
    s["shell_angle"], s["shell_vx"], s["shell_vy"] = sa, SHELL_SPEED * np.cos(np.radians(sa)), SHELL_SPEED * np.sin(np.radians(sa))
    s["shell_x"], s["shell_y"] = off_grid(rng.uniform(150, 560, (n, 20))), off_grid(rng.uniform(220, 420, (n, 20)))
    # slot 3: on the text box, (45 +- 9, 3.5) px; slot 17: on the bar, (45 +- 15, 89); shell slot 5: its top edge in row 6 or 7
    for slot, on, x, y in ((3, (i & 1) != 0, 355 + rng.integers(-45, 46, n) + 0.3, np.full(n, 97.7)),
                           (17, (i & 2) != 0, 355 + rng.integers(-75, 76, n) + 0.3, np.full(n, 525.3))):
        s["missile_alive"][:, slot] = on
        s["missile_x"][:, slot], s["missile_y"][:, slot] = x - s["missile_vx"][:, slot] * back_up, y - s["missile_vy"][:, slot] * back_up
    s["shell_alive"][:, 5] = (i & 4) != 0
    s["shell_x"][:, 5] = 355 + rng.integers(-45, 46, n) + 0.3 - s["shell_vx"][:, 5] * back_up
    s["shell_y"][:, 5] = 80 + 5 * (7.0 + D.SHELL_EXT) + rng.uniform(-4, 4, n).round(1) + 0.03 - s["shell_vy"][:, 5] * back_up
    s["points"] = s["raw_points"] = np.where(i & 8, 37, 0)
    s["vlner"] = np.where(i & 16, 4, 0)
    return s


def test_combinations(sfa, oracle_mod, model, monkeypatch):
    """Missiles of two slots and a shell of one env on different boxes, in many lanes of a tile at once"""
    n = 333
    snaps = combination_snaps(oracle_mod, n, np.random.default_rng(72))
    env = image_batch(sfa, n, snaps)
    words = check_records(env.draw_records(True), snaps, np.zeros(n, bool), "combinations")
    fl = words[:, D.W_FLAGS]
    for bit in (D.F_NEAR_TEXT, D.F_NEAR_BAR, D.F_OTHER_TEXT, D.F_OTHER_BAR, D.F_BAKED_TEXT, D.F_BAKED_BAR):
        assert (fl & bit).any() and not (fl & bit).all(), hex(bit)
    assert ((fl & (D.F_NEAR_TEXT | D.F_OTHER_TEXT)) == D.F_OTHER_TEXT).any()  # within reach only
    plain = in_place_batch(sfa, monkeypatch, n, snaps)
    check_same_frames(env, plain, "combinations")
    plain.close()
    check_model_frames(model, env, snaps, range(0, 64), "combinations")
    env.close()


# ---------------------------------------------------------------- integer logic

def far_projectiles(s, rng, mm, sm):
    """missile / shell masks [n] as projectiles far from the score and the bar (rows 24..74), the shells away from the fortress"""
    n = len(s)
    tab = missile_table()
    bits = lambda m: ((np.asarray(m, np.int64)[:, None] >> np.arange(20)) & 1).astype(np.int32)
    ang = rng.integers(0, 360, (n, 20))
    s["missile_alive"], s["shell_alive"] = bits(mm), bits(sm)
    s["missile_angle"], s["missile_vx"], s["missile_vy"] = ang, tab[ang, 0], tab[ang, 1]
    s["missile_x"], s["missile_y"] = off_grid(rng.uniform(150, 560, (n, 20))), off_grid(rng.uniform(200, 450, (n, 20)))
    sa = rng.integers(0, 360, (n, 20)) + 0.5
    s["shell_angle"], s["shell_vx"], s["shell_vy"] = sa, SHELL_SPEED * np.cos(np.radians(sa)), SHELL_SPEED * np.sin(np.radians(sa))
    s["shell_x"] = off_grid(np.where(rng.random((n, 20)) < 0.5, rng.uniform(150, 310, (n, 20)), rng.uniform(400, 560, (n, 20))))
    s["shell_y"] = off_grid(rng.uniform(200, 450, (n, 20)))


def integer_case(O, name, rng):
    """(snaps, envs to hold against the numpy renderer)"""
    from lockstep import fresh

    if name == "merge":
        hi, mi = np.meshgrid(np.arange(20), np.arange(-1, 20), indexing="ij")
        sm = np.concatenate([(1 << hi.ravel()) | (rng.integers(0, 1 << 20, hi.size) & ((1 << hi.ravel()) - 1)),
                             rng.integers(0, 1 << 20, 2000) >> rng.integers(0, 20, 2000)])
        mm = np.concatenate([np.where(mi.ravel() < 0, 0, 1 << np.maximum(mi.ravel(), 0)), rng.integers(0, 1 << 20, 2000) >> rng.integers(0, 20, 2000)])
        s = fresh(O, GAMETYPE, len(sm))
        far_projectiles(s, rng, mm, sm)
        return s, np.concatenate([np.arange(0, 420, 7), 420 + np.arange(0, 2000, 50)])
    if name == "bar":
        v, t = np.meshgrid(np.arange(16), [0, 249, 250, 251, 4000], indexing="ij")
        s = fresh(O, GAMETYPE, v.size)
        s["vlner"], s["fort_vuln_timer"] = v.ravel(), t.ravel()
        return s, np.arange(v.size)
    if name == "points":
        p = np.array([-513, -512, -511, -1, 0, 1, 511, 512, 513, -0.95, 0.95, 1.000001, -1.000001, 37, 9999999], np.float32)
        s = fresh(O, GAMETYPE, len(p))
        s["points"] = s["raw_points"] = p
        return s, np.arange(len(p))
    assert name == "fort_angle"
    a, alive, on = np.meshgrid(np.arange(360), [1, 0], [0, 1], indexing="ij")
    s = fresh(O, GAMETYPE, a.size)
    s["fort_angle"] = s["fort_last_angle"] = a.ravel()
    s["fort_alive"] = alive.ravel()
    s["ship_x"] = np.where(on.ravel(), 415.0, PARK[0])  # (415, 300) -> 51.6..62.4 x 38.6..49.4 px: on the picture and on the explosion
    s["ship_y"] = PARK[1]
    # against the numpy renderer: all 360 live headings under the ship (a heading between two pictures is drawn in place
    # whatever the ship does), every seventh and every picture's with the ship clear, every eleventh of the dead fortress
    a, alive, on = a.ravel(), alive.ravel(), on.ravel()
    return s, np.flatnonzero((alive == 1) & ((on == 1) | (a % 7 == 0) | (a % 10 == 0)) | (alive == 0) & (a % 11 == 0))


@pytest.mark.parametrize("name", ["merge", "bar", "points", "fort_angle"])
def test_integer_logic(sfa, oracle_mod, model, monkeypatch, name):
    """merge (every highest shell slot against no missile and each single missile, and random mask pairs), the bar's state,
    the truncation of the points, every fortress heading alive and dead with the ship clear of its picture and on it"""
    rng = np.random.default_rng(73)
    snaps, shown = integer_case(oracle_mod, name, rng)
    n = len(snaps)
    env = image_batch(sfa, n, snaps)
    words = check_records(env.draw_records(True), snaps, np.zeros(n, bool), name)
    plain = in_place_batch(sfa, monkeypatch, n, snaps)
    check_same_frames(env, plain, name)
    plain.close()
    check_model_frames(model, env, snaps, shown, name)
    if name == "merge":
        merged = (words[:, D.W_FLAGS] & D.F_MERGE_SHELLS) != 0
        assert merged[:420].sum() > 50 and (~merged[:420]).sum() > 50 and merged[420:].any()
        # the shared decision: with every live shell slot below 8, the same scene with every shell 12 slots higher (same order,
        # 1 + the highest slot > 8: nothing merges) is the same frame
        low = np.flatnonzero((snaps["shell_alive"][:, 8:] == 0).all(1) & (snaps["shell_alive"] != 0).any(1))
        assert len(low) > 100 and merged[low].any()
        up = snaps.copy()
        for k in ("shell_alive", "shell_x", "shell_y", "shell_vx", "shell_vy", "shell_angle"):
            up[k][low] = np.roll(snaps[k][low], 12, axis=1)
        raised = image_batch(sfa, n, up)
        assert not (raised.draw_records(True)[low, 20:24].copy().view("<u4")[:, 0] & D.F_MERGE_SHELLS).any()
        t = torch.from_numpy(low).to(env.device)
        for mode in ("image", "image-raw"):
            assert torch.equal(env.render(mode)[t], raised.render(mode)[t]), mode
        raised.close()
    env.close()


def test_the_twentieth_missile_draws_like_the_first(sfa, oracle_mod, model, monkeypatch):
    """SF_DRF_MISSILE19: with a single missile alive, the frame is the same whether it sits in slot 19 or in slot 0 -- and both
    batches pass the three checks (the places are off the whole pixels: no ties)"""
    from lockstep import fresh

    n = 200
    rng = np.random.default_rng(74)
    tab = missile_table()
    a, b = fresh(oracle_mod, GAMETYPE, n), fresh(oracle_mod, GAMETYPE, n)
    ang = rng.integers(0, 360, n)
    x, y = off_grid(rng.uniform(120, 590, n)), off_grid(np.where(np.arange(n) % 3 == 0, rng.uniform(70, 130, n), rng.uniform(70, 550, n)))
    for s, slot in ((a, 0), (b, 19)):
        s["missile_alive"][:, slot] = 1
        s["missile_x"][:, slot], s["missile_y"][:, slot], s["missile_angle"][:, slot] = x, y, ang
        s["missile_vx"][:, slot], s["missile_vy"][:, slot] = tab[ang, 0], tab[ang, 1]
    ea, eb = image_batch(sfa, n, a), image_batch(sfa, n, b)
    wa, wb = (check_records(e.draw_records(True), s, np.zeros(n, bool), what) for e, s, what in ((ea, a, "slot 0"), (eb, b, "slot 19")))
    plain = in_place_batch(sfa, monkeypatch, n, b)
    check_same_frames(eb, plain, "slot 19 in place")
    plain.close()
    assert not (wa[:, D.W_FLAGS] & D.F_MISSILE19).any() and (wb[:, D.W_FLAGS] & D.F_MISSILE19).all()
    assert np.array_equal(wa[:, D.W_FLAGS], wb[:, D.W_FLAGS] & ~np.uint32(D.F_MISSILE19))
    check_same_frames(ea, eb, "slot 19 against slot 0")
    check_model_frames(model, eb, b, range(0, n, 5), "slot 19")
    ea.close()
    eb.close()


# ---------------------------------------------------------------- one tick

@pytest.mark.parametrize("mover", ["missile", "shell", "combinations"])
def test_one_tick_leaves_the_models_records(sfa, oracle_mod, model, headings, monkeypatch, mover):
    """The step kernel gathers the projectile flags with the state in registers, along its own routes: shells that moved
    (the dense pass and, from slot 16 on, the walk), missiles through an atomic OR into the owner's event word.  The sweeps
    one tick of motion in front of their places, one no-op tick: the records the step left equal the model's of the state
    after the tick and the records rebuilt from that state, the observation equals the in-place batch's and the numpy
    renderer's -- and the tick itself is the oracle's.  Every third line's ship is dead, mid-explosion."""
    O = oracle_mod
    rng = np.random.default_rng(75)
    if mover == "combinations":
        n = 333
        snaps, lines = combination_snaps(O, n, rng, back_up=True), None
        snaps["ship_alive"][::3], snaps["ship_death_timer"][::3] = 0, 100
    else:
        snaps, line_of, place, lines = sweep_batch(O, mover, headings, rng, back_up=True, dead_ships=True)
        n = len(snaps)
    env = image_batch(sfa, n, snaps)
    plain = in_place_batch(sfa, monkeypatch, n, snaps)
    orc = O.OracleVecEnv(GAMETYPE, n)  # (lockstep.load_both's two halves: its batch is a features batch)
    orc.load_snapshots(snaps, None)
    noop = torch.zeros(n, dtype=torch.uint8, device=env.device)
    obs = env.step_tensors(noop)[0].clone()
    assert torch.equal(obs, plain.step_tensors(noop)[0]), "the in-place batch's observation"
    plain.close()
    orc.step(np.zeros(n, np.int32))
    sd = env.state_dict()
    bad = compare_state(sd, orc.snapshots())
    assert not bad, bad
    after = snaps_from_state(O, sd)
    dead = snaps["ship_alive"] == 0
    assert dead.any() and not after["ship_alive"][dead].any()
    stepped = env.draw_records(False)
    # (the bystanders of the combination envs end the tick anywhere: a tie among them is not compared, and there are few)
    allowed = np.ones(n, bool) if lines is None else (place < 0) & (line_of >= 0)
    words = check_records(stepped, after, allowed, mover)
    assert (D.header(after)[1] < D.TIE).sum() <= (n // 10 if lines is None else 3 * len(lines))
    rebuilt = env.draw_records(True)
    live = D.live_bytes(words)
    assert np.array_equal(np.where(live, stepped, 0), np.where(live, rebuilt, 0)), np.argwhere(live & (stepped != rebuilt))[:8].tolist()
    if lines is None:
        sel = np.arange(0, 64)
    else:
        assert mover != "shell" or (after["shell_alive"][:, 16:] != 0).any()
        order = line_table(line_of, place, len(lines))
        check_flips(words, order, lines)
        sel, j = select_frames(words, order, line_of, place)
    shown = check_model_frames(model, env, after, sel, mover, small=obs)
    print("one tick of %s: %d envs, %d frames against the model" % (mover, n, shown))
    env.close()


# ---------------------------------------------------------------- the explosion cache when its keys change

def test_explosion_cache_when_points_and_bar_change(sfa, oracle_mod, model, monkeypatch):
    """A ship that died right under the score or right over the bar: its explosion's cache entry holds the score's / the bar's
    box as drawn over it, keyed by the points and the bar's state.  At frames 0, 5 and 11 of the explosion set_field changes
    them (in play: the ship's own missiles land while it explodes) -- points inside and outside the picture table, vlner
    across a change of the bar's state and into kill-ready.  Product against in place at every tick, both sizes; against the
    numpy renderer at the tick of each change and the one after."""
    from lockstep import fresh

    O = oracle_mod
    n, T = 64, 14
    rng = np.random.default_rng(76)
    i = np.arange(n)
    s = fresh(O, GAMETYPE, n)
    s["ship_alive"], s["ship_death_timer"] = 0, 0
    s["ship_x"] = 355 + rng.integers(-60, 61, n)
    s["ship_y"] = np.where(i % 2 == 0, 150 + rng.integers(0, 12, n), 470 + rng.integers(0, 12, n))
    points = np.array([0, 37, 511, 512, 600, -5, 100000, 0], np.float32)
    vlner = np.array([0, 4, 9, 10, 11, 12, 0, 3], np.int32)
    env, plain = image_batch(sfa, n, s), in_place_batch(sfa, monkeypatch, n, s)
    noop = torch.zeros(n, dtype=torch.uint8, device=env.device)
    shown = np.arange(0, n, 3)  # against the numpy renderer: under the score and over the bar, both timers
    assert {(int(k) % 2, int(k) % 4 < 2) for k in shown} == {(0, True), (0, False), (1, True), (1, False)}
    change = 0
    for t in range(T):
        if t in (0, 5, 11):
            for e in (env, plain):
                p = points[(i // 2 + change) % len(points)]
                e.set_field("points", p)
                e.set_field("raw_points", p)
                e.set_field("vlner", vlner[(i // 3 + change) % len(vlner)])
                e.set_field("fort_vuln_timer", np.where(i % 4 < 2, 0, 300).astype(np.int32))
            change += 1
            check_same_frames(env, plain, ("set", t))
        o1, o2 = env.step_tensors(noop)[0], plain.step_tensors(noop)[0]
        assert torch.equal(o1, o2), t
        check_same_frames(env, plain, t)
        if t in (0, 1, 5, 6, 11, 12):
            after = snaps_from_state(O, env.state_dict())
            assert not after["ship_alive"].any(), t
            check_model_frames(model, env, after, shown, ("explosion", t), small=o1)
    env.close()
    plain.close()
