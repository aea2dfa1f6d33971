"""The three observation columns that come out of the project's own numerical code -- aim, vdir and ndist (columns 6, 7, 8 of
`features` and `normalized-features`, thresholds of them in `monitors`) -- as a plain 70-digit restatement of
Game::computeExtra (oracle/sf_oracle.c:340-368) and of the observation writers' use of it (:700-742); the bounds the device's
values are held to; and the states they are held on.  No GPU, no torch: `decimal` and numpy.

THE REFERENCE.  The inputs are the doubles and integers of `state_dict()`.  The differences ship - fortress are taken in
binary64, as every restatement takes them (one IEEE subtraction, the same bits everywhere); from there on everything is exact:
atan2 to 70 digits (the libm value plus a correction, `atan2_hp`), pi to 70 digits, the wraps on the exact value.  A new game's
row is this definition too, computeExtra(spawn), not the reference program's stale heap.

THE BOUNDS, in degrees, each a sum of named terms (`AIM_TERMS`, `VDIR_TERMS`); u(m) is half an ulp of a double of magnitude
below m, 2^-53 * m for a power of two m.

  angle        1e-15 rad: sf_atan2_core's contract (sf_lane_dev.h).  The exact forms (near-axis, exact-degree) are correctly
               rounded, u(4) = 2.2e-16, and the device libm of a new game's row is faithful, under an ulp, 4.4e-16: both inside
               the core's term.  In degrees: 1e-15 * 180 / pi = 5.73e-14.
  rad2deg      a / M_PI is the correctly rounded quotient (sf_div_const), |q| <= 1: u(1) * 180 = 1.00e-14; the divisor is
               M_PI, not pi, relative 3.9e-17: 180 * 3.9e-17 = 0.70e-14; the product q * 180 is below 256: u(256) = 1.42e-14.
  aim          `- angle`: |deg - angle| <= 180 + 359 < 1024: u(1024) = 5.68e-14.  `+ 180`: the sum lies in [-359, 360]:
               u(512) = 2.84e-14.  `+ 360` on the wrap: the result is below 256: u(256) = 1.42e-14.
               AIM_BOUND = 5.73 + 1.00 + 0.70 + 1.42 + 5.68 + 2.84 + 1.42 = 1.88e-13 degrees.
  vdir         two angles, 2 * 1e-15 rad.  The first angle is derived, +-M_PI - a_pos: one rounding below 4, u(4) = 2.22e-16,
               and M_PI for pi, 1.22e-16 (on the fortress row it is a libm call that returns 0 or +-M_PI: inside that).  The
               difference is below 8: u(8) = 4.44e-16.  The wrap -+2 M_PI: 2 M_PI for 2 pi, 2.45e-16, one rounding below 4,
               2.22e-16.  Sum 3.26e-15 rad = 1.87e-13 degrees; then rad2deg as above, 3.12e-14.
               VDIR_BOUND = 2.18e-13 degrees.
  normalised   aim / 180 clamped: AIM_BOUND / 180 + u(2).  (vdir % 360) / 360: the fmod is exact, `+ 360` rounds below 512,
               the quotient below 1: (VDIR_BOUND + u(512)) / 360 + u(1).

aim lies in [-180, 360] and vdir in [-180, 180] (closed: the wraps compare a rounded value), the normalised vdir in [0, 1], and
all of them are compared ON THE CIRCLE (mod 360; the normalised forms mod 2 and mod 1): next to a wrap the exact value and a value
one rounding off land on opposite ends of the range, and both name the same angle.  vdir of a ship at rest is 0.0 exactly.

ndist has no bound: -1 + (|sx - 355| - 40) / 80 in IEEE operations that sf_div_const reproduces bit for bit, and
sqrt(dx * dx) == |dx| in binary64.  The float64 column is numpy's evaluation of that expression, the float32 column its float32,
the normalised column its clamp.

float32: a float32 observation is (float) of the double, so it is float32(x) for some x within the bound of the reference: it
lies between float32(ref - B) and float32(ref + B), at most two neighbouring floats (`check_column`).

monitors: where the reference is further than the bound from a threshold (aim against 3, and against the wrap at -180, where
the two ends of the range fall on different sides of 3), the column must show the reference's side; inside the band either
passes.  ndist's thresholds have no band.  The share of values inside a band must stay under 1 % (`BAND_SHARE_MAX`).

THE STATES (`states()`): about 3 000 of them in named families, each a state in front of ONE tick without keys; `after_tick`
is where the ship stands afterwards.  What each family claims of itself is asserted by tests/test_bearing_columns_model.py."""
import math
from decimal import Context, Decimal, localcontext

import numpy as np

CTX = Context(prec=70)
FORT_X, FORT_Y = 355.0, 315.0
NDIST_A, NDIST_B = 40.0, 80.0


def u(m):
    """half an ulp of a double whose magnitude is below the power of two m"""
    assert m > 0 and math.frexp(m)[0] == 0.5
    return m * 2.0 ** -54  # (an ulp in [m / 2, m) is m * 2^-53)


RAD = 180.0 / math.pi  # (only ever scales a bound)
M_PI_ERR = 1.2246467991473532e-16  # pi - M_PI
ANGLE_CORE = 1e-15            # rad: sf_atan2_core's contract
RAD2DEG_TERMS = {"quotient a / M_PI": u(1) * 180, "M_PI for pi in the divisor": 180 * M_PI_ERR / math.pi, "product q * 180": u(256)}
AIM_TERMS = dict({"angle (core)": ANGLE_CORE * RAD, "- angle": u(1024), "+ 180": u(512), "+ 360 on the wrap": u(256)}, **RAD2DEG_TERMS)
VDIR_TERMS = dict({"bearing (core)": ANGLE_CORE * RAD, "velocity angle (core)": ANGLE_CORE * RAD,
                   "+-M_PI - a_pos, rounding": u(4) * RAD, "M_PI for pi": M_PI_ERR * RAD, "a_vel - ov": u(8) * RAD,
                   "2 M_PI for 2 pi on the wrap": 2 * M_PI_ERR * RAD, "wrap, rounding": u(4) * RAD}, **RAD2DEG_TERMS)
AIM_BOUND = sum(AIM_TERMS.values())
VDIR_BOUND = sum(VDIR_TERMS.values())
NAIM_BOUND = AIM_BOUND / 180 + u(2)
NVDIR_BOUND = (VDIR_BOUND + u(512)) / 360 + u(1)
BAND_SHARE_MAX = 0.01
# (column, bound, period, closed range) of the two bounded columns per observation type
RULES = {"features": {6: (AIM_BOUND, 360, (-180, 360)), 7: (VDIR_BOUND, 360, (-180, 180))},
         "normalized-features": {6: (NAIM_BOUND, 2, (-1, 1)), 7: (NVDIR_BOUND, 1, (0, 1))}}


# ---------------------------------------------------------------- 70-digit arithmetic

def _sincos(T):
    s, c, term, k = Decimal(0), Decimal(0), Decimal(1), 0
    while abs(term) > Decimal(10) ** -68:
        if k % 2 == 0:
            c += term if k % 4 == 0 else -term
        else:
            s += term if k % 4 == 1 else -term
        k += 1
        term = term * T / k
    return s, c


def atan2_hp(y, x):
    """atan2(y, x) of two doubles to 70 digits: the libm value t0 plus atan((y cos t0 - x sin t0) / (x cos t0 + y sin t0)), sin
    and cos of t0 by their series.  The signs of zeros count as in C (atan2(-0.0, -1) is -pi)."""
    with localcontext(CTX):
        t0 = math.atan2(y, x)
        T = Decimal(t0)
        s, c = _sincos(T)
        Y, X = Decimal(y), Decimal(x)
        t = (Y * c - X * s) / (X * c + Y * s)
        return T + t - t ** 3 / 3  # (|t| < 1e-15: the next term is below 1e-75)


def atan2_correctly_rounded(y, x):
    """atan2(y, x) of two doubles, correctly rounded, by 70-digit arithmetic"""
    with localcontext(CTX):
        theta = atan2_hp(y, x)
        t0 = math.atan2(y, x)
        cands = [t0, math.nextafter(t0, math.inf), math.nextafter(t0, -math.inf)]
        return min(cands, key=lambda v: abs(Decimal(v) - theta))


PI = atan2_hp(0.0, -1.0)
with localcontext(CTX):
    DEG = Decimal(180) / PI

_cache = {}


def _atan2_cached(y, x):
    k = (float(y).hex(), float(x).hex())
    v = _cache.get(k)
    if v is None:
        v = _cache[k] = atan2_hp(float(y), float(x))
    return v


# ---------------------------------------------------------------- the reference

def bearings(sx, sy):
    """the exact bearing of the ship from the fortress, atan2(sy - 315, sx - 355) on the binary64 differences, in degrees"""
    with localcontext(CTX):
        return [_atan2_cached(np.float64(y) - FORT_Y, np.float64(x) - FORT_X) * DEG for x, y in zip(sx, sy)]


def reference(sx, sy, vx, vy, angle):
    """Game::computeExtra at 70 digits.  Arrays as state_dict() returns them; per lane `aim` and `vdir` (Decimal, degrees, in
    their ranges), `ndist` (float64, exact), and the normalised forms `naim`, `nvdir` (Decimal), `nndist` (float64)."""
    sx, sy, vx, vy = (np.asarray(a, np.float64) for a in (sx, sy, vx, vy))
    angle = np.asarray(angle)
    aim, vdir, naim, nvdir = [], [], [], []
    with localcontext(CTX):
        for i in range(len(sx)):
            dx, dy = sx[i] - FORT_X, sy[i] - FORT_Y  # binary64, as every restatement takes them
            o = _atan2_cached(dy, dx) * DEG - int(angle[i]) + 180
            if o < -180:
                o += 360
            aim.append(o)
            if float(vx[i]) * float(vx[i]) + float(vy[i]) * float(vy[i]) == 0.0:  # norm() == 0, in binary64 as the game takes it
                d = Decimal(0)
            else:
                d = _atan2_cached(vy[i], vx[i]) - _atan2_cached(-(FORT_Y - sy[i]), FORT_X - sx[i])
                if d > PI:
                    d -= 2 * PI
                if d < -PI:
                    d += 2 * PI
                d *= DEG
            vdir.append(d)
            naim.append(max(Decimal(-1), min(Decimal(1), o / 180)))
            nvdir.append((d % 360 + 360) % 360 / 360)  # Python's float %: the divisor's sign
    ndist = -1 + (np.abs(sx - FORT_X) - NDIST_A) / NDIST_B
    return {"aim": aim, "vdir": vdir, "ndist": ndist, "naim": naim, "nvdir": nvdir, "nndist": np.clip(ndist, -1.0, 1.0)}


def _f32(d):
    """a Decimal rounded to the nearest float32 (one rounding)"""
    f = np.float32(float(d))
    c = [f, np.nextafter(f, np.float32(np.inf)), np.nextafter(f, np.float32(-np.inf))]
    return min(c, key=lambda v: abs(Decimal(float(v)) - d))


def check_column(dev, ref, bound, period, rng, f32=False):
    """One bounded column against the reference, on the circle.  dev: float64 or float32 array; ref: Decimals.  Returns (err,
    ok): err[i] the circular distance in units of the bound (float32: the distance to the allowed interval of floats, 0 inside
    it), ok[i] whether the rule of the module's docstring holds, the closed range included."""
    n = len(ref)
    err, ok = np.zeros(n), np.zeros(n, bool)
    lo, hi = Decimal(rng[0]), Decimal(rng[1])
    with localcontext(CTX):
        B, P = Decimal(bound), Decimal(period)
        for i in range(n):
            v = float(dev[i])
            if not (rng[0] <= v <= rng[1]):  # (a NaN fails here)
                err[i] = np.inf
                continue
            d = Decimal(v)
            if not f32:
                e = abs(d - ref[i]) % P
                e = min(e, P - e)
                err[i] = float(e / B)
                ok[i] = e <= B
                continue
            best = None
            for s in (0, 1, -1):  # the same angle one period off, where it still lies in the range
                c = ref[i] + s * P
                a, b = max(c - B, lo), min(c + B, hi)
                if a > b:
                    continue
                fa, fb = Decimal(float(_f32(a))), Decimal(float(_f32(b)))
                e = Decimal(0) if fa <= d <= fb else min(abs(d - fa), abs(d - fb))
                best = e if best is None or e < best else best
            err[i] = float(best / B)
            ok[i] = best == 0
    return err, ok


def close_on_circle_f32(dev, ref, bound, period):
    """check_column's float32 rule in vector form, for a float64 reference that is itself within the bound's half of the truth
    (the CPU oracle's column): float32(x) is within half a float32 ulp of x, so |dev - ref| on the circle is at most the bound
    plus that half ulp.  No Decimal: cheap enough for the large batches of the played tests."""
    d64, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    d = np.abs(d64 - ref)
    d = np.minimum(d, np.abs(period - d))
    half_ulp = np.spacing(np.maximum(np.abs(np.asarray(dev, np.float32)), np.abs(ref).astype(np.float32))).astype(np.float64) / 2
    return d <= bound + half_ulp + np.spacing(np.float64(period))  # (the last term: `period - d` rounds)


def aim_band(aim):
    """lanes whose aim is within the bound of a threshold of `monitors`: 3 itself, and the wrap at -180 (the range's two ends
    fall on different sides of 3)"""
    with localcontext(CTX):
        B = Decimal(AIM_BOUND)
        return np.array([abs(a - 3) <= B or abs(a + 180) <= B or abs(a - 180) <= B for a in aim])


def monitors_columns(ref):
    """columns 4..9 of `monitors` from the reference, and the mask [n, 6] of entries where either side passes"""
    n = len(ref["aim"])
    want = np.empty((n, 6))
    want[:, 0] = [0.5 if a < 3 else -0.5 for a in ref["aim"]]
    want[:, 1] = [0.5 if a > 3 else -0.5 for a in ref["aim"]]
    nd = ref["ndist"]
    want[:, 2], want[:, 3] = np.where(nd > .75, .5, -.5), np.where(nd > .25, .5, -.5)
    want[:, 4], want[:, 5] = np.where(nd < -.25, .5, -.5), np.where(nd < -.75, .5, -.5)
    free = np.zeros((n, 6), bool)
    free[:, 0] = free[:, 1] = aim_band(ref["aim"])
    return want, free


def other_columns(sd, obs_type, youturn, lanes=None):
    """every column outside aim / vdir / ndist as `state_dict()` implies it, float64 [n, dim] (the three columns hold NaN); for
    monitors columns 0..3.  kill_ready as the kernels define it: vlner > 10 and the vulnerability timer under 250."""
    g = (lambda k: np.asarray(sd[k])) if lanes is None else (lambda k: np.asarray(sd[k])[..., lanes])
    fl = g("flags")
    n_missiles = np.array([bin(int(m)).count("1") for m in g("missile_mask")], np.float64)
    vl = g("vlner").astype(np.float64)
    kill_ready = ((g("vlner") > 10) & (g("fort_vuln_timer") < 250)).astype(np.float64)
    ship, fort = ((fl & 1) != 0).astype(np.float64), ((fl & 2) != 0).astype(np.float64)
    timers = [g(k).astype(np.float64) for k in ("fire_timer", "thrust_timer", "left_timer", "right_timer")][: 4 if youturn else 2]
    nan = np.full(len(fl), np.nan)
    if obs_type == "monitors":
        return np.stack([np.where(n_missiles > 0, .5, -.5), np.where(fort > 0, .5, -.5), np.where(vl > 10, .5, -.5),
                         np.where(kill_ready > 0, .5, -.5)], 1)
    if obs_type == "features":  # (the shells column shows the missiles: SRC/pymodule.cpp:131-134)
        cols = [ship, g("ship_x"), g("ship_y"), g("ship_vx"), g("ship_vy"), g("ship_angle").astype(np.float64), nan, nan, nan,
                fort, g("fort_angle").astype(np.float64), vl, kill_ready, n_missiles, n_missiles] + timers
        return np.stack(cols, 1)
    cols = [ship, g("ship_x") / 90, g("ship_y") / 92, g("ship_vx") / 10, g("ship_vy") / 10, g("ship_angle").astype(np.float64) / 360,
            nan, nan, nan, fort, g("fort_angle").astype(np.float64) / 360, np.maximum(vl, 10) / 10, kill_ready, n_missiles / 20,
            n_missiles / 20] + [t / 5294.0 for t in timers]
    return np.clip(np.stack(cols, 1), -1, 1)


# ---------------------------------------------------------------- the states

FAMILIES = ("dense", "table_pos", "table_vel", "select", "razor", "aim_wrap", "vdir", "ndist")


def _ulp_sides(v):
    return [v, np.nextafter(v, np.inf), np.nextafter(v, -np.inf)]


def _octants(u_, v_):
    """(dy, dx) with |.| = (v, u) in all eight octants"""
    return [(sy * a, sx * b) for a, b in ((v_, u_), (u_, v_)) for sy in (1, -1) for sx in (1, -1)]


def lattice_velocity(rng):
    """a velocity as the game makes it: a sum of 0.3 * (cos, sin)(6 k degrees), added thrust by thrust"""
    vx = vy = 0.0
    for k in rng.integers(0, 60, rng.integers(1, 9)):
        vx += 0.3 * math.cos(math.radians(6.0 * k))
        vy += 0.3 * math.sin(math.radians(6.0 * k))
    return vx, vy


def states():
    """The deterministic inputs: a structured array (family, note, sx, sy, vx, vy, angle) of states in front of one tick without
    keys.  Wherever a family's claim is about where the ship stands AFTER the tick (all but `dense`), sx + vx and sy + vy are
    exact -- the velocity is zero or the numbers have few bits -- and `after_tick` says where that is."""
    rng = np.random.default_rng(20250607)
    rows = []

    def add(fam, note, px, py, vx=0.0, vy=0.0, angle=None):
        """the ship is to stand at (px, py) after its move"""
        sx, sy = px - vx, py - vy
        assert fam == "dense" or (sx + vx == px and sy + vy == py), (fam, note, px, py, vx, vy)
        rows.append((fam, note, sx, sy, vx, vy, int(rng.integers(0, 360)) if angle is None else angle))

    # dense: the play area, velocities as the game makes them and random ones
    for i in range(900):
        v = lattice_velocity(rng) if i % 2 else tuple(rng.uniform(-4, 4, 2))
        add("dense", "lattice" if i % 2 else "random", rng.uniform(20, 690), rng.uniform(20, 606), v[0], v[1], angle=i % 360)
    # table step: min / max on every knot k/16 and every switch point (2k+1)/32 of rint(q * 16), an ulp to either side, in all
    # eight octants; once in the position difference (u = 96: the ship's ulp is 2^-44, the knots' products are integers) ...
    qs = [("knot", k / 16.0) for k in range(17)] + [("switch", (2 * k + 1) / 32.0) for k in range(16)]
    for kind, q in qs:
        for o, (dy, dx) in enumerate(_octants(96.0, q * 96.0)):
            small_is_x = abs(dx) < abs(dy) or (q == 1.0 and o >= 4)
            for j, s in enumerate(_ulp_sides(FORT_X + dx if small_is_x else FORT_Y + dy)):
                add("table_pos", "%s %g oct %d side %d" % (kind, q, o, j), s if small_is_x else FORT_X + dx, FORT_Y + dy if small_is_x else s)
    # ... and once in the velocity (u = 3: every component and its neighbours are doubles; the tick leaves a velocity alone)
    for kind, q in qs:
        for o, (vy, vx) in enumerate(_octants(3.0, q * 3.0)):
            small_is_x = abs(vx) < abs(vy) or (q == 1.0 and o >= 4)
            for j, s in enumerate(_ulp_sides(vx if small_is_x else vy) if kind == "switch" or o % 2 == 0 else [vx if small_is_x else vy]):
                px, py = [(455.0, 250.0), (240.0, 380.0), (300.0, 200.0)][(o + j) % 3]
                rows.append(("table_vel", "%s %g oct %d side %d" % (kind, q, o, j), px, py, s if small_is_x else vx, vy if small_is_x else s,
                             int(rng.integers(0, 360))))
    # octant and axis selects
    for r in (64.0, 150.0):
        for sy_ in (1, -1):
            for sx_ in (1, -1):
                for j, s in enumerate(_ulp_sides(FORT_Y + sy_ * r)):
                    add("select", "diagonal side %d" % j, FORT_X + sx_ * r, s)
    e = 2.0 ** -44  # the ship's ulp next to the fortress's row and column
    for sgn in (1, -1):
        for d in (0.0, 2.0 ** -20 - e, 2.0 ** -20, 2.0 ** -20 + e, -(2.0 ** -20 - e), -(2.0 ** -20 + e), e, -e):
            # 128 * 2^-27 = 2^-20: the hand-over between the core and the near-axis form
            add("select", "y axis dx %g" % d, FORT_X + d, FORT_Y + sgn * 128.0)
            add("select", "negative x axis dy %g" % (sgn * d), FORT_X - 128.0, FORT_Y + sgn * d)
            add("select", "positive x axis dy %g" % (sgn * d), FORT_X + 128.0, FORT_Y + sgn * d)  # (no exact form there)
        for d in (1, 3, 5, 7, 11, 13, 17, 19, 23, 29):  # inside the near-axis form, where x / y is no multiple of the result's ulp
            add("select", "y axis dx %g" % (d * e), FORT_X + d * e, FORT_Y + sgn * 100.0)
            add("select", "negative x axis dy %g" % (sgn * d * e), FORT_X - 100.0, FORT_Y + sgn * d * e)
    # razor hand-over: bearings at k degrees -+ 0.9e-9 and -+ 1.1e-9, either side of the 1e-9 trigger, and on the ray
    for k in (1, 7, 30, 44, 45, 60, 89, 91, 120, 135, 150, 179, -1, -7, -30, -45, -60, -89, -91, -120, -150, -179):
        for off in (0.0, 0.9e-9, -0.9e-9, 1.1e-9, -1.1e-9):
            th = math.radians(k) + math.radians(off)
            r = 150.0 + abs(k) / 8.0
            add("razor", "%d deg %+g" % (k, off), FORT_X + r * math.cos(th), FORT_Y + r * math.sin(th))
    for x in (FORT_X + 150.0, FORT_X - 150.0):
        add("razor", "y == 0", x, FORT_Y)  # (0 and 180 degrees: the razor leaves y == 0 alone)
    # aim wrap: rad2deg(a) - angle + 180 on -180 (bearing -k degrees, angle 360 - k), just above and just below
    for k in range(1, 180, 9):
        for off in (0.0, 0.5e-9, -0.5e-9, 2e-9, -2e-9):
            th = math.radians(-k) + math.radians(off)
            add("aim_wrap", "-%d deg %+g" % (k, off), FORT_X + 170.0 * math.cos(th), FORT_Y + 170.0 * math.sin(th), angle=360 - k)
    # vdir: velocity exactly at and exactly away from the fortress (vdir at 0 and at +-180: v parallel to (fx - sx, sy - fy),
    # the reference's first angle), a last-bit nudge to either side
    for dxp, dyp in ((96.0, 40.0), (-72.0, 24.0), (80.0, -120.0), (-100.0, -52.0), (40.0, 96.0), (-24.0, 72.0), (120.0, 8.0), (-8.0, -120.0)):
        for sgn in (1, -1):
            for j, vy in enumerate(_ulp_sides(sgn * -dyp / 64.0)):
                add("vdir", "%s the fortress, nudge %d" % ("at" if sgn > 0 else "away from", j), FORT_X - dxp, FORT_Y - dyp, sgn * dxp / 64.0, vy)
    for dx in (90.0, -90.0, 171.5, -60.25):  # the fortress row (the second atan2 branch) and an ulp off it
        for j, y in enumerate(_ulp_sides(FORT_Y)):
            for v in ((0.75, 0.0), (-0.75, 0.0), (0.0, 0.0)) + (((0.5, 0.25), (-1.5, -0.5)) if j == 0 else ()):
                add("vdir", "fortress row side %d" % j, FORT_X + dx, y, v[0], v[1])
    for px, py in ((455.0, 250.0), (240.0, 380.0), (300.0, 200.0), (430.0, 400.0)):
        for v in ((1.25, 0.0), (-1.25, 0.0), (0.0, 1.25), (0.0, -1.25)):
            add("vdir", "velocity on an axis", px, py, v[0], v[1])
        for v in ((1e-17, 0.5), (0.5, 1e-17), (1e-17, 1e-17), (-1e-17, 1e-17), (-0.5, -1e-17), (1e-17, -0.5)):
            rows.append(("vdir", "component 1e-17", px, py, v[0], v[1], int(rng.integers(0, 360))))  # (p + 1e-17 == p)
        for v in ((-0.0, 1.0), (1.0, -0.0), (-1.0, -0.0), (-1.0, 0.0), (0.0, -0.0), (-0.0, -0.0), (-0.0, -1.0)):
            add("vdir", "negative zero" if v[0] * v[0] + v[1] * v[1] else "at rest", px, py, v[0], v[1])
        add("vdir", "at rest", px, py)
    # ndist: sx at 355, either side of it, where |dx| = 40 (-1), and at 0, 155, 555 and 710, where the normalised form clamps
    for x in (355.0, 315.0, 395.0, 0.0, 155.0, 555.0, 710.0, 175.0, 215.0, 255.0, 295.0, 415.0, 455.0, 495.0, 535.0):  # (... and monitors' thresholds)
        for j, s in enumerate(_ulp_sides(x) if x else [0.0, 2.0 ** -40]):
            add("ndist", "sx %g side %d" % (x, j), s, 380.0)
    dt = np.dtype([("family", "U12"), ("note", "U48"), ("sx", "f8"), ("sy", "f8"), ("vx", "f8"), ("vy", "f8"), ("angle", "i4")])
    return np.array(rows, dt)


def after_tick(st):
    """where the ships of `states()` stand after one tick without keys (Game::updateShip: pos += vel)"""
    return st["sx"] + st["vx"], st["sy"] + st["vy"]


def family_table(st, errs):
    """{family: max of errs over its lanes}; errs is per lane of a batch tiled over the states (lane i takes state i % P)"""
    fam = st["family"][np.arange(len(errs)) % len(st)]
    return {f: float(np.max(errs[fam == f])) for f in FAMILIES if (fam == f).any()}
