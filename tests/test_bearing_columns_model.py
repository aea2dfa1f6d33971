"""tests/bearingref.py proved on the host: the 70-digit reference against an independent library, the bounds as the sums of
their terms, the generator's states against what each family claims of itself, and a host restatement of the kernels' code
(tests/native/bearing_cols.c: sf_atan2_core, sf_atan2<true> with both exact forms, compute_extras, the three writers) held to
the reference by the very rules the GPU test applies (tests/test_gpu_bearing_columns.py).  That run says whether reference,
bounds and inputs are consistent, and whether the share conditions of `monitors` hold; three mutants of the restatement must
FAIL it -- a tolerance that lets them pass is what this file is here to prevent.

The angles themselves are held too, which only the host can see: the core within its 1e-15 rad, the exact forms to half an ulp.
That is where the second mutant shows: pi's low part is 1.2e-16 rad, 7e-15 degrees, a third of a rounding of `- angle`, so no
bound on the COLUMNS that is derived from the roundings can notice its loss; the angle's half ulp does."""
import math
import os
import subprocess
from decimal import Decimal, localcontext
from fractions import Fraction

import numpy as np
import pytest

import bearingref as br

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MUTANTS = {"MUT_NO_SEVENTH": "the series without its 1/7 term", "MUT_PI_LO": "the near-axis form without pi's low part",
           "MUT_VDIR_SIGN": "M_PI - a_pos with the wrong sign on dy < 0"}


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    """the states, where they stand after the tick, the reference there, and the host model's rows (per build)"""
    st = br.states()
    px, py = br.after_tick(st)
    ref = br.reference(px, py, st["vx"], st["vy"], st["angle"])
    tmp = tmp_path_factory.mktemp("bearing_cols")
    inp = str(tmp / "in.bin")
    np.stack([px, py, st["vx"], st["vy"], st["angle"].astype(np.float64)], 1).tofile(inp)

    def model(define=None, mode="core"):
        exe = str(tmp / ("model_" + (define or "plain")))
        if not os.path.exists(exe):
            subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "spacefortress_amd", "csrc")]
                                  + (["-D" + define] if define else [])
                                  + [os.path.join(ROOT, "tests", "native", "bearing_cols.c"), "-o", exe, "-lm"])
        out = str(tmp / "out.bin")
        subprocess.check_call([exe, mode, inp, out])
        return np.fromfile(out).reshape(len(st), -1)

    return st, px, py, ref, model


def _hold(st, px, py, ref, rows):
    """Every rule of bearingref on the model's rows.  Returns ({check: {family: worst, in units of its bound}}, [failures])."""
    table, bad = {}, []

    def note(name, err, ok):
        table[name] = br.family_table(st, err)
        seen = {}
        for i in np.flatnonzero(~ok):  # (up to three per family)
            f = str(st["family"][i])
            seen[f] = seen.get(f, 0) + 1
            if seen[f] <= 3:
                bad.append((name, f, str(st["note"][i]), float(err[i])))

    for name, col, key, rule in (("aim f64", 2, "aim", br.RULES["features"][6]), ("vdir f64", 3, "vdir", br.RULES["features"][7]),
                                 ("naim f64", 5, "naim", br.RULES["normalized-features"][6]),
                                 ("nvdir f64", 6, "nvdir", br.RULES["normalized-features"][7])):
        note(name, *br.check_column(rows[:, col], ref[key], *rule))
    for name, col, key, rule in (("aim f32", 14, "aim", br.RULES["features"][6]), ("vdir f32", 15, "vdir", br.RULES["features"][7]),
                                 ("naim f32", 17, "naim", br.RULES["normalized-features"][6]),
                                 ("nvdir f32", 18, "nvdir", br.RULES["normalized-features"][7])):
        note(name, *br.check_column(rows[:, col].astype(np.float32), ref[key], *rule, f32=True))
    # ndist: bit for bit, its float32 and its clamp
    for name, col, want in (("ndist", 4, ref["ndist"]), ("nndist", 7, ref["nndist"]), ("ndist f32", 16, ref["ndist"].astype(np.float32)),
                            ("nndist f32", 19, ref["nndist"].astype(np.float32))):
        ok = rows[:, col] == want
        note(name, (~ok).astype(np.float64), ok)
    # vdir of a ship at rest is 0.0 exactly
    rest = st["vx"] * st["vx"] + st["vy"] * st["vy"] == 0.0
    ok = ~rest | (rows[:, 3] == 0.0)
    note("vdir at rest", (~ok).astype(np.float64), ok)
    # monitors, with the band
    want, free = br.monitors_columns(ref)
    ok = ((rows[:, 8:14] == want) | free).all(1)
    note("monitors", (~ok).astype(np.float64), ok)
    # the angles: the core within its contract, the exact forms correctly rounded
    with localcontext(br.CTX):
        for name, col, args in (("a_pos", 0, (py - br.FORT_Y, px - br.FORT_X)), ("a_vel", 1, (st["vy"], st["vx"]))):
            err, ok = np.zeros(len(st)), np.ones(len(st), bool)
            for i in range(len(st)):
                if col == 1 and rest[i]:
                    continue
                a = rows[i, col]
                exact_form = col == 0 and rows[i, 20] != 0
                lim = Decimal(math.ulp(a)) / 2 if exact_form else Decimal(br.ANGLE_CORE)
                e = abs(Decimal(a) - br.atan2_hp(float(args[0][i]), float(args[1][i])))
                err[i], ok[i] = float(e / lim), e <= lim
            note(name, err, ok)
    return table, bad


def _print(title, table):
    fams = [f for f in br.FAMILIES]
    print("\n" + title)
    print("%-14s" % "check" + "".join("%11s" % f for f in fams))
    for name, row in table.items():
        print("%-14s" % name + "".join("%11.3g" % row[f] if f in row else "%11s" % "-" for f in fams))


# ---------------------------------------------------------------- the reference and the bounds

def test_reference_against_mpmath():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 80
    with localcontext(br.CTX):
        assert abs(br.PI - Decimal(str(mp.pi))) < Decimal(10) ** -66
        rng = np.random.default_rng(5)
        args = [(0.0, -1.0), (-0.0, -1.0), (1.0, 0.0), (-1.0, 0.0), (0.0, 1.0), (-0.0, 1.0), (3.0, 3.0), (1e-17, -0.5), (0.5, 1e-17)]
        args += [tuple(rng.uniform(-400, 400, 2)) for _ in range(200)]
        for y, x in args:
            want = mp.atan2(mp.mpf(y), mp.mpf(x))
            if y == 0 and math.copysign(1, y) < 0 and x < 0:
                want = -mp.pi  # (mpmath has no signed zero)
            assert abs(br.atan2_hp(y, x) - Decimal(mp.nstr(want, 75))) < Decimal(10) ** -64, (y, x)
    for y, x in args[6:60]:
        assert abs(br.atan2_correctly_rounded(y, x) - math.atan2(y, x)) <= math.ulp(math.atan2(y, x))


def test_bounds_are_the_sums_of_their_terms():
    assert br.AIM_BOUND == sum(br.AIM_TERMS.values()) and br.VDIR_BOUND == sum(br.VDIR_TERMS.values())
    assert len(br.AIM_TERMS) == 7 and len(br.VDIR_TERMS) == 10
    # what the docstring derives: 1.88e-13 and 2.18e-13 degrees; every term is a rounding or a contract, none above 6e-14
    assert abs(br.AIM_BOUND - 1.88e-13) < 1e-15 and abs(br.VDIR_BOUND - 2.18e-13) < 1e-15
    assert max(list(br.AIM_TERMS.values()) + list(br.VDIR_TERMS.values())) < 6e-14
    assert br.u(1) == 2.0 ** -54 and br.u(256) * 2 == math.ulp(200.0) and br.u(4) * 2 == math.ulp(math.pi)


# ---------------------------------------------------------------- the generator's claims

def test_the_states_are_what_their_families_claim(world):
    st, px, py, ref, model = world
    assert 2500 <= len(st) <= 3600 and set(st["family"]) == set(br.FAMILIES)
    assert len(br.states()) == len(st) and br.states().tobytes() == st.tobytes()  # deterministic
    rows = model()
    fam, note = st["family"], st["note"]
    dx, dy = px - br.FORT_X, py - br.FORT_Y
    # table step: per knot / switch point and octant the three sides give min / max on q, above it and below it
    for f, a, b in (("table_pos", dy, dx), ("table_vel", st["vy"], st["vx"])):
        groups = {}
        for i in np.flatnonzero(fam == f):
            groups.setdefault(str(note[i]).rsplit(" side", 1)[0], []).append(i)
        full = 0
        for key, idx in groups.items():
            q = Fraction(float(key.split()[1]))
            rel = []
            for i in idx:
                u_, v_ = max(abs(a[i]), abs(b[i])), min(abs(a[i]), abs(b[i]))
                rel.append((Fraction(v_) > q * Fraction(u_)) - (Fraction(v_) < q * Fraction(u_)))
            assert rel[0] == 0, (f, key)  # on the knot / the switch point exactly
            if len(idx) == 3:
                full += 1
                assert sorted(rel) == [-1, 0, 1] or (q == 0 and sorted(rel) == [0, 1, 1]) or (q == 1 and sorted(rel) == [-1, -1, 0]), (f, key, rel)
                if key.startswith("switch"):  # rint(q * 16) really switches between the two sides
                    ks = {r: math.floor(Fraction(float(min(abs(a[i]), abs(b[i])))) / Fraction(float(max(abs(a[i]), abs(b[i])))) * 16 + Fraction(1, 2))
                          for r, i in zip(rel, idx) if r}
                    assert ks[1] == ks[-1] + 1, (f, key, ks)
        assert len(groups) == 33 * 8 and full >= 16 * 8
    # selects: which form the restatement takes
    form = rows[:, 20]
    sel = fam == "select"
    for i in np.flatnonzero(sel):
        n = str(note[i])
        if n.startswith("diagonal side 0"):
            assert abs(dx[i]) == abs(dy[i])
        elif n.startswith("diagonal"):
            assert abs(dx[i]) != abs(dy[i]) and abs(abs(dx[i]) - abs(dy[i])) < 1e-13
        elif n.startswith(("y axis", "negative x axis")):
            small, big = (dx[i], dy[i]) if n.startswith("y axis") else (dy[i], dx[i])
            assert abs(big) in (100.0, 128.0) and (form[i] == 1) == (abs(small) * 2.0 ** 27 < abs(big)), (n, small, form[i])
        else:
            assert dx[i] == 128.0 and form[i] == (0 if dy[i] == 0 or abs(dy[i]) > 1e-12 else 2), (n, form[i])
    assert {0.0, 1.0} <= set(form[sel]) and (np.abs(dx[sel]) == 2.0 ** -20).any() and (np.abs(dy[sel]) == 2.0 ** -20).any()
    # razor: the exact bearing sits where the note says, and the trigger takes the side it should
    deg = br.bearings(px, py)
    for i in np.flatnonzero(fam == "razor"):
        n = str(note[i])
        if n == "y == 0":
            assert dy[i] == 0 and form[i] == (1 if dx[i] < 0 else 0)
            continue
        k, off = int(n.split()[0]), float(n.split()[2])
        d = abs(float(deg[i] - k))
        assert abs(d - abs(off)) < 2e-12, (n, d)
        assert form[i] == (2 if abs(off) < 1e-9 else 0), (n, form[i])
    # aim wrap: on the ray the aim is within the bound of the wrap, the others are beside it and outside the band
    band = br.aim_band(ref["aim"])
    for i in np.flatnonzero(fam == "aim_wrap"):
        off = float(str(note[i]).split()[2])
        a = float(ref["aim"][i])
        assert min(abs(a + 180), abs(a - 180)) < 3e-9 and band[i] == (off == 0.0), (note[i], a)
        if off:
            assert (a > 0) == (off < 0)  # below -180 the aim wraps to the top of its range
    # vdir: at and away from the fortress, the nudges on either side
    for key, centre in (("at the fortress", 0), ("away from the fortress", 180)):
        for j in (0, 1, 2):
            off = np.array([float(abs(ref["vdir"][i]) - centre) for i in np.flatnonzero((fam == "vdir") & (note == "%s, nudge %d" % (key, j)))])
            assert len(off) == 8
            assert (np.abs(off) < 1e-30).all() if j == 0 else ((np.abs(off) > 1e-16) & (np.abs(off) < 1e-12)).all(), (key, j, off)
    row = (fam == "vdir") & np.char.startswith(note, "fortress row side 0")
    assert row.sum() == 20 and (dy[row] == 0).all()
    off_row = (fam == "vdir") & np.char.startswith(note, "fortress row side") & ~row
    assert off_row.sum() == 24 and (np.abs(dy[off_row]) == 2.0 ** -44).all()
    nz = (fam == "vdir") & (note == "negative zero")
    assert nz.sum() == 20 and (np.signbit(st["vx"][nz]) | np.signbit(st["vy"][nz])).all()
    rest = st["vx"] * st["vx"] + st["vy"] * st["vy"] == 0.0
    assert ((fam == "vdir") & rest).sum() >= 16 and all(ref["vdir"][i] == 0 for i in np.flatnonzero(rest))
    # ndist: the clamps and every threshold of monitors are met exactly
    nd = ref["ndist"][fam == "ndist"]
    assert {-1.5, -1.0, 1.0, 0.75, 0.25, -0.25, -0.75} <= set(nd.tolist()) and nd.max() > 2.9
    assert (ref["nndist"] <= 1).all() and (ref["nndist"] >= -1).all()
    # the share of monitors' values inside a band
    assert band.mean() < br.BAND_SHARE_MAX, band.mean()
    print("\nstates: %d; per family: %s; aim within its bound of a threshold: %.2f %%"
          % (len(st), {f: int((fam == f).sum()) for f in br.FAMILIES}, 100 * band.mean()))


# ---------------------------------------------------------------- the host model and its mutants

@pytest.mark.parametrize("mode", ["core", "libm"])
def test_host_restatement_holds_the_bounds(world, mode):
    """`core`: the step kernel's form (table step, exact forms); `libm`: a new game's (the C library's atan2, exact forms)."""
    st, px, py, ref, model = world
    table, bad = _hold(st, px, py, ref, model(mode=mode))
    _print("host restatement (%s): worst per family, in units of the bound" % mode, table)
    assert not bad, bad[:10]
    # the bounds are neither missed nor idle: the worst column error is a fair share of its bound
    worst = max(max(table[k].values()) for k in ("aim f64", "vdir f64"))
    assert 0.05 < worst <= 1.0, worst


@pytest.mark.parametrize("define", sorted(MUTANTS))
def test_mutants_fail(world, define):
    st, px, py, ref, model = world
    table, bad = _hold(st, px, py, ref, model(define=define))
    _print("mutant %s (%s)" % (define, MUTANTS[define]), table)
    failing = sorted({(name, fam) for name, fam, _, _ in bad})
    print("fails:", failing)
    assert bad, "the bounds let %s pass" % define
    # (float32 cannot see the first two: 2.4e-10 degrees is 1e-5 of a float32 ulp at 180, and no state sits that close to a tie)
    expect = {"MUT_NO_SEVENTH": [("aim f64", "table_pos"), ("vdir f64", "table_vel"), ("naim f64", "table_pos"), ("a_pos", "table_pos")],
              "MUT_PI_LO": [("a_pos", "select")], "MUT_VDIR_SIGN": [("vdir f64", "vdir"), ("nvdir f32", "dense")]}[define]
    assert set(expect) <= set(failing), failing
