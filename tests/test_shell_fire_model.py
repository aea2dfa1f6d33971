"""A split launch of the step kernel leaves the arithmetic of the shell the fortress fires to the tile's missile wave, and the
new shell out of the games' wave's shell walk on the tick it is fired (spacefortress_amd/csrc/sf_kernels.hip, updateFortress).
That rests on geometry: the ship is alive behind updateShip, so it is not inside the small hexagon; the shell sits shell_speed
= 6 from the fortress; shell and ship collide at 13.  tests/native/shell_fire_model.cpp compiles the kernel's own small-hexagon
test (its text, taken out of sf_lane_dev.h here) over sf_layout.h's edge constants on the host and checks

  * on a dense disc of points around the hexagon (7 200 directions x radii 0 .. 48 in steps of 1 / 128), on its vertices and
    edge midpoints and a hair to either side of them: every point the test REJECTS is farther from the fortress than 19;
  * the smallest such distance against the analytic inradius (the nearest edge line: 34, the bottom edge);
  * the shot's first position, formed as the kernel forms it, inside the play area for 720 000 directions.

The margin: a rejected point is at more than 34 from the fortress, 15 more than the 19 that a first-tick collision needs."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spacefortress_amd", "csrc")
MARGIN = 15.0  # inradius 34 - (shell_speed 6 + collision radius 13)


def _small_hex_text():
    """SF_EDGE_TEST and inside_small_hex as sf_lane_dev.h has them."""
    dev = open(os.path.join(CSRC, "sf_lane_dev.h")).read()
    macro = re.search(r"#define SF_EDGE_TEST\(nx, ny, px, py\).*?\n(?=__device__)", dev, re.S).group(0)
    fn = re.search(r"__device__ __forceinline__ bool inside_small_hex\(double x, double y\) \{.*?\n\}\n", dev, re.S).group(0)
    assert "SF_SMALL_HEX_EDGES(SF_EDGE_TEST)" in fn and "return !(m < 0);" in fn
    return macro + fn


def test_every_rejected_point_is_out_of_the_new_shells_reach(tmp_path):
    (tmp_path / "small_hex_extract.h").write_text(_small_hex_text())
    exe = str(tmp_path / "shell_fire_model")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + CSRC, "-I" + str(tmp_path),
                           os.path.join(ROOT, "tests", "native", "shell_fire_model.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0, out.stdout
    v = {k: float(x) for k, x in re.findall(r"(\w+)=([-0-9.e+]+)", out.stdout)}
    assert v["violations"] == 0 and v["outside"] == 0 and v["fast"] == 0
    assert v["inradius"] == 34.0                                     # the bottom edge, y = 349
    assert v["inradius"] < v["min_rejected"] <= v["inradius"] + 0.01  # strictly beyond the line; the disc's step is 1 / 128
    assert v["min_rejected"] - 19.0 >= MARGIN
    assert v["rejected"] > 1e7 and v["accepted"] > 1e7               # both sides of the boundary were probed
    assert v["max_speed"] <= 6.0 + 1e-12


def test_the_kernel_fires_only_for_a_ship_alive_behind_update_ship():
    """The tick's order, and the split launch's hand-over as the record describes it: the decision in the games' wave, the
    arithmetic in the missile wave, the new bit out of the walk."""
    src = open(os.path.join(CSRC, "sf_kernels.hip")).read()
    lay = open(os.path.join(CSRC, "sf_layout.h")).read()
    ship, fort, shells = (src.index("// ---- " + s) for s in ("updateShip (", "updateFortress (", "updateShells ("))
    assert ship < fort < shells
    body = src[fort:shells]
    assert "const bool ship_up = L.fl & SF_FL_SHIP_ALIVE;" in body                       # read behind updateShip
    assert "const bool lock = ship_up && L.fort_t >= sfc::lock_time && (L.fl & SF_FL_FORT_ALIVE);" in body
    assert "const bool fire = lock && slot < SF_NSLOT;" in body
    assert "if (lane == 0u) hflags[3] = shot;" in body                                   # on every path: straight-line code
    assert src.index("hflags[1] = 0x80000000u | wp;") < src.index("hflags[3])) == 0u && ++spins < kSpinLimit") < src.index("hflags[2] = 1u;")
    assert "const double nrm = sqrt(dd.x * dd.x + dd.y * dd.y);" in src
    assert "sfc::shell_speed * (dd.x / nrm), svy = sfc::shell_speed * (dd.y / nrm);" in src
    assert "if constexpr (SPLIT) L.smask |= new_s_bit;" in src[shells:]
    assert "shell_speed = 6" in lay and "shell_hit_r2 = 13.0 * 13.0" in lay and "width_d = 710, height_d = 626" in lay
