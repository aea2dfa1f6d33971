"""The step kernel computes what a tick's missile events do to the fortress and the score in closed form, from the number
of hits and misses (spacefortress_amd/csrc/sf_events.h), where the reference walks the missile slots in order
(SRC/game.cpp:353-402).  tests/native/event_replay.c compiles that very header on the host and holds it to a slot-order walk,
exhaustively: fortress alive and dead, fort_vuln_timer on both sides of the window's edge, vlner 0..13, every sequence of up to
six events, four starting scores, both scorings; all outputs and the float bits of the three score words."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spacefortress_amd", "csrc")


def test_closed_form_equals_the_slot_order_walk(tmp_path):
    exe = str(tmp_path / "event_replay")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-I" + CSRC,
                           os.path.join(ROOT, "tests", "native", "event_replay.c"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout
    # 2 scorings x 2 x 5 timers x 14 vlner x (2^0 + ... + 2^6 = 127 sequences) x 4 scores
    assert "mismatches=0 of %d" % (2 * 2 * 5 * 14 * 127 * 4) in out.stdout, out.stdout


def test_the_kernel_uses_the_checked_function_and_its_constants():
    """The kernel calls sf_missile_events with the constants the host program uses, keeps no event loop, and asserts the
    zero miss penalty the closed form rests on."""
    src = open(os.path.join(CSRC, "sf_kernels.hip")).read()
    lay = open(os.path.join(CSRC, "sf_layout.h")).read()
    assert '#include "sf_events.h"' in src and src.count("sf_missile_events(") == 1
    assert "sfc::vuln_time, sfc::vuln_threshold, sfc::Score<SHAPED>::destroy_reward)" in src
    assert "static_assert(sfc::Score<false>::miss_penalty == 0.0f && sfc::Score<true>::miss_penalty == 0.0f" in src
    assert not re.search(r"while\s*\(\s*__ballot\(ev\b", src)
    assert "vuln_time = 250" in lay and "vuln_threshold = 10" in lay
    assert "destroy_reward = SHAPED ? 1.0f : 100.0f" in lay
