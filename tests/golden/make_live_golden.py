#!/usr/bin/env python3
"""Generate tests/golden/live_reference.json: the runs of tests/test_oracle_golden.py's two live tests
(test_oracle_vs_reference_live, test_oracle_vs_reference_live_kills) played by the REAL reference engine, kept as digests
(tests/test_oracle_golden.py::digest) so that the tests hold the oracle to them where oracle/_ref is not built; and, under
"renderer", the sha256 of the frames the reference's own renderer drew in tests/test_frames_golden.py's live run.

Run in the build container only (needs the reference; builds oracle/_ref via oracle/Makefile).  The output is data --
sha256 digests of the states / rewards the reference produced, and counts -- never reference source.

    python tests/golden/make_live_golden.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from oracle import oracle as O  # noqa: E402
from test_frames_golden import live_renderer_ticks  # noqa: E402
from test_oracle_golden import digest, live_kill_runs, live_random_runs, shaped_reward  # noqa: E402


def main():
    O.build()
    assert O.have_ref() and O.have_refdraw(), "oracle/_ref/libsfref.so or libsfrefdraw.so missing: needs the reference + cairo"
    out = {}
    for gametype in ("youturn", "autoturn", "test-youturn", "test-autoturn"):
        shaped = gametype in ("youturn", "autoturn")
        rec = out[gametype] = {}
        for aset, _, keys, acts in live_random_runs(O, gametype):
            rr = O.RefGame(gametype).replay(keys[acts])
            rec["random_aset%d" % aset] = digest(rr["snaps"], rr["done"], shaped_reward(rr["eng_reward"], rr["snaps"]["vlner"], shaped))
        r = O.RefGame(gametype)
        rec["rollout"] = int(r.rollout(500000, 11))
        rec["rollout_snapshot"] = digest(r.snapshot())
        for policy, _, keys, acts in live_kill_runs(O, gametype):
            rr = O.RefGame(gametype).replay(keys[acts])
            rec["kills_" + policy] = digest(rr["snaps"], rr["done"], shaped_reward(rr["eng_reward"], rr["snaps"]["vlner"], shaped))
            rec["kills_%s_engine_rewards" % policy] = int((np.asarray(rr["eng_reward"]) > 0).sum())
    out["renderer"] = {}
    for gametype in ("youturn", "autoturn"):
        g = O.RefDrawGame(gametype, seed=7, spawn_skip=3)
        h = hashlib.sha256()
        for _ in live_renderer_ticks(g):
            h.update(g.draw().tobytes())
        out["renderer"][gametype] = h.hexdigest()
    with open(os.path.join(HERE, "live_reference.json"), "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", os.path.join(HERE, "live_reference.json"))


if __name__ == "__main__":
    main()
