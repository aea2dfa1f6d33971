"""Timing of sf_render_view (HIP events): 1, 16 and 256 lanes in the GUI view (450 x 460) and Game's default view (710 x 626),
colour, BGRx, on a batch in mid-game (explosions, missiles, shells).  One JSON line per case.
    python tools/view_probe.py [reps]
The bytes written are the yardstick: 450 x 460 x 4 = 828 KB per lane (8 TB/s HBM: 0.1 us per lane)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spacefortress_amd import SFVecEnv  # noqa: E402

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 50
env = SFVecEnv(256, gametype="youturn", obs_type="features")
env.reset()
env.seed_actions(1)
for _ in range(400):
    env.step_sampled()
views = {"gui": dict(viewport=(130, 80, 450, 460)), "game": dict()}
for name, v in views.items():
    for n in (1, 16, 256):
        out = env.render_view(**v, lanes=range(0, n))
        for _ in range(3):
            env.render_view(**v, lanes=range(0, n), out=out)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            env.render_view(**v, lanes=range(0, n), out=out)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1000.0 / reps
        mb = out.numel() / 1e6
        print(json.dumps(dict(view=name, shape=list(out.shape[1:]), lanes=n, us_per_call=round(us, 1), us_per_lane=round(us / n, 2),
                              mb_written=round(mb, 2), gb_per_s=round(mb / us * 1e3, 1), reps=reps)))
env.close()
