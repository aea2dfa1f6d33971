"""A batch's lifecycle, three times over: every buffer a batch makes lazily or replaces -- the missile slot view, the lane
scratch rows, the tables of another image geometry, the view cache with an eviction, the render resources of a feature batch --
is walked, the batch destroyed, and the next cycle must give the same bytes.  Nothing here provokes an error, and nothing is
said about free device memory: the card is shared."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

N, SEED, STEPS = 64, 7, 40
GEOMETRIES = ((.25, (130, 80, 450, 460), 3), (.3, (100, 60, 500, 520), 2))  # 112 x 115 and 150 x 156 pixels
VIEWS = ((90, 92), (120, 122), (150, 153), (180, 184), (225, 230))  # five of them: one more than the cache holds
GUI = (130, 80, 450, 460)


def _cycle(sfa):
    rng = np.random.default_rng(3)
    script = rng.integers(0, 5, (STEPS, N))
    script[rng.random((STEPS, N)) < .5] = 1  # FIRE half of the time: missiles in flight for the slot view
    out = {}
    img = sfa.SFVecEnv(N, gametype="youturn", obs_type="image", seed=SEED)
    feat = sfa.SFVecEnv(N, gametype="youturn", obs_type="features", seed=SEED)
    try:
        actions = torch.from_numpy(script).to(img.device)
        for name, env in (("img", img), ("feat", feat)):
            env.reset()
            for t in range(STEPS):  # 1. the fixed action script
                obs = env.step_tensors(actions[t])[0]
            out[name + ".obs"] = obs.cpu().numpy()
            # 2. the slot view: made, edited, flushed
            mx = env.get_field("missile_x")
            assert (env.get_field("missile_mask") != 0).any(), "the script must leave missiles in flight"
            env.set_field("missile_x", mx + 1.5)
            out[name + ".missile_x"] = env.get_field("missile_x")
        # 3. the scratch rows: made for one lane, then freed and regrown for three (both batches: same preset, seed, table)
        for dst in (img, feat):
            dst.copy_lanes([5], [9], src=feat)
            dst.copy_lanes([1, 2, 3], [10, 11, 12], src=feat)
        # 4. two other geometries in turn, a frame in each, and back to the default: the device tables are replaced twice
        for k, g in enumerate(GEOMETRIES):
            img.set_image_geometry(*g)
            out["geom%d" % k] = img.render("image").cpu().numpy()
        img.set_image_geometry()
        # 5. five views through the four-entry cache, then the first again: one eviction and one rebuild
        for k, (w, h) in enumerate(VIEWS + VIEWS[:1]):
            out["view%d" % k] = feat.render_view(w, h, GUI, 3.0, True, format="gray", lanes=range(0, 8)).cpu().numpy()
        # 6. one frame of each kind, from both batches (the feature batch makes its render resources here)
        for name, env in (("img", img), ("feat", feat)):
            for mode in ("image", "image-raw"):
                out["%s.%s" % (name, mode)] = env.render(mode).cpu().numpy()
            for f in env.field_names():
                out["%s.field.%s" % (name, f)] = env.get_field(f)
    finally:
        img.close()  # 7.
        feat.close()
    return out


def test_three_lifecycles_give_the_same_bytes():
    import spacefortress_amd as sfa
    from spacefortress_amd import _lib

    assert os.path.exists(_lib.LIB_PATH), "libsfmi.so not built: the GPU tests never fall back"
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    first = _cycle(sfa)
    assert np.array_equal(first["view0"], first["view%d" % len(VIEWS)]), "a rebuilt view draws what the first one drew"
    assert first["img.image"].any() and first["feat.image-raw"].any() and first["geom1"].any() and first["view3"].any()
    for cycle in (2, 3):
        again = _cycle(sfa)
        assert again.keys() == first.keys()
        for k in first:
            assert first[k].dtype == again[k].dtype and first[k].tobytes() == again[k].tobytes(), (cycle, k)
