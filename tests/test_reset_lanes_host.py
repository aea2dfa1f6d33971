"""The masked reset's surface without a GPU: the exports are declared, bound and refuse NULL arguments with a text before any
device work (include/sfmi.h: sf_reset_lanes; include/sfmi_masked.h: sf_eplog_restart_where); the wrappers name the reason they have no reset_lanes."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from spacefortress_amd import _lib, build

    build.build()
    return _lib


def test_the_header_declares_what_the_library_binds(lib):
    text = open(os.path.join(ROOT, "include", "sfmi.h")).read()
    masked = open(os.path.join(ROOT, "include", "sfmi_masked.h")).read()
    for name, n_args, hdr, table in (("sf_reset_lanes", 4, text, lib.SYMBOLS),
                                     ("sf_eplog_restart_where", 3, masked, lib.MASKED_SYMBOLS)):
        m = re.search(r"^int %s\(([^)]*)\);" % name, hdr, re.M)
        assert m and len(m.group(1).split(",")) == n_args, name
        assert len(table[name][1]) == n_args
        assert hasattr(lib.lib(), name)
    bare = re.sub(r"/\*.*?\*/", "", masked, flags=re.S)
    assert set(re.findall(r"\b(sf_[a-z_0-9]+)\s*\(", bare)) == set(lib.MASKED_SYMBOLS)
    assert "ENV:163-178" in masked
    assert "ENV:163-178" in text[text.index("env.reset() in the envs the caller chooses"):text.index("int sf_reset_lanes")]


def test_null_arguments_are_refused_with_a_text(lib):
    L = lib.lib()
    assert L.sf_reset_lanes(None, None, None, None) == lib.SF_ERR_ARG and b"sf_reset_lanes" in L.sf_last_error()
    assert L.sf_eplog_restart_where(None, None, None) == lib.SF_ERR_ARG and b"sf_eplog_restart_where" in L.sf_last_error()


def test_the_wrappers_name_their_reason(lib):
    from spacefortress_amd.framestack import FrameStack
    from spacefortress_amd.rollout import DeviceRollout
    from spacefortress_amd.frame_rollout import FrameRollout
    from spacefortress_amd.vecnormalize import SFVecNormalize

    for cls in (FrameStack, DeviceRollout, FrameRollout, SFVecNormalize):
        w = cls.__new__(cls)  # (no device needed: the refusal does not look at the instance)
        assert not hasattr(w, "reset_lanes")
        with pytest.raises(AttributeError, match="%s has no reset_lanes" % cls.__name__):
            w.reset_lanes
