"""Lane states on the host (no GPU): the row format include/sfmi.h documents, the Python constants that mirror it, and the
argument errors the C ABI decides before it launches anything."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from spacefortress_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _define(name):
    txt = open(os.path.join(ROOT, "include", "sfmi.h")).read()
    m = re.search(r"#define %s (0x[0-9A-Fa-f]+|\d+)" % name, txt)
    return int(m.group(1), 0)


def test_row_size_and_header_constants():
    L = _lib.lib()
    assert L.sf_lane_state_bytes() == _define("SF_LANE_STATE_BYTES") == _lib.LANE_STATE_BYTES == 1136
    assert _lib.LANE_STATE_BYTES % 16 == 0
    assert _define("SF_LANE_STATE_MAGIC") == _lib.LANE_STATE_MAGIC
    assert _define("SF_LANE_STATE_VERSION") == _lib.LANE_STATE_VERSION
    # the documented layout: header, 7 chunks, 40 shell pieces, 20 missile pieces, headings (20 x uint16) + 8 pad bytes
    assert 16 + 7 * 16 + 40 * 16 + 20 * 16 + 48 == _lib.LANE_STATE_BYTES


def test_argument_errors_before_any_launch():
    L = _lib.lib()
    rows = np.zeros((4, _lib.LANE_STATE_BYTES), np.uint8)
    p = rows.ctypes.data_as(C.c_void_p)
    assert L.sf_save_lanes(None, None, _lib.ACT_I32, 4, p, None) == _lib.SF_ERR_ARG
    assert L.sf_load_lanes(None, None, _lib.ACT_I64, 4, p, 4, None, None, None) == _lib.SF_ERR_ARG
    assert L.sf_copy_lanes(None, None, None, None, _lib.ACT_I32, 4, None, None) == _lib.SF_ERR_ARG
    assert L.sf_check_lanes(None, None) == _lib.SF_ERR_ARG
    hdr = np.zeros(4, np.uint32)
    assert L.sf_lane_state_header(None, hdr.ctypes.data_as(C.c_void_p)) == _lib.SF_ERR_ARG


def test_lane_states_container_on_the_host(tmp_path):
    torch = pytest.importorskip("torch")
    from spacefortress_amd.lanes import LaneStates

    with pytest.raises(ValueError):
        LaneStates(torch.zeros((3, 100), dtype=torch.uint8), "youturn", 1, 65536)
    rows = torch.arange(3 * _lib.LANE_STATE_BYTES, dtype=torch.int64).remainder(251).to(torch.uint8).reshape(3, -1)
    hdr = np.array([_lib.LANE_STATE_MAGIC | _lib.LANE_STATE_VERSION, 1, 7, 65536], np.uint32)
    rows[:, :16] = torch.from_numpy(hdr.view(np.uint8).copy())
    s = LaneStates(rows, "autoturn", 7, 65536, build_id="x")
    assert len(s) == 3 and len(s[1]) == 1 and len(s[[0, 2]]) == 2
    assert np.array_equal(s.headers(), np.tile(hdr, (3, 1)))
    assert torch.equal(s[2].rows[0], rows[2])
    s.save(tmp_path / "rows.pt")
    t = LaneStates.load(tmp_path / "rows.pt")
    assert torch.equal(t.rows, rows) and (t.gametype, t.seed, t.spawn_table_len, t.build_id) == ("autoturn", 7, 65536, "x")
    torch.save(s, tmp_path / "obj.pt")
    u = torch.load(tmp_path / "obj.pt", weights_only=False)
    assert torch.equal(u.rows, rows) and u.seed == 7
