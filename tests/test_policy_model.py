"""The numpy model of the policy head (tests/policyref.py), held to what it restates.  No GPU.

  * its Philox is the published one on all four counter words (Random123's known answers);
  * its log-probabilities and entropies are log_softmax's and -(p * log p).sum() in float64, to float32's precision;
  * its draws have the row's distribution: over 2^20 consecutive lanes of a fixed stream the counts are constants, and they
    lie within four binomial standard deviations of p * 2^20;
  * the edge counts of the rows the GPU tests use stay under the 0.5 % those tests require;
  * the header declares what the binding binds.
"""
import os
import re

import numpy as np
import pytest
import torch

import policyref as PR


def test_philox_known_answers_on_four_counter_words():
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for c, k, want in kat:
        got = PR.philox4x32_10([np.array([x], np.uint64) for x in c], k)
        assert tuple(int(g[0]) for g in got) == want
    # the head's stream is not the step sampler's: the third counter word differs, and so does every draw looked at
    lanes = np.arange(4096, dtype=np.uint64)
    step = PR.philox4x32_10((lanes, np.uint64(3), np.uint64(0), np.uint64(0)), (7, 0))[0]
    head = PR.draw_words(7, 0, 4096, 3)
    assert (step != head).mean() > 0.99
    # per-wave ticks: env i reads ticks[i // 64]
    ticks = np.array([5, 9], np.uint32)
    w = PR.draw_words(11, 100, 70, ticks)
    assert np.array_equal(w[:64], PR.draw_words(11, 100, 64, 5)) and np.array_equal(w[64:], PR.draw_words(11, 164, 6, 9))


def _rows(kind, n, A, seed):
    r = np.random.default_rng([seed, A])
    if kind == "random":
        return r.standard_normal((n, A)).astype(np.float32)
    if kind == "masked":
        return PR.general_rows(n, A, 1.0, seed)
    x = r.uniform(-80, 80, (n, A)).astype(np.float32)  # a spread of +-80: most of a row underflows to e[k] == 0
    return x


@pytest.mark.parametrize("kind", ["random", "masked", "spread"])
@pytest.mark.parametrize("A", [1, 3, 5, 16, 32])
def test_logp_and_entropy_are_log_softmax_in_float64(kind, A):
    n = 2000
    x = _rows(kind, n, A, 3)
    out = PR.policy_head(x, seed=5)
    assert not out["bad"].any() and (out["action"] >= 0).all() and (out["action"] < A).all()
    assert (np.take_along_axis(out["e"], out["action"][:, None], 1) > 0).all()  # never an action of probability 0
    t = torch.from_numpy(x).double()
    ls, p = torch.log_softmax(t, 1), torch.softmax(t, 1)
    want_logp = ls.gather(1, torch.from_numpy(out["action"])[:, None])[:, 0].numpy()
    plogp = torch.where(p > 0, p * ls, torch.zeros_like(p))  # (0 * -inf: a masked action adds nothing)
    want_ent = -plogp.sum(1).numpy()
    # the model against exact arithmetic: the bounds the device is held to, against the model, hold here a fortiori
    assert (np.abs(out["logp"] - want_logp) <= PR.logp_bound(A, out["xa_minus_m"])).all()
    assert (np.abs(out["entropy"] - want_ent) <= PR.entropy_bound(A)).all()
    # argmax mode: the first maximum, the same entropy
    det = PR.policy_head(x, mode=1)
    assert np.array_equal(det["action"], x.argmax(1)) and np.array_equal(det["entropy"], out["entropy"])
    assert (det["logp"] >= out["logp"]).all()


def test_bad_rows_play_action_zero_and_read_nan():
    x = np.zeros((6, 4), np.float32)
    x[1, 2] = np.nan
    x[2, 0] = np.inf
    x[3] = -np.inf
    x[4, 1:] = -np.inf
    for mode in (0, 1):
        out = PR.policy_head(x, mode=mode, seed=1)
        assert out["bad"].tolist() == [False, True, True, True, False, False]
        assert (out["action"][out["bad"]] == 0).all() and np.isnan(out["logp"][out["bad"]]).all()
        assert np.isnan(out["entropy"][out["bad"]]).all() and not np.isnan(out["logp"][~out["bad"]]).any()
        assert out["action"][4] == 0 and out["logp"][4] == 0 and out["entropy"][4] == 0


FREQ_ROWS = [np.zeros(5, np.float32),
             np.array([1.0, -0.5, 2.0, -np.inf, 0.25], np.float32),
             np.array([3.0, 0.0, -1.0, 2.5, -np.inf, 0.5, 1.5, -2.0, 0.0, 0.0, -np.inf, 1.0, -4.0, 2.0, 0.75, -0.25], np.float32)]


@pytest.mark.parametrize("r", range(3))
def test_frequencies_over_a_million_lanes_of_the_fixed_stream(r):
    N, row = 1 << 20, FREQ_ROWS[r]
    out = PR.policy_head(np.broadcast_to(row, (N, row.size)), seed=0x5EED0000 + r, first_lane=12345, ticks=2)
    counts = np.bincount(out["action"], minlength=row.size)
    p = torch.softmax(torch.from_numpy(row).double(), 0).numpy()
    sd = np.sqrt(N * p * (1 - p))
    assert (counts[p == 0] == 0).all()
    assert (np.abs(counts - p * N) <= 4 * sd).all(), (counts, p * N, sd)


def test_the_gpu_tests_rows_are_seldom_on_the_edge():
    """tests/test_gpu_policy_head.py requires at most 0.5 % of a case's rows within the margin of a boundary: a property of
    the model and the chosen seeds, checked here for every general case it runs."""
    import test_gpu_policy_head as G

    for n, A, scale, seed in G.GENERAL_CASES:
        x = PR.general_rows(n, A, scale, seed)
        for tick in range(3):
            out = PR.policy_head(x, seed=G.SEED, first_lane=G.FIRST_LANE, ticks=tick)
            assert (out["edge"] <= PR.edge_margin(A)).sum() <= 0.005 * n, (n, A, scale, seed, tick)


def test_header_declares_what_the_binding_binds():
    import spacefortress_amd
    from spacefortress_amd import _lib as lib
    from spacefortress_amd import build as sfbuild

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.path.join(root, "include", "sfmi_policy.h")
    bare = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    assert set(re.findall(r"\b(sf_[a-z_0-9]+)\s*\(", bare)) == set(lib.POLICY_SYMBOLS) == {"sf_policy_sample"}
    m = re.search(r"sf_policy_sample\(([^)]*)\)", bare)
    assert m and len(m.group(1).split(",")) == len(lib.POLICY_SYMBOLS["sf_policy_sample"][1]) == 14
    assert os.path.abspath(path) in [os.path.abspath(h) for h in sfbuild.HEADERS if os.path.isabs(h)]
    assert "sf_policy.hip" in sfbuild.SOURCES
    assert "PolicyHead" in spacefortress_amd.__all__
    # the header's constants are the binding's and the model's
    defs = dict(re.findall(r"#define (SF_POLICY_[A-Z_]+) (\w+)", bare))
    assert int(defs["SF_POLICY_SAMPLE"]) == lib.POLICY_SAMPLE and int(defs["SF_POLICY_ARGMAX"]) == lib.POLICY_ARGMAX
    assert int(defs["SF_POLICY_MAX_ACTIONS"]) == lib.POLICY_MAX_ACTIONS
    assert int(defs["SF_POLICY_COUNTER_WORD"].rstrip("u"), 16) == PR.COUNTER_WORD


def test_the_built_library_exports_the_call():
    from spacefortress_amd import _lib
    from spacefortress_amd import build as sfbuild

    sfbuild.build()
    assert hasattr(_lib.lib(), "sf_policy_sample")
