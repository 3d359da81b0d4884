"""gfw_flow_pyrlk's kernels (gyroflow_amd/csrc/gfw_flow.hip) and the entry point's check and staging (gfw_flow_host.h) interpreted on the host (tests/_emu_flow.py)
against the fixed-point statement (tests/_flowstmt.py): every next, status, per-level iteration count, the compacted arrays and the grid points, bit for bit, over
tests/_flowcase.ALL_SPECS (the analytic scenes and the out-of-level exit case) — with the frames and every pyramid level between inaccessible pages, once with their last and once with their first byte against one.
The statement's result of a case is computed once and shared with tests/test_gpu_flow.py."""
import numpy as np
import pytest

import _emu_flow as EF
import _flowcase as FC
import _flowstmt as FS

NAMES = sorted(FC.ALL_SPECS)


@pytest.mark.parametrize("guard", ["end", "start"])
@pytest.mark.parametrize("name", NAMES)
def test_interpreted_kernels_equal_the_statement_to_the_bit(name, guard):
    c = FC.case(name)
    FC.assert_equal_to_statement(EF.flow_pyrlk(c.frames, c.width, c.pairs, c.features, guard=guard), c.statement, name)


@pytest.mark.parametrize("guard", ["end", "start"])
@pytest.mark.parametrize("name", NAMES)
def test_the_grid_mode_equals_the_statement_to_the_bit(name, guard):
    c = FC.case(name)
    got = EF.flow_pyrlk(c.frames, c.width, c.pairs, None, guard=guard)
    FC.assert_equal_to_statement(got, c.grid_statement, name + " grid", FC.GRID_OUTPUTS)
    if name in FC.SPECS:
        assert 10 < got["grid_counts"].min() and got["grid_counts"].max() < got["grid_points"].shape[1]      # the flat rectangle's nodes are filtered out


def test_the_cases_are_not_degenerate():
    for name in sorted(FC.SPECS):
        s = FC.case(name).statement
        assert 0 < (s["status"] == 0).sum() < len(s["status"]) // 2
        assert len(set(s["iters"][:, 0].tolist())) > 4 and s["iters"].max() == 30                       # iteration counts differ; some track runs all 30
        assert s["pair_first"][-1] < (s["status"] == 1).sum()                                           # the filter drops a tracked point
    # the out-of-level exit (tests/test_flow_statement.py says which feature leaves where): status 0 with level 0 entered, after no update and after some
    s = FC.case("exits-96x64").statement
    assert ((s["status"] == 0) & (s["iters"][:, 0] == 0)).sum() > 20 and ((s["status"] == 0) & (s["iters"][:, 0] >= 1)).sum() >= 4
    assert ((s["status"] == 0) & (s["iters"][:, 1] >= 1) & (s["iters"][:, 1] < 30)).sum() > 20                # .. and an upper level left after some updates


def test_without_optional_outputs_the_work_space_serves():
    c = FC.case("cut-200x168")
    got = EF.flow_pyrlk(c.frames, c.width, FC.PAIRS, None, iters=False, grid_outputs=False)
    FC.assert_equal_to_statement(got, c.grid_statement, "grid without optional outputs", ("next", "status", "pair_first", "points_a", "points_b"))
    assert (got["iters"] == -7).all() and (got["grid_points"] == -7.0).all() and (got["grid_counts"] == -7).all()


def test_a_pair_alone_and_no_pairs():
    c = FC.case("cut-200x168")
    got = EF.flow_pyrlk(c.frames, c.width, [FC.PAIRS[2]], c.features)
    s, n = c.statement, FC.N_FEATURES
    assert np.array_equal(got["next"].view(np.uint32), s["next"][2 * n:].view(np.uint32)) and np.array_equal(got["status"], s["status"][2 * n:])
    assert np.array_equal(got["points_b"], s["points_b"][s["pair_first"][2]:]) and got["pair_first"].tolist() == [0, s["pair_first"][3] - s["pair_first"][2]]
    got = EF.flow_pyrlk(c.frames, c.width, np.zeros((0, 2), dtype=np.int32), c.features)
    assert got["pair_first"].tolist() == [-7]                                                           # n_pairs = 0 succeeds and writes nothing


def test_the_smallest_frame_has_one_level():
    g = np.random.default_rng(1)
    frames = g.integers(0, 256, (2, 24, 24)).astype(np.uint8)
    frames[1] = np.roll(frames[0], 1, axis=1)
    feats = [np.array([[0.0, 0.0], [23.0, 23.0], [11.5, 12.25], [23.99, 0.5]], dtype=np.float32)] * 2
    FC.assert_equal_to_statement(EF.flow_pyrlk(frames, 24, [(0, 1), (1, 0)], feats), FS.flow_pyrlk(frames, [(0, 1), (1, 0)], feats), "24 x 24")


def test_the_entry_points_check_names_the_pair_or_frame():
    c = FC.case("cut-200x168")
    run = lambda **kw: EF.flow_pyrlk(kw.pop("frames", c.frames), kw.pop("width", c.width), kw.pop("pairs", FC.PAIRS), kw.pop("features", c.features), guard=None, **kw)
    with pytest.raises(EF.Refused, match=r"pair 1: frames \(1, 3\) outside the call's 3 frames"):
        run(pairs=[(0, 1), (1, 3)])
    with pytest.raises(EF.Refused, match="pair 2: frame 2 paired with itself"):
        run(pairs=[(0, 1), (1, 2), (2, 2)])
    with pytest.raises(EF.Refused, match="frame 1: feat_first descends"):
        run(feat_first=[0, 70, 60, 210])
    with pytest.raises(EF.Refused, match="frame 0: 4097 features"):
        run(features=[np.zeros((4097, 2), dtype=np.float32)] + c.features[1:])
    with pytest.raises(EF.Refused, match="reserved slot"):
        run(reserved=1)
    with pytest.raises(EF.Refused, match="point mode 0 without features"):
        run(features=None, mode=0)
    with pytest.raises(EF.Refused, match="stride 208 under the width 209"):
        run(width=209)
    with pytest.raises(EF.Refused, match="frames of 23 x 168"):
        run(width=23)
    with pytest.raises(EF.Refused, match="negative count"):
        run(n_frames=-1)
    with pytest.raises(EF.Refused, match="4097 frames"):
        run(n_frames=4097)
    with pytest.raises(EF.Refused, match="65536 pairs"):
        run(pairs=np.zeros((65536, 2), dtype=np.int32))
    with pytest.raises(EF.Refused, match="the grid of a 24 x 8192 frame has 196608 nodes"):
        run(frames=np.zeros((2, 8192, 24), dtype=np.uint8), width=24, features=None, pairs=[(0, 1)])
