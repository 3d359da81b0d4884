"""gfw_flow_dis's kernels (gyroflow_amd/csrc/gfw_dis.hip, and the grid kernel of gfw_flow.hip) and the entry point's check and staging (gfw_dis_host.h) interpreted on
the host (tests/_emu_dis.py) against the fixed-point statement (tests/_disstmt.py): the grid points and counts, pair_first, points_a, points_b and the finest level's
dense field, bit for bit, on the three scenes of tests/_discase.py at both finest scales — with the frames, every array of the work space and every output between
inaccessible pages.  The statement's result of a configuration is computed once and shared with tests/test_gpu_dis.py."""
import numpy as np
import pytest

import _discase as DC
import _disstmt as DS
import _emu_dis as ED


@pytest.mark.parametrize("name,finest", DC.CONFIGS)
def test_interpreted_kernels_equal_the_statement_to_the_bit(name, finest):
    c = DC.case(name)
    DC.assert_equal_to_statement(ED.flow_dis(c.frames, c.width, c.pairs, finest, guard="end"), DC.statement(name, finest)[0], "%s finest %d" % (name, finest))


@pytest.mark.parametrize("name", ["exits-96x64", "cut-200x168"])
def test_with_the_first_byte_of_every_array_against_an_inaccessible_page(name):
    c = DC.case(name)
    DC.assert_equal_to_statement(ED.flow_dis(c.frames, c.width, c.pairs, 2, guard="start"), DC.statement(name, 2)[0], name + " guard start")


def test_the_cases_are_not_degenerate():
    for name in sorted(DC.SPECS):
        s, _ = DC.statement(name, 2)
        assert 10 < s["grid_counts"].min() and s["grid_counts"].max() < s["grid_points"].shape[1]       # the flat rectangle's nodes are filtered out
        assert np.abs(s["flow"]).max() > 1.0                                                            # level pixels: the pair (0, 2) moves about 6 px of level 0
        c = DC.case(name)
        L = DS.Level(DS.pyramid(c.frames[0, :, :c.width])[2], DS.pyramid(c.frames[1, :, :c.width])[2])
        assert 0 < (~L.descended).sum() < L.descended.sum()                                             # the flat rectangle's patches are never descended
    assert any(t for tr in DC.statement("exits-96x64", 2)[1] for t in tr)


def test_without_optional_outputs_the_work_space_serves():
    c = DC.case("cut-200x168")
    got = ED.flow_dis(c.frames, c.width, c.pairs, 2, grid_outputs=False, flow=False)
    DC.assert_equal_to_statement(got, DC.statement("cut-200x168", 2)[0], "without optional outputs", ("pair_first", "points_a", "points_b"))
    assert (got["flow"] == -7.0).all() and (got["grid_points"] == -7.0).all() and (got["grid_counts"] == -7).all()


def test_a_pair_alone_and_no_pairs():
    c = DC.case("cut-200x168")
    s, _ = DC.statement("cut-200x168", 2)
    got = ED.flow_dis(c.frames, c.width, [c.pairs[2]], 2)
    assert np.array_equal(got["points_b"].view(np.uint32), s["points_b"][s["pair_first"][2]:].view(np.uint32)) and np.array_equal(got["flow"][0].view(np.uint32), s["flow"][2].view(np.uint32))
    assert got["pair_first"].tolist() == [0, s["pair_first"][3] - s["pair_first"][2]]
    got = ED.flow_dis(c.frames, c.width, np.zeros((0, 2), dtype=np.int32), 2)
    assert got["pair_first"].tolist() == [-7] and (got["grid_counts"] == -7).all()                      # n_pairs = 0 succeeds and writes nothing


def test_every_rejection_names_its_reason_and_leaves_the_outputs_untouched():
    c = DC.case("cut-200x168")

    def refused(text, **kw):
        args = dict(frames=c.frames, width=c.width, pairs=c.pairs, finest=2, guard=None)
        args.update(kw)
        with pytest.raises(ED.Refused, match=text) as e:
            ED.flow_dis(args.pop("frames"), args.pop("width"), args.pop("pairs"), args.pop("finest"), **args)
        assert all((o == -7).all() for o in e.value.outputs.values())

    refused(r"pair 1: frames \(1, 3\) outside the call's 3 frames", pairs=[(0, 1), (1, 3)])
    refused(r"pair 0: frames \(-1, 1\) outside", pairs=[(-1, 1)])
    refused("pair 2: frame 2 paired with itself", pairs=[(0, 1), (1, 2), (2, 2)])
    refused("reserved slot", reserved=1)
    refused("variational_iters 5", variational_iters=5)
    refused(r"finest_scale 3 \(1 or 2\)", finest=3)
    refused(r"finest_scale 0 \(1 or 2\)", finest=0)
    refused("stride 199 under the width 200", stride=199)
    refused("negative count", n_frames=-1)
    refused("4097 frames", n_frames=4097)
    refused("65536 pairs", pairs=np.zeros((65536, 2), dtype=np.int32))
    refused("frames of 200 x 8193", frames=np.zeros((2, 8193, 200), dtype=np.uint8), pairs=[(0, 1)])
    refused("frames of 256 x 24 have the coarsest scale 1, under the finest scale 2", frames=np.zeros((2, 24, 256), dtype=np.uint8), width=256, pairs=[(0, 1)])
    refused("the grid of a 16 x 8192 frame has 131072 nodes", frames=np.zeros((2, 8192, 16), dtype=np.uint8), width=16, pairs=[(0, 1)], finest=1)


def test_the_refused_size_is_served_at_the_finest_scale_1():
    g = np.random.default_rng(2)
    base = g.integers(0, 256, (24, 260)).astype(np.uint8)
    frames = np.stack([base[:, 2:258], base[:, 0:256]])
    DC.assert_equal_to_statement(ED.flow_dis(frames, 256, [(0, 1), (1, 0)], 1), DS.flow_dis(frames, [(0, 1), (1, 0)], 1), "256 x 24 at finest scale 1")
