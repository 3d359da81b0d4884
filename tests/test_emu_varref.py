"""gfw_flow_dis_refined's kernels (gyroflow_amd/csrc/gfw_varref.hip behind gfw_dis.hip and the grid kernel of gfw_flow.hip) and the entry point's check and plan
(gfw_varref_host.h) interpreted on the host (tests/_emu_varref.py) against the statement (tests/_varrefstmt.py): pair_first, the points and the finest level's dense
field, bit for bit, on the three scenes of tests/_discase.py at both finest scales — with the frames, every array of both work spaces and every output between
inaccessible pages.  The statement's result of a configuration is computed once and shared with tests/test_gpu_varref.py."""
import numpy as np
import pytest

import _discase as DC
import _disstmt as DS
import _emu_varref as EV
import _varrefcase as VC
import _varrefstmt as VS


@pytest.mark.parametrize("name,finest", DC.CONFIGS)
def test_interpreted_kernels_equal_the_statement_to_the_bit(name, finest):
    c = DC.case(name)
    got = EV.flow_dis_refined(c.frames, c.width, c.pairs, finest, guard="end")
    DC.assert_equal_to_statement(got, VC.statement(name, finest), "%s finest %d" % (name, finest))
    # the launches of the header's formula: the pyramid levels, the grid, per level three passes, the dense field and 2 + F (1 + 2 S), the scan, the nodes
    coarsest = DS.coarsest_scale(c.width, c.frames.shape[1])
    assert got["launches"] == 3 + coarsest + (4 + 2 + 5 * (1 + 2 * 5)) * (coarsest - finest + 1)


def test_with_the_first_byte_of_every_array_against_an_inaccessible_page():
    c = DC.case("exits-96x64")
    DC.assert_equal_to_statement(EV.flow_dis_refined(c.frames, c.width, c.pairs, 2, guard="start"), VC.statement("exits-96x64", 2), "guard start")


def test_another_configuration():
    c = DC.case("cut-200x168")
    got = EV.flow_dis_refined(c.frames, c.width, c.pairs, 2, VC.OTHER)
    DC.assert_equal_to_statement(got, VC.statement("cut-200x168", 2, VC.OTHER), "2 fixed-point and 3 SOR iterations")
    assert got["launches"] == 3 + 3 + (4 + 2 + 2 * (1 + 2 * 3)) * 2


def test_no_fixed_point_iteration_is_the_unrefined_call_to_the_bit():
    c = DC.case("cut-200x168")
    got = EV.flow_dis_refined(c.frames, c.width, c.pairs, 2, VS.DEFAULT._replace(fixed_point_iters=0))
    plain = EV.flow_dis_refined(c.frames, c.width, c.pairs, 2, unrefined_call=True)
    assert got.pop("launches") == 3 + 3 + 4 * 2 and plain.pop("launches") == 0             # no refinement launch
    for k in plain:
        assert np.array_equal(got[k].view(np.uint32), plain[k].view(np.uint32)), k
    DC.assert_equal_to_statement(got, DC.statement("cut-200x168", 2)[0], "fixed_point_iters = 0")


def test_a_pair_alone_is_its_slice_of_the_three_pair_call():
    c = DC.case("cut-200x168")
    s = VC.statement("cut-200x168", 2)
    got = EV.flow_dis_refined(c.frames, c.width, [c.pairs[2]], 2)
    assert np.array_equal(got["points_b"].view(np.uint32), s["points_b"][s["pair_first"][2]:].view(np.uint32)) and np.array_equal(got["flow"][0].view(np.uint32), s["flow"][2].view(np.uint32))
    assert got["pair_first"].tolist() == [0, s["pair_first"][3] - s["pair_first"][2]]
    got = EV.flow_dis_refined(c.frames, c.width, np.zeros((0, 2), dtype=np.int32), 2)
    assert got["pair_first"].tolist() == [-7] and got["launches"] == 0                                  # n_pairs = 0 succeeds and writes nothing


def test_every_rejection_names_its_reason_and_leaves_the_outputs_untouched():
    c = DC.case("cut-200x168")

    def refused(text, cfg=VS.DEFAULT, **kw):
        args = dict(pairs=c.pairs, finest=2, guard=None)
        args.update(kw)
        with pytest.raises(EV.Refused, match=text) as e:
            EV.flow_dis_refined(c.frames, c.width, args.pop("pairs"), args.pop("finest"), cfg, **args)
        assert all((o == -7).all() for o in e.value.outputs.values())

    r = VS.DEFAULT._replace
    refused("variational_iters 5 in gfw_flow_dis_cfg beside fixed_point_iters 5 in gfw_flow_varref_cfg", variational_iters=5)
    refused("variational_iters 3 in gfw_flow_dis_cfg beside fixed_point_iters 0", r(fixed_point_iters=0), variational_iters=3)
    refused(r"fixed_point_iters -1 \(0 to 64\)", r(fixed_point_iters=-1))
    refused(r"fixed_point_iters 65 \(0 to 64\)", r(fixed_point_iters=65))
    refused(r"sor_iters 0 \(1 to 64\)", r(sor_iters=0))
    refused(r"sor_iters 65 \(1 to 64\)", r(sor_iters=65))
    for name in ("alpha", "delta", "gamma"):
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            refused("%s .* \\(finite and above 0\\)" % name, r(**{name: bad}))
    for bad in (0.0, 2.0, -0.5, float("nan"), float("inf")):
        refused(r"omega .* \(between 0 and 2, both excluded\)", r(omega=bad))
    refused("refinement configuration: the reserved slots", ref_reserved=(0, 1))
    refused("refinement configuration: the reserved slots", ref_reserved=(1, 0))
    # what gfw_flow_dis refuses is refused here with its words
    refused("DIS flow configuration: the reserved slot", reserved=1)
    refused(r"finest_scale 3 \(1 or 2\)", finest=3)
    refused(r"pair 1: frames \(1, 3\) outside the call's 3 frames", pairs=[(0, 1), (1, 3)])
    refused("pair 2: frame 2 paired with itself", pairs=[(0, 1), (1, 2), (2, 2)])
