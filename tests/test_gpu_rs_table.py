"""gfw_sync_rs_search / gfw_sync_rs_costs on the MI355X over the case table of tests/_rstablecase.py — tabulated tracks: ties inside and across the lanes' runs of the
pick kernel, NaN samples in every position of a run, NaN points, non-finite candidates, exact hits, sign flips, short and irregular tracks, the edges of the round
schedule — against the f64 statement (tests/_rssyncstmt.py, `nonfinite=True`), whose precondition is asserted before any device output is read.  One context serves
the module.  NaN is data here: every call is an ordinary call on valid buffers.

Comparison rule (tests/_rstablecase.differs): NaNs at the same indices with any sign or payload, everything else equal as uint64 views.  No tolerance."""
import numpy as np
import pytest

from gyroflow_amd import warp
import _rssynccase as RC
import _rssyncstmt as RS
import _rstablecase as T
from test_gpu_rs_sync import backend_for, device_outputs, rows_of_tensor

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    b = backend_for(T.camera())
    yield b
    b.close()


def run(be, c, ranges=None):
    args = (c.cam.kp, RC.cfg_of(c.cam, c.cfg), c.ranges if ranges is None else ranges, c.track[0], c.track[1])
    if c.kind == "costs":
        return be.sync_rs_costs(*args, c.cands)
    res, cand, cost = be.sync_rs_search(*args, c.initial_s, c.radius_s, rounds=True)
    return RC.rows_of(res), cand, cost


_ran = {}


def ran(be, name):
    """the device's result of a case: computed once, shared"""
    if name not in _ran:
        T.reference(name)                                                              # the precondition, before any device output is read
        _ran[name] = run(be, T.case(name))
    return _ran[name]


@pytest.mark.parametrize("name", T.NAMES)
def test_the_device_equals_the_statement_on_the_table(be, name):
    got = ran(be, name)
    assert warp.last_backend() in ("sync_rs_search", "sync_rs_costs")
    assert T.compare(name, got) == [], T.case(name).branch


@pytest.mark.parametrize("name,other", T.SAME)
def test_negated_samples_change_nothing(be, name, other):
    """the metamorphic equality on the device's own results: negating samples of the track leaves every output bit as it was"""
    assert T.differs(T.case(name), ran(be, name), ran(be, other)) == []


def test_the_clean_range_of_a_call_equals_its_lone_call(be):
    name = "nan_two_ranges"
    c = T.case(name)
    lone = run(be, c, ranges=c.ranges[c.lone:c.lone + 1])
    assert T.compare(name, lone, rows=slice(c.lone, c.lone + 1)) == []
    assert T.differs(c, lone, ran(be, name), rows=slice(c.lone, c.lone + 1)) == []


@pytest.mark.parametrize("name", T.DEVICE_OUTPUT_CASES)
def test_device_outputs_of_a_nan_case_and_a_tie_case(be, name):
    import torch
    c = T.case(name)
    T.reference(name)
    outs = device_outputs(len(c.ranges), RS.candidates_total(c.cfg, c.radius_s))
    torch.cuda.synchronize()
    assert be.sync_rs_search(c.cam.kp, RC.cfg_of(c.cam, c.cfg), c.ranges, c.track[0], c.track[1], c.initial_s, c.radius_s, out_ptrs=tuple(o.data_ptr() for o in outs)) is None
    be.synchronize()
    assert T.compare(name, (rows_of_tensor(outs[0]), outs[1].cpu().numpy(), outs[2].cpu().numpy())) == []


def test_device_output_of_the_given_candidates(be):
    import torch
    name = "given_nonfinite"
    c = T.case(name)
    T.reference(name)
    costs = torch.full((len(c.cands[0]),), -7.0, dtype=torch.float64, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    assert be.sync_rs_costs(c.cam.kp, RC.cfg_of(c.cam, c.cfg), c.ranges, c.track[0], c.track[1], c.cands, out_ptr=costs.data_ptr()) is None
    be.synchronize()
    assert T.compare(name, [costs.cpu().numpy()]) == []
