"""gfw_sync_rs_search's and gfw_sync_rs_costs' kernels (gyroflow_amd/csrc/gfw_sync_rs.hip) interpreted on the host (tests/_emu_rs_sync.py) over the case table of
tests/_rstablecase.py — tabulated tracks: ties, NaN samples in every position of a lane's run, exact hits, sign flips, the edges of the schedule — against the f64
statement (tests/_rssyncstmt.py, `nonfinite=True`), whose precondition is asserted first.  Every array of the work space lies against an inaccessible page: at its end
for every case of the table (the whole table runs here: 152 s measured, a 601-candidate case 3 to 4 s), at its start as well for one case of every shape (FRONT).

Comparison rule (tests/_rstablecase.differs): NaNs at the same indices with any sign or payload, everything else equal as uint64 views.  No tolerance."""
import pytest

import _emu_rs_sync as ER
import _rssynccase as RC
import _rstablecase as T

FRONT = ["nan_repro_2020", "first_zero_run_start_257", "nan_candidate0_21", "exact_hit_nan_minimum", "track_2_samples", "radius_below_step", "pair_of_2", "given_nonfinite"]


def run(c, guard=1, ranges=None):
    cam = c.cam
    args = (cam.kp, cam.clip.model, cam.clip.digital, RC.cfg_of(cam, c.cfg), c.ranges if ranges is None else ranges, c.track[0], c.track[1])
    if c.kind == "costs":
        return ER.sync_rs_costs(*args, c.cands, guard=guard)
    return ER.sync_rs_search(*args, c.initial_s, c.radius_s, guard=guard)


_ran = {}


def ran(name):
    """the interpreted kernels' result of a case with guard pages behind the arrays: computed once, shared"""
    if name not in _ran:
        T.reference(name)                                                              # the precondition, before any kernel output is read
        _ran[name] = run(T.case(name))
    return _ran[name]


@pytest.mark.parametrize("name", T.NAMES)
def test_interpreted_kernels_equal_the_statement_on_the_table(name):
    assert T.compare(name, ran(name)) == [], T.case(name).branch


@pytest.mark.parametrize("name", FRONT)
def test_with_the_guard_pages_in_front_of_the_arrays(name):
    T.reference(name)
    assert T.compare(name, run(T.case(name), guard=2)) == [], T.case(name).branch


@pytest.mark.parametrize("name,other", T.SAME)
def test_negated_samples_change_nothing(name, other):
    """the metamorphic equality on the kernels' own results: negating samples of the track leaves every output bit as it was"""
    assert T.differs(T.case(name), ran(name), ran(other)) == []


def test_the_clean_range_of_a_call_equals_its_lone_call():
    name = "nan_two_ranges"
    c = T.case(name)
    lone = run(c, ranges=c.ranges[c.lone:c.lone + 1])
    assert T.compare(name, lone, rows=slice(c.lone, c.lone + 1)) == []
    both = ran(name)
    assert T.differs(c, lone, both, rows=slice(c.lone, c.lone + 1)) == []
