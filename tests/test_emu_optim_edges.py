"""The case table of tests/_optimcase.py through the sync-point choice's kernel SOURCE (gyroflow_amd/csrc/gfw_sync_optim.hip) and the entry points' host arithmetic,
interpreted on the host (tests/_emu_sync_optim.py): every case, all seven outputs — lf, mf, hf, rank, masked rank, suppressed rank, points — against the f32
statement under the table's rule (NaNs at the same indices with any sign or payload, everything else equal as uint32 / uint64 views).  The precondition of a case is
asserted on the statement before a kernel output is read (`O.reference`).

Before the pick kernel reported a lane's NaN to lane 0, three cases failed here, on `points` alone: nan_repro, nan_run_first and nan_run_inside — a NaN inside a lane's
run of two or more windows that is not the run's last element, with a larger value in front of it (the cases tests/test_optim_case_statement.py's `no_nan_reset`
variant changes)."""
import numpy as np
import pytest

import _emu_sync_optim as E
import _optimcase as O
import _syncoptimstmt as S


@pytest.mark.parametrize("name", O.NAMES)
def test_every_output_equals_the_statement(name):
    c = O.case(name)
    s = O.reference(name)
    e = E.run(c.gyro, c.rate, c.target, c.trims)
    n = S.fft_size(c.rate)
    assert list(e["shape"]) == [n, len(s["rank"]), S.as_usize(c.rate / 16.0 / 2.0 * 8.0), (len(s["rank"]) + c.target - 1) // c.target] + S.band_bins(n, c.rate)
    assert O.compare(name, e) == [], (name, c.branch)


@pytest.mark.parametrize("name", ["nan_repro", "trip_mfmax50_below", "extreme_3e38"])
def test_the_rank_entry_on_three_cases(name):
    c, s = O.case(name), O.reference(name)
    e = E.run(c.gyro, c.rate, points=False)
    assert O.compare(name, e, keys=("lf", "mf", "hf", "rank")) == [] and np.all(e["rank_nms"] == -7.0)


def test_the_exact_hits_on_the_constants_where_the_search_found_one():
    for name in O.exact_names():
        test_every_output_equals_the_statement(name)
