"""The case table of tests/_optimcase.py on the MI355X: every case through `Backend.sync_optim_points(..., details=True)` and `Backend.sync_optim_rank`, one 64 x 32
context for the file, against the f32 statement under the table's rule — NaNs at the same indices with any sign or payload (the device's default NaN need not be the
host's), everything else equal as uint32 / uint64 views: no tolerance.  The precondition of a case is asserted on the statement before a device output is read.  A NaN,
an infinity or a subnormal in the data is ordinary input to these kernels: the tiny_* cases hold the device's fold, squares and root to IEEE arithmetic without
flush-to-zero."""
import numpy as np
import pytest

from gyroflow_amd import synchronization as SY, synthetic as SF, warp
import _optimcase as O
import _syncoptimstmt as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be():
    fr = SF.SyntheticFrame("NV12", 64, 32, seed=1)
    pl = fr.planes[0]
    b = warp.Backend(pl["params"], pl["pixel_type"], fr.model, fr.digital, warp.host_buffers(pl["src"], pl["size"], pl["dst"].copy(), pl["out_size"]))
    yield b
    b.close()


@pytest.mark.parametrize("name", O.NAMES)
def test_every_output_equals_the_statement(be, name):
    c, s = O.case(name), O.reference(name)
    pts, rank, ratio, nms = be.sync_optim_points(c.gyro, c.rate, c.target, c.trims, details=True)
    assert warp.last_backend() == "sync_optim_points"
    lf, mf, hf, rank2 = be.sync_optim_rank(c.gyro, c.rate)
    assert warp.last_backend() == "sync_optim_rank"
    assert ratio == s["ratio"]
    got = dict(points=pts, rank=rank, rank_nms=nms, lf=lf, mf=mf, hf=hf)
    assert O.compare(name, got, keys=tuple(got)) == [], (name, c.branch)
    assert S.same_bits_nan(rank2, rank)


def test_the_exact_hits_on_the_constants_where_the_search_found_one(be):
    for name in O.exact_names():
        test_every_output_equals_the_statement(be, name)


@pytest.mark.parametrize("name", O.DEVICE_OUTPUT_CASES)
def test_device_outputs_equal_the_host_outputs(be, name):
    import torch
    c, s = O.case(name), O.reference(name)
    pts, rank, ratio, nms = be.sync_optim_points(c.gyro, c.rate, c.target, c.trims, details=True)
    n_w = len(rank)
    dev = torch.device("cuda", 0)
    d_pts = torch.full((c.target + 8,), -1.0, dtype=torch.float64, device=dev)
    d_n = torch.full((1,), -1, dtype=torch.int32, device=dev)
    d_rank, d_nms = (torch.full((n_w + 8,), -1.0, dtype=torch.float32, device=dev) for _ in range(2))
    torch.cuda.synchronize()
    assert be.sync_optim_points(c.gyro, c.rate, c.target, c.trims, out_ptrs=(d_pts.data_ptr(), d_n.data_ptr(), d_rank.data_ptr(), d_nms.data_ptr())) == ratio
    be.synchronize()
    n = int(d_n.cpu()[0])
    h_pts, h_rank, h_nms = d_pts.cpu().numpy(), d_rank.cpu().numpy(), d_nms.cpu().numpy()
    assert n == len(pts) == len(s["points"]) and S.same_bits_nan(h_pts[:n], pts) and np.all(h_pts[n:] == -1.0)                     # nothing is written behind n_points
    assert S.same_bits_nan(h_rank[:n_w], rank) and S.same_bits_nan(h_nms[:n_w], nms) and np.all(h_rank[n_w:] == -1.0) and np.all(h_nms[n_w:] == -1.0)
    assert O.compare(name, dict(points=h_pts[:n], rank=h_rank[:n_w], rank_nms=h_nms[:n_w]), keys=("points", "rank", "rank_nms")) == []


def test_the_python_mirror_on_a_nan_case(be):
    c, s = O.case(O.MIRROR_CASE), O.reference(O.MIRROR_CASE)
    pts, rank, ratio = SY.OptimSync(c.rate, c.gyro).run(c.target, list(c.trims), be)
    assert warp.last_backend() == "sync_optim_points"
    assert ratio == s["ratio"] and S.same_bits_nan(pts, s["points"]) and S.same_bits_nan(rank, s["rank"]) and np.count_nonzero(np.isnan(rank)) == 1
