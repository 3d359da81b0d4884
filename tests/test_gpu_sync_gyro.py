"""gfw_sync_gyro_costs / gfw_sync_gyro_search on the MI355X: the gyro-match offset search of all ranges in one device call, against the numpy statement
(tests/_syncgyrostmt.py).  The arithmetic is f64 and a candidate's sum is the reference's sequential fold, so every comparison is bit for bit: no tolerance.
The shapes are the interpreter tier's (tests/test_emu_sync_gyro.py); one search has the default size (5 ranges x (10 000 + 200) candidates x 90 samples)."""
import ctypes as C

import numpy as np
import pytest

from gyroflow_amd import abi, synchronization as SY, synthetic as S, warp
import _syncgyrostmt as G

pytestmark = pytest.mark.gpu

INV = abi.ERR_INVALID_ARGUMENT
same_bits, make_range = G.same_bits, G.make_range
F64_MAX = G.F64_MAX


@pytest.fixture()
def be():
    fr = S.SyntheticFrame("NV12", 64, 32, seed=1)
    pl = fr.planes[0]
    b = warp.Backend(pl["params"], pl["pixel_type"], fr.model, fr.digital, warp.host_buffers(pl["src"], pl["size"], pl["dst"].copy(), pl["out_size"]))
    yield b
    b.close()


def small_ranges():
    """the shapes at which the kernel can go wrong: 1, 2, 3 and 130 estimated samples; gyro slices of 1, 2 and 3000; None entries; duplicate keys; a descending slice;
    a window that the queries leave on both sides; a coarsely sampled gyro (plateaus); a range without samples; a gyro that nothing reaches"""
    est, _, gyro, _ = make_range(40, 600, seed=3)
    dup = np.concatenate([gyro, gyro[100:300] + np.array([0.0001, 50.0, -20.0, 5.0])])
    dup_has = np.ones(len(dup), dtype=np.uint8)
    dup_has[[150, 660]] = 0
    est_has = np.ones(40, dtype=np.uint8)
    est_has[[0, 7, 8, 39]] = 0
    gyro_has = np.ones(600, dtype=np.uint8)
    gyro_has[::3] = 0
    return [make_range(130, 3000, seed=11), make_range(1, 1, seed=1), make_range(2, 2, seed=2), make_range(3, 3000, seed=3), make_range(1, 3000, seed=4),
            (est, None, dup, dup_has), (est, est_has, gyro[::-1].copy(), gyro_has), make_range(8, 301, seed=5, start_ms=180.0, gyro_from_ms=100.0, fps=50.0),
            make_range(4, 60, seed=9, rate=10.0, fps=2.5), make_range(0, 40, seed=13), make_range(10, 50, seed=10, gyro_from_ms=-90000.0),
            make_range(33, 700, seed=14, rate=200.0, offset_ms=-31.7)]


@pytest.fixture(scope="module")
def small():
    ranges = small_ranges()
    return ranges, [G.search(e, eh, g, gh, 3.0, 300.0) for e, eh, g, gh in ranges]


def check_against_statement(res, coarse, fine_costs, stated):
    for i, s in enumerate(stated):
        r = res[i]
        assert (r.found, r.n_coarse) == (s["found"], s["n_coarse"]), i
        assert same_bits(coarse[i], s["coarse_costs"]), i
        assert same_bits([r.coarse_value, r.coarse_cost, r.value, r.cost], [s["coarse_value"], s["coarse_cost"], s["value"], s["cost"]]), (i, r.value, s["value"])
        assert same_bits(fine_costs[i], s["fine_costs"]), i


def test_costs_picks_and_fine_costs_equal_the_statement(be, small):
    ranges, stated = small
    res, coarse, fine_costs = be.sync_gyro_search(ranges, 3.0, 300.0, costs=True)
    assert warp.last_backend() == "sync_gyro_search"
    check_against_statement(res, coarse, fine_costs, stated)
    assert any(np.all(s["coarse_costs"] == F64_MAX) for s in stated) and any(0 < np.sum(s["coarse_costs"] == F64_MAX) < 600 for s in stated)
    plain = be.sync_gyro_search(ranges, 3.0, 300.0)                                   # without the cost outputs
    assert [bytes(r) for r in plain] == [bytes(r) for r in res]
    for i, r in enumerate(ranges):                                                    # each range equals its own single-range call
        one = be.sync_gyro_search([r], 3.0, 300.0)
        assert bytes(one[0]) == bytes(res[i]), i


def test_caller_candidates_equal_the_searchs_own_coarse_costs(be, small):
    ranges, stated = small
    cc = G.coarse_candidates(3.0, 300.0)
    got = be.sync_gyro_costs(ranges, [cc] * len(ranges))
    assert warp.last_backend() == "sync_gyro_costs"
    for i, s in enumerate(stated):
        assert same_bits(got[i], s["coarse_costs"]), i
    counts = [1, 63, 64, 65, 255, 256, 257, 600, 0, 5, 2, 300]                       # both sides of a wave and of a workgroup; none
    cands = [np.random.RandomState(k).uniform(-200.0, 200.0, k) for k in counts]
    got = be.sync_gyro_costs(ranges, cands)
    for i, (e, eh, g, gh) in enumerate(ranges):
        assert same_bits(got[i], G.costs(cands[i], e, eh, G.Tree(g, gh))), i


def device_outputs(n, n_coarse):
    import torch
    dev = torch.device("cuda", 0)
    return (torch.zeros(n * 5, dtype=torch.float64, device=dev), torch.full((n * max(n_coarse, 1),), -1.0, dtype=torch.float64, device=dev),
            torch.full((n * 200,), -1.0, dtype=torch.float64, device=dev))


def test_host_and_device_outputs_agree(be, small):
    import torch
    ranges, _ = small
    res, coarse, fine_costs = be.sync_gyro_search(ranges, 3.0, 300.0, costs=True)
    d_res, d_coarse, d_fine = device_outputs(len(ranges), 600)
    torch.cuda.synchronize()
    assert be.sync_gyro_search(ranges, 3.0, 300.0, result_ptr=d_res.data_ptr(), coarse_ptr=d_coarse.data_ptr(), fine_ptr=d_fine.data_ptr()) is None
    assert d_res.cpu().numpy().tobytes() == b"".join(bytes(r) for r in res)
    assert same_bits(d_coarse.cpu().numpy().reshape(len(ranges), 600), coarse) and same_bits(d_fine.cpu().numpy().reshape(len(ranges), 200), fine_costs)
    cc = [G.coarse_candidates(3.0, 300.0)[: 7 + 50 * i] for i in range(len(ranges))]
    host = be.sync_gyro_costs(ranges, cc)
    d_costs = torch.full((sum(len(c) for c in cc),), -1.0, dtype=torch.float64, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    assert be.sync_gyro_costs(ranges, cc, out_ptr=d_costs.data_ptr()) is None
    assert same_bits(d_costs.cpu().numpy(), np.concatenate(host))


def test_an_asynchronous_context_takes_more_calls_than_the_ring_has_slots(be):
    """device outputs, GFW_OPT_SYNCHRONOUS 0: one call more than the staging ring has slots, other data each time, queued without waiting; each result equals its lone
    synchronous call"""
    import torch
    dev = torch.device("cuda", 0)
    calls = abi.SYNC_GYRO_RING_SLOTS + 1
    data = [[make_range(20 + 30 * k, 500 + 700 * k, seed=40 + k, offset_ms=5.0 * k - 3.0), make_range(3 + k, 90, seed=50 + k)] for k in range(calls)]
    sizes = [40.0 + 25.0 * k for k in range(calls)]
    alone = [be.sync_gyro_search(data[k], 1.0, sizes[k], costs=True) for k in range(calls)]
    outs = [device_outputs(2, int(sizes[k]) * 2) for k in range(calls)]
    torch.cuda.synchronize(dev)
    be.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    be.set_option(abi.OPT_SYNCHRONOUS, 0)
    for k in range(calls):
        d_res, d_coarse, d_fine = outs[k]
        be.sync_gyro_search(data[k], 1.0, sizes[k], result_ptr=d_res.data_ptr(), coarse_ptr=d_coarse.data_ptr(), fine_ptr=d_fine.data_ptr())
    be.synchronize()
    for k in range(calls):
        res, coarse, fine_costs = alone[k]
        d_res, d_coarse, d_fine = outs[k]
        assert d_res.cpu().numpy().tobytes() == b"".join(bytes(r) for r in res), k
        assert same_bits(d_coarse.cpu().numpy().reshape(coarse.shape), coarse) and same_bits(d_fine.cpu().numpy().reshape(2, 200), fine_costs), k
    assert len({bytes(a[0][0]) for a in alone}) == calls                             # the calls did differ


def test_one_search_of_the_default_size(be):
    """5 ranges x (10 000 coarse + 200 fine) candidates x 90 estimated samples, a 1 kHz gyro cut to the window of each range"""
    c = G.Clip(60.0, 1000.0, -271.83, seed=77, duration_s=30.0, span=[(6.0 + 4.0 * k, 7.5 + 4.0 * k) for k in range(5)])
    ins = G.range_inputs(c.estimated_gyro, c.raw_imu, c.duration_ms, c.fps, c.ranges, 0.0, 5000.0)
    ranges = [(r["est"], r["est_has"], r["gyro"], r["gyro_has"]) for r in ins]
    assert len(ranges) == 5 and all(len(r[0]) == 90 for r in ranges)
    stated = [G.search(e, eh, g, gh, 0.0, 5000.0) for e, eh, g, gh in ranges]
    res, coarse, fine_costs = be.sync_gyro_search(ranges, 0.0, 5000.0, costs=True)
    assert coarse.shape == (5, 10000)
    check_against_statement(res, coarse, fine_costs, stated)
    for r in res:
        assert abs(r.value - c.offset_ms) <= 2.0                                      # 1 ms + one period of the 1 kHz gyro


def test_an_empty_search_finds_nothing(be):
    ranges = small_ranges()[:3]
    for size in (0.0, 0.9):
        res, coarse, fine_costs = be.sync_gyro_search(ranges, 5.0, size, costs=True)
        assert [r.found for r in res] == [0, 0, 0] and [r.n_coarse for r in res] == [0, 0, 0] and coarse.shape == (3, 0)
        assert np.all(fine_costs == 0.0)
    assert be.sync_gyro_search([], 5.0, 100.0) == []                                  # no ranges: nothing is written
    assert all(len(x) == 0 for x in be.sync_gyro_costs(ranges, [[], [], []]))


def test_slices_that_start_inside_their_arrays(be, small):
    """est_first[0], gyro_first[0] and cand_first[0] above 0, host and device outputs: range r's costs are the caller's entries cand_first[r] ..; what lies in front of
    a first[0] is not read and not written"""
    import torch
    ranges = small[0][:8]
    n = len(ranges)
    cands = [np.random.RandomState(70 + k).uniform(-200.0, 200.0, k) for k in (1, 63, 64, 65, 255, 256, 257, 0)]
    plain = be.sync_gyro_costs(ranges, cands)
    ef, e, eh, gf, g, gh = warp.Backend._sync_gyro_ranges(ranges)
    cf = np.zeros(n + 1, dtype=np.int32)
    cf[1:] = np.cumsum([len(c) for c in cands])
    cand = np.concatenate(cands)
    ef, e, eh = G.lead_in(ef, e, eh, 5, 1e9)
    gf, g, gh = G.lead_in(gf, g, gh, 7, -1e9)
    cf, cand, _ = G.lead_in(cf, cand, None, 300, 12345.0)
    costs = np.full(len(cand), -7.0)
    tail = (cf.ctypes.data, cand.ctypes.data, len(cand))
    assert raw_call(be, False, ef, e, eh, len(e), gf, g, gh, len(g), n, tail + (costs.ctypes.data, 0)) == 0, be.lib.gfw_last_error()
    assert np.all(costs[:300] == -7.0) and same_bits(costs[300:], np.concatenate(plain))
    d_costs = torch.full((len(cand),), -7.0, dtype=torch.float64, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    assert raw_call(be, False, ef, e, eh, len(e), gf, g, gh, len(g), n, tail + (d_costs.data_ptr(), 1)) == 0, be.lib.gfw_last_error()
    assert same_bits(d_costs.cpu().numpy(), costs)
    res = (abi.SyncResult * n)()
    want = be.sync_gyro_search(ranges, 3.0, 300.0)
    assert raw_call(be, True, ef, e, eh, len(e), gf, g, gh, len(g), n, (C.c_double(3.0), C.c_double(300.0), C.cast(res, C.c_void_p), None, None, 0)) == 0
    assert [bytes(res[i]) for i in range(n)] == [bytes(r) for r in want]


def raw_call(be, search, ef, e, eh, n_est, gf, g, gh, n_gyro, n, tail):
    p = lambda a: None if a is None else (a if isinstance(a, int) else a.ctypes.data)
    fn = be.lib.gfw_sync_gyro_search if search else be.lib.gfw_sync_gyro_costs
    return fn(be.ctx, p(ef), p(e), p(eh), n_est, p(gf), p(g), p(gh), n_gyro, n, *tail)


def test_every_rejected_argument_names_its_range_and_leaves_the_outputs_untouched(be):
    ranges = small_ranges()[:4]
    ef, e, eh, gf, g, gh = warp.Backend._sync_gyro_ranges(ranges)
    n = len(ranges)
    res = np.full(n * 5, -3.0)
    coarse, fine = np.full(n * 200, -3.0), np.full(n * 200, -3.0)
    outs = (res.ctypes.data, coarse.ctypes.data, fine.ctypes.data, 0)

    def rejected(what, rc, *names):
        assert rc == INV, (what, rc)
        msg = be.lib.gfw_last_error().decode()
        for name in names:
            assert name in msg, (what, msg)
        assert np.all(res == -3.0) and np.all(coarse == -3.0) and np.all(fine == -3.0), what

    def search(ef_=ef, e_=e, eh_=eh, ne=len(e), gf_=gf, g_=g, gh_=gh, ng=len(g), n_=n, init=0.0, size=100.0, outs_=outs):
        return raw_call(be, True, ef_, e_, eh_, ne, gf_, g_, gh_, ng, n_, (C.c_double(init), C.c_double(size)) + tuple(outs_))

    assert search() == 0 and not np.all(res == -3.0)                                  # the arguments as they are: accepted
    res[:] = -3.0; coarse[:] = -3.0; fine[:] = -3.0
    rejected("a negative range count", search(n_=-1), "negative")
    rejected("too many ranges", search(n_=abi.SYNC_GYRO_RANGES_MAX + 1), "ranges")
    rejected("a null first array", search(ef_=None), "estimated samples")
    rejected("a null gyro first array", search(gf_=None), "gyro samples")
    rejected("samples without their array", search(e_=None), "estimated samples")
    rejected("gyro samples without their array", search(g_=None), "gyro samples")
    rejected("a null result array", search(outs_=(None, coarse.ctypes.data, fine.ctypes.data, 0)), "result")
    rejected("a negative length", search(ne=-1), "estimated samples")
    bad = ef.copy(); bad[0] = -1
    rejected("a negative first", search(ef_=bad), "range 0", "estimated samples")
    bad = ef.copy(); bad[3] = bad[2] - 1
    rejected("a descending first array", search(ef_=bad), "range 2", "estimated samples", "descends")
    bad = gf.copy(); bad[2] = bad[1] - 1
    rejected("a descending gyro first array", search(gf_=bad), "range 1", "gyro samples", "descends")
    rejected("a slice outside its array", search(ne=int(ef[3])), "range 3", "estimated samples", "outside")
    rejected("a gyro slice outside its array", search(ng=int(gf[2]) - 1), "range 1", "gyro samples", "outside")
    for what, kw in (("a NaN initial offset", dict(init=float("nan"))), ("an infinite initial offset", dict(init=float("inf"))), ("a NaN search size", dict(size=float("nan"))),
                     ("an infinite search size", dict(size=float("inf"))), ("a negative search size", dict(size=-1.0))):
        rejected(what, search(**kw), "search")
    rejected("too many candidates", search(size=1000000.5), "candidates")
    # counts over the limits: rejected before any sample is read
    big = np.array([0, abi.SYNC_GYRO_EST_MAX + 1], dtype=np.int32)
    rejected("too many estimated samples", search(ef_=big, ne=int(big[1]), gf_=gf[:2].copy(), n_=1), "range 0", "estimated samples", "at most")
    big = np.array([0, 5, 5 + abi.SYNC_GYRO_SAMPLES_MAX + 1], dtype=np.int32)
    rejected("too many gyro samples", search(gf_=big, ng=int(big[2]), ef_=ef[:3].copy(), n_=2), "range 1", "gyro samples", "at most")
    # gfw_sync_gyro_costs
    cf = np.array([0, 2, 4, 6, 8], dtype=np.int32)
    cand = np.zeros(8)
    costs = np.full(8, -3.0)

    def cost_call(cf_=cf, cand_=cand, nc=8, costs_=costs):
        p = lambda a: None if a is None else a.ctypes.data
        return raw_call(be, False, ef, e, eh, len(e), gf, g, gh, len(g), n, (p(cf_), p(cand_), nc, p(costs_), 0))

    assert cost_call() == 0 and not np.any(costs == -3.0)
    costs[:] = -3.0
    bad = cf.copy(); bad[2] = 1
    for what, kw, names in (("a descending candidate first array", dict(cf_=bad), ("range 1", "candidates", "descends")),
                            ("candidates outside their array", dict(nc=7), ("range 3", "candidates", "outside")),
                            ("candidates without their array", dict(cand_=None), ("candidates",)),
                            ("a null cost array", dict(costs_=None), ("cost",)),
                            ("a null candidate first array", dict(cf_=None), ("candidates",))):
        rc = cost_call(**kw)                                                          # (each call right before its message is read)
        assert rc == INV, what
        msg = be.lib.gfw_last_error().decode()
        assert all(nm in msg for nm in names), (what, msg)
        assert np.all(costs == -3.0), what


@pytest.mark.parametrize("i", [3, 7])
def test_the_python_mirror_end_to_end_on_planted_clips(be, i):
    """synchronization.find_offsets_essential — guards, range cut, gyro window, low-pass, one device search, the 90 % rule — within the statement test's bound, and
    equal to the statement; the fast initial offset of rs-sync from it"""
    c = G.planted(i)
    ranges = c.ranges + [(12000000, 13500000), (5, 5)]
    sp = SY.SyncParams(0.0, 5000.0)
    got = SY.find_offsets_essential(c.estimated_gyro, c.raw_imu, c.duration_ms, c.fps, ranges, sp, be)
    assert len(got) == 2
    for middle, value, cost in got:
        assert abs(value - c.offset_ms) <= 1.0 + 1000.0 / c.rate, (value, c.offset_ms)
    want = G.find_offsets(c.estimated_gyro, c.raw_imu, c.duration_ms, c.fps, ranges, 0.0, 5000.0)
    assert same_bits(np.array(got), np.array(want))
    assert SY.initial_offset_fast(c.estimated_gyro, c.raw_imu, c.duration_ms, c.fps, ranges, sp, be) == ((got[0][1] + got[1][1]) / 2.0, 3000.0)
    assert SY.initial_offset_fast(c.estimated_gyro, c.raw_imu, c.duration_ms, c.fps, [(5, 5)], sp, be) == (0.0, 5000.0)
    narrow = SY.SyncParams(0.0, abs(c.offset_ms) + 20.0)                              # the planted offset lies beyond 90 % of this range: found, and turned away
    assert SY.find_offsets_essential(c.estimated_gyro, c.raw_imu, c.duration_ms, c.fps, c.ranges, narrow, be) == []
