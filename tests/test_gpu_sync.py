"""gfw_sync_visual_costs / gfw_sync_visual_search on the MI355X: the visual-features offset and readout-time search of a range in one device call, against the host
statement (tests/_syncstmt.py) over the planted ranges of tests/_synccase.py ("gpu" shape: 6 pairs of 1, 10, 63, 64, 65 and 200 points; 40 + 200 candidates a search).

(a) a cost equals the statement's fold over the call's OWN mapped points to the bit: integer arithmetic, no tolerance.
(b) the mapped points match the statement's within twice the per-clip point figure of tests/golden/sync_rotation_sensitivity.json (the device's f64 acos / sin
    are the device library's: an f32 rotation entry can differ in its last bits; the fixture displaces every entry by -2 .. +2 ULP).
(c) the statement's cost AT the candidate a stage returns is at most the statement's minimum over that stage's candidates plus twice the fixture's cost figure."""
import ctypes as C

import numpy as np
import pytest

from gyroflow_amd import abi, synthetic as S, warp
import _pairbase as PB
import _synccase as SC
import _syncstmt as SS

pytestmark = pytest.mark.gpu

SENS = SC.sensitivity()
INV = abi.ERR_INVALID_ARGUMENT


def backend_for(clip, tracks=True):
    fr = S.SyntheticFrame("NV12", clip.size[0], clip.size[1], seed=3, lens=clip.lens, pixels=True)
    pl = fr.planes[0]
    b = warp.host_buffers(pl["src"], pl["size"], pl["dst"].copy(), pl["out_size"])
    be = warp.Backend(pl["params"], pl["pixel_type"], fr.model, fr.digital, b)
    if tracks:
        be.set_quaternion_tracks(*clip.tracks)
    return be


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def sample_candidates(name, mode):
    """eight candidates of the case: both ends of the coarse stage, the statement's coarse pick and its neighbour, four fine ones"""
    st = SC.stored(name, "gpu", mode)
    coarse = SC.stage_candidates(name, "gpu", mode)
    cp = st["coarse_pick"]
    fine = SC.stage_candidates(name, "gpu", mode, coarse[cp][0 if mode == 0 else 1])
    return [coarse[0], coarse[-1], coarse[cp], coarse[max(cp - 1, 0)], fine[0], fine[st["fine_pick"]], fine[137], fine[-1]]


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", sorted(SC.CLIPS))
def test_costs_fold_their_own_mapped_points_and_the_points_match_the_statement(name, mode):
    rng, _ = SC.planted(name, "gpu", mode)
    clip = rng.clip
    cands = sample_candidates(name, mode)
    be = backend_for(clip)
    try:
        costs, mapped = be.sync_visual_costs(rng.kp, SC.sync_search(clip), rng.pairs, cands, mapped=True)
        assert warp.last_backend() == "sync_visual_costs"
        assert same_bits(be.sync_visual_costs(rng.kp, SC.sync_search(clip), rng.pairs, cands), costs)                  # without the mapped output
    finally:
        be.close()
    assert mapped.shape == (len(cands), rng.total, 2, 2)
    worst = 0.0
    for i, (offs, readout) in enumerate(cands):
        assert costs[i] == SS.fold_mapped(rng, mapped[i]), (name, mode, i, costs[i])                                   # (a)
        ref = SS.mapped_points(rng, offs, readout)
        worst = max(worst, float(np.max(np.abs(mapped[i] - ref))))
    bar = 2.0 * SENS[name]["point_max_abs_px"]
    print("%s mode %d: mapped points differ from the statement's by at most %.3g px (bar %.3g)" % (name, mode, worst, bar))
    assert worst <= bar, (name, mode, worst, bar)                                                                      # (b)


def check_pick(name, mode, res, coarse_costs, fine_costs):
    """(c) for both stages; -> the figures"""
    st = SC.stored(name, "gpu", mode)
    col = 0 if mode == 0 else 1
    bar = 2.0 * SENS[name]["cost_max_abs"]
    coarse = SC.stage_candidates(name, "gpu", mode)
    assert res.found == 1 and res.n_coarse == len(coarse) == len(coarse_costs)
    ci = [c[col] for c in coarse].index(res.coarse_value)                         # the candidates are made by one formula on both sides: equal to the bit
    assert res.coarse_cost == coarse_costs[ci] and ci == SS.find_min(list(coarse_costs))                              # the device's own costs: its pick is their last minimum
    over_c = st["coarse_costs"][ci] - min(st["coarse_costs"])
    fine = SC.stage_candidates(name, "gpu", mode, res.coarse_value)
    fi = [c[col] for c in fine].index(res.value)
    assert res.cost == fine_costs[fi] and fi == SS.find_min(list(fine_costs))
    if ci == st["coarse_pick"]:
        ref_fine = st["fine_costs"]
    else:                                                                         # another coarse pick within the bar: the statement's costs of ITS fine stage
        rng, _ = SC.planted(name, "gpu", mode)
        ref_fine = [SS.cost(rng, o, r) for o, r in fine]
    over_f = ref_fine[fi] - min(ref_fine)
    print("%s mode %d: coarse pick %g (statement %g), statement cost there %g over its minimum; fine pick %.2f (statement %.2f), %g over (bar %g); truth %g"
          % (name, mode, res.coarse_value, coarse[st["coarse_pick"]][col], over_c, res.value, st["value"], over_f, bar, SC.truth(name, mode)))
    assert over_c <= bar, (name, mode, over_c, bar)
    assert over_f <= bar, (name, mode, over_f, bar)


def search_call(be, rng, name, mode, **kw):
    a = SC.search_args(name, "gpu", mode)
    return be.sync_visual_search(rng.kp, SC.sync_search(rng.clip), rng.pairs, mode, a.get("initial_offset", 0.0), a.get("search_size", 0.0), a.get("readout", 0.0),
                                 a.get("fps", 30.0), **kw)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", sorted(SC.CLIPS))
def test_search_returns_a_minimum_of_the_statement(name, mode):
    """host outputs, synchronous context; then device outputs on a synchronous and an asynchronous context, two calls queued back to back: the same bits"""
    import torch
    dev = torch.device("cuda", 0)
    rng, _ = SC.planted(name, "gpu", mode)
    be = backend_for(rng.clip)
    try:
        res, coarse, fine = search_call(be, rng, name, mode, costs=True)
        assert warp.last_backend() == "sync_visual_search"
        check_pick(name, mode, res, coarse, fine)
        plain = search_call(be, rng, name, mode)
        assert bytes(plain) == bytes(res)
        d_res = torch.zeros(5, dtype=torch.float64, device=dev)                   # gfw_sync_result: two int32, four f64
        d_coarse = torch.full((len(coarse),), -1.0, dtype=torch.float64, device=dev)
        d_fine = torch.full((200,), -1.0, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        assert search_call(be, rng, name, mode, result_ptr=d_res.data_ptr(), coarse_ptr=d_coarse.data_ptr(), fine_ptr=d_fine.data_ptr()) is None
        assert d_res.cpu().numpy().tobytes() == bytes(res) and same_bits(d_coarse.cpu().numpy(), coarse) and same_bits(d_fine.cpu().numpy(), fine)
        d_res.zero_(); d_coarse.fill_(-1.0); d_fine.fill_(-1.0)
        d_res2 = torch.zeros(5, dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)
        be.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        be.set_option(abi.OPT_SYNCHRONOUS, 0)
        search_call(be, rng, name, mode, result_ptr=d_res.data_ptr(), coarse_ptr=d_coarse.data_ptr(), fine_ptr=d_fine.data_ptr())      # asynchronous: in order on the stream
        search_call(be, rng, name, mode, result_ptr=d_res2.data_ptr())                                                                  # ... and a second call behind it
        be.synchronize()
        assert d_res.cpu().numpy().tobytes() == bytes(res) and d_res2.cpu().numpy().tobytes() == bytes(res)
        assert same_bits(d_coarse.cpu().numpy(), coarse) and same_bits(d_fine.cpu().numpy(), fine)
        assert bytes(search_call(be, rng, name, mode)) == bytes(res)                                                                    # asynchronous context, host output
    finally:
        be.close()


def random_pairs(sizes, seed, size=(320, 180)):
    g = np.random.default_rng(seed)
    pairs = []
    for k, n in enumerate(sizes):
        p = np.stack([g.uniform(0.0, size[0], n), g.uniform(0.0, size[1], n)], 1).astype(np.float32)
        q = (p + g.normal(0.0, 2.5, (n, 2))).astype(np.float32)
        pairs.append((1300000 + 400000 * k, 1366667 + 400000 * k, p, q))
    return pairs


def test_the_largest_pair_and_one_point_more():
    """4096 points fill the 16 KB of LDS a workgroup may ask for; 4097 are rejected, with the pair named"""
    clip = SC.CLIPS["fisheye-r12"]
    rng = SS.Range(clip, random_pairs([3, 4096, 0, 130], 77))
    cands = [(2.5, 12.0), (0.0, 0.0), (-3.0, -7.5)]
    be = backend_for(clip)
    try:
        costs, mapped = be.sync_visual_costs(rng.kp, SC.sync_search(clip), rng.pairs, cands, mapped=True)
        for i in range(len(cands)):
            assert costs[i] == SS.fold_mapped(rng, mapped[i]) and costs[i] > 0.0, (i, costs[i])
        ref = SS.mapped_points(rng, *cands[1])
        assert float(np.max(np.abs(mapped[1] - ref))) <= 2.0 * SENS["fisheye-r12"]["point_max_abs_px"]
        with pytest.raises(warp.GfwError) as e:
            be.sync_visual_costs(rng.kp, SC.sync_search(clip), random_pairs([3, 4097], 78), cands)
        assert e.value.code == INV and "pair 1" in str(e.value) and "4097" in str(e.value)
    finally:
        be.close()


def test_sync_offsets_are_kept_or_cleared():
    """use_sync_offsets 1 reads the context's offsets (for_rs), 0 clears them (visual_features.rs:13-15): 0 on a context WITH offsets equals a context without, to the bit"""
    clip = SS.PlantedClip("with-offsets", readout=12.0, track_scale=14.0)
    clip.sync_offsets, clip.duration_ms = (np.array([900000, 2500000, 4300000], dtype=np.int64), np.array([2.0, -1.5, 3.25])), 5000.0
    pairs = SC.planted("fisheye-r12", "gpu", 0)[0].pairs
    cands = [(7.0, 12.0), (7.3, 0.0), (-2.0, -5.0)]
    out = {}
    for key, offsets, use in (("with-1", True, 1), ("with-0", True, 0), ("without-0", False, 0)):
        be = backend_for(clip)
        try:
            be.set_sync_offsets(clip.duration_ms, *(clip.sync_offsets if offsets else ((), ())))
            out[key] = be.sync_visual_costs(SS.Range(clip, pairs).kp, SC.sync_search(clip, use), pairs, cands, mapped=True)
        finally:
            be.close()
    assert same_bits(out["with-0"][0], out["without-0"][0]) and same_bits(out["with-0"][1], out["without-0"][1])
    assert not np.array_equal(out["with-1"][0], out["with-0"][0]) and not np.array_equal(out["with-1"][1], out["with-0"][1])
    kept = SS.Range(clip, pairs, use_sync_offsets=True)
    for i, (offs, readout) in enumerate(cands):
        assert out["with-1"][0][i] == SS.fold_mapped(kept, out["with-1"][1][i])
        assert float(np.max(np.abs(out["with-1"][1][i] - SS.mapped_points(kept, offs, readout)))) <= 2.0 * SENS["fisheye-r12"]["point_max_abs_px"]


def test_empty_inputs_succeed():
    rng, _ = SC.planted("fisheye-r0", "gpu", 0)
    clip, search = rng.clip, SC.sync_search(rng.clip)
    be = backend_for(clip)
    try:
        assert np.array_equal(be.sync_visual_costs(rng.kp, search, [], [(0.0, 0.0), (1.0, 5.0)]), [0.0, 0.0])         # n_pairs = 0: every cost is 0
        assert be.sync_visual_costs(rng.kp, search, rng.pairs, np.zeros((0, 2))).shape == (0,)                         # n_candidates = 0
        empty = (1000000, 1066667, np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32))
        with_empty = [rng.pairs[3], empty, rng.pairs[5]]
        assert same_bits(be.sync_visual_costs(rng.kp, search, with_empty, [(7.0, 0.0)]),
                         be.sync_visual_costs(rng.kp, search, [rng.pairs[3], rng.pairs[5]], [(7.0, 0.0)]))            # a pair with 0 points contributes 0
        res, coarse, fine = be.sync_visual_search(rng.kp, search, rng.pairs, 0, 0.0, 0.9, 0.0, costs=True)            # `0.9 as usize` = 0 candidates
        assert res.found == 0 and res.n_coarse == 0 and len(coarse) == 0 and np.all(fine == 0.0)
        assert be.sync_visual_search(rng.kp, search, rng.pairs, 1, scaled_fps=2000.0).found == 0                       # (1000 / 2000) as isize = 0
        res, coarse, fine = be.sync_visual_search(rng.kp, search, [], 0, 0.0, 5.0, 0.0, costs=True)                   # no pairs: every cost 0, the last candidate wins twice
        assert res.found == 1 and np.all(coarse == 0.0) and np.all(fine == 0.0) and res.coarse_value == 1.5 and res.value == 1.5 - 1.0 + 199 * 0.01 and res.cost == 0.0
    finally:
        be.close()


def test_arguments():
    rng, _ = SC.planted("fisheye-r0", "gpu", 0)
    clip, kp, search = rng.clip, rng.kp, SC.sync_search(rng.clip)
    ts, first, pa, pb = warp.Backend._sync_pairs(rng.pairs)
    cand = np.array([[7.0, 0.0], [8.0, 0.0]])
    out = np.full(2, -7.0)
    res = abi.SyncResult(found=-7)
    be = backend_for(clip)
    lib = be.lib
    try:
        def costs(ctx=be.ctx, kp=kp, search=search, ts=ts.ctypes.data, first=first, pa=pa.ctypes.data, n_pairs=len(rng.pairs), cand=cand.ctypes.data, n=2, out=out.ctypes.data):
            return lib.gfw_sync_visual_costs(ctx, C.byref(kp) if kp is not None else None, C.byref(search) if search is not None else None, ts,
                                             first.ctypes.data if first is not None else None, pa, pb.ctypes.data, n_pairs, cand, n, out, None, 0)

        def find(search=search, mode=0, size=5.0, fps=30.0, result=C.cast(C.byref(res), C.c_void_p)):
            return lib.gfw_sync_visual_search(be.ctx, C.byref(kp), C.byref(search), ts.ctypes.data, first.ctypes.data, pa.ctypes.data, pb.ctypes.data, len(rng.pairs),
                                              mode, 0.0, size, 0.0, fps, result, None, None, 0)

        def rejected(rc, *words):
            msg = lib.gfw_last_error()
            assert rc == INV and all(w in msg for w in words), (rc, msg, words)

        rejected(costs(ctx=None)); rejected(costs(kp=None)); rejected(costs(search=None))
        rejected(costs(n_pairs=-1), b"negative"); rejected(costs(n=-1), b"negative")
        rejected(costs(ts=None), b"pair_ts_us"); rejected(costs(first=None), b"pair_first"); rejected(costs(pa=None), b"points_a")
        rejected(costs(cand=None), b"candidates"); rejected(costs(out=None), b"costs")
        bad = first.copy(); bad[3] = bad[2] - 1
        rejected(costs(first=bad), b"pair 2", b"descends")
        bad = first.copy(); bad[0] = -1
        rejected(costs(first=bad), b"pair 0", b"negative")
        bad = first.copy(); bad[5:] += 5000
        rejected(costs(first=bad), b"pair 4", b"4096")
        for field, value, word in (("width", 0, b"0 x 180"), ("height", -3, b"320 x -3"), ("horizontal_readout", 2, b"horizontal_readout 2"), ("use_sync_offsets", 2, b"use_sync_offsets 2"),
                                   ("width", 65536, b"2^32"), ("height", 65536, b"2^32")):
            s2 = abi.SyncSearch.from_buffer_copy(search)
            setattr(s2, field, value)
            rejected(costs(search=s2), word)
        s2 = abi.SyncSearch.from_buffer_copy(search)
        s2.width, s2.height = 46341, 46341                                        # 2 * 46341^2 = 2^32 + 9266: the first square over; 46340 x 46341 passes this check
        rejected(costs(search=s2), b"2^32")
        for slot in (0, 1):
            s2 = abi.SyncSearch.from_buffer_copy(search)
            s2.reserved[slot] = 1
            rejected(costs(search=s2), b"reserved")
        for flag in (abi.FLAG_HAS_IBIS_DATA, abi.FLAG_HAS_MESH_DATA, abi.FLAG_HAS_FPD_DATA):
            k2 = kp.copy()
            k2.flags |= flag
            rejected(costs(kp=k2), b"does not cover")
        rejected(find(mode=2), b"mode 2"); rejected(find(mode=-1), b"mode"); rejected(find(result=None), b"result")
        rejected(find(size=2.0e6), b"candidates"); rejected(find(mode=1, fps=0.0), b"candidates")
        bare = backend_for(clip, tracks=False)
        try:
            assert lib.gfw_sync_visual_costs(bare.ctx, C.byref(kp), C.byref(search), ts.ctypes.data, first.ctypes.data, pa.ctypes.data, pb.ctypes.data, len(rng.pairs),
                                             cand.ctypes.data, 2, out.ctypes.data, None, 0) == INV and b"tracks" in lib.gfw_last_error()
        finally:
            bare.close()
        assert np.all(out == -7.0) and res.found == -7                            # outputs untouched by every rejection
        assert costs() == 0 and np.all(out >= 0.0) and find() == 0 and res.found == 1 and res.n_coarse == 5
    finally:
        be.close()


def test_a_pair_set_that_starts_behind_unused_points_gives_the_same_bits():
    """pair_first[0] = 3: the firsts are staged as given and the points from the arrays' start (tests/_pairbase.py)"""
    rng, cands = PB.visual()
    be = backend_for(rng.clip)
    costs = PB.assert_base_does_not_matter(lambda: be.sync_visual_costs(rng.kp, SC.sync_search(rng.clip), rng.pairs, cands), "sync_visual_costs")
    be.close()
    assert len(costs) == 3 and len(set(costs.tolist())) == 3 and costs[1] == min(costs)
