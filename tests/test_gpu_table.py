"""The case table of tests/_tablecase.py on the MI355X, through gfw_sync_visual_costs, gfw_sync_visual_search, gfw_zoom_fovs and gfw_sync_gyro_costs: an identity
lens and plateau tracks make the points handed in the mapped points, so the sync fold (ballot / mbcnt compaction, the bisection over ballot counts, the u64 LDS
add, the dynamic LDS size), the two-level reduce and the zoom rounds run on inputs chosen for their edges.  Every comparison is bit for bit (NaN as NaN), against
the statements and between host and device outputs; every case's precondition is asserted on the statement first.  One 64 x 32 context per lens model; no
specialised builds."""
import numpy as np
import pytest

from gyroflow_amd import abi, synthetic as S, warp
import _syncgyrostmt as G
import _tablecase as T

pytestmark = pytest.mark.gpu

COSTS = {c.name: c for c in T.sync_cost_cases()}
SEARCHES = {c.name: c for c in T.search_cases()}
GROUPS = {g.name: g for g in T.zoom_groups()}
_CTX = {}


@pytest.fixture(scope="module")
def contexts():
    """model name -> a 64 x 32 context of that lens model (the searches' own sizes travel in SyncSearch / ZoomSearch)"""
    def get(clip):
        name = clip.lens["model"]
        if name not in _CTX:
            fr = S.SyntheticFrame("NV12", 64, 32, seed=1, lens=clip.lens)
            pl = fr.planes[0]
            _CTX[name] = warp.Backend(pl["params"], pl["pixel_type"], fr.model, fr.digital, warp.host_buffers(pl["src"], pl["size"], pl["dst"].copy(), pl["out_size"]))
        return _CTX[name]
    yield get
    for be in _CTX.values():
        be.close()
    _CTX.clear()


def device(shape, dtype):
    import torch
    t = torch.full(shape, -1.0, dtype=dtype, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    return t


@pytest.mark.parametrize("name", list(COSTS))
def test_costs_fold_the_table(name, contexts):
    import torch
    case = COSTS[name]
    want = T.precondition_sync(case)
    be = contexts(case.clip)
    be.set_quaternion_tracks(*case.clip.tracks)
    kp, search, n = case.range.kp, case.search(), len(case.candidates)
    costs, mapped = be.sync_visual_costs(kp, search, case.pairs, case.candidates, mapped=True)
    assert warp.last_backend() == "sync_visual_costs"
    for c in range(n):
        assert T.same_bits(mapped[c], case.expected[c]), (name, c)
        assert costs[c] == want[c], (name, c, costs[c], want[c])
    assert T.same_bits(be.sync_visual_costs(kp, search, case.pairs, case.candidates), costs)                           # without the mapped output
    d_costs, d_mapped = device((n,), torch.float64), device((n, max(case.range.total, 1), 2, 2), torch.float32)
    assert be.sync_visual_costs(kp, search, case.pairs, case.candidates, out_ptr=d_costs.data_ptr(), mapped_ptr=d_mapped.data_ptr()) is None
    assert T.same_bits(d_costs.cpu().numpy(), costs)
    if case.range.total:
        assert T.same_bits(d_mapped.cpu().numpy(), mapped)


@pytest.mark.parametrize("name", list(SEARCHES))
def test_search_picks_the_last_of_equal_minima(name, contexts):
    import torch
    case = SEARCHES[name]
    st = T.precondition_search(case)
    be = contexts(case.clip)
    be.set_quaternion_tracks(*case.clip.tracks)
    a = case.args
    args = (case.range.kp, case.search(), case.pairs, case.mode, a["initial_offset"], a["search_size"], a["readout"], a["fps"])
    res, coarse, fine_costs = be.sync_visual_search(*args, costs=True)
    assert warp.last_backend() == "sync_visual_search"
    T.check_search(case, res, coarse, fine_costs)                      # (the entry point has no output for the fine candidates: `value` is the one picked)
    assert bytes(be.sync_visual_search(*args)) == bytes(res)
    d_res, d_coarse, d_fine = device((5,), torch.float64), device((len(coarse),), torch.float64), device((200,), torch.float64)
    assert be.sync_visual_search(*args, result_ptr=d_res.data_ptr(), coarse_ptr=d_coarse.data_ptr(), fine_ptr=d_fine.data_ptr()) is None
    assert d_res.cpu().numpy().tobytes() == bytes(res) and T.same_bits(d_coarse.cpu().numpy(), coarse) and T.same_bits(d_fine.cpu().numpy(), fine_costs)
    # the fine candidates, through the cost entry: the statement's 200 cost what the search's fine stage cost
    assert T.same_bits(be.sync_visual_costs(case.range.kp, case.search(), case.pairs, st["fine"]), fine_costs)


@pytest.mark.parametrize("name", list(GROUPS))
def test_zoom_rounds(name, contexts):
    """one call in shuffled order (the 16:9 group: 76 frames), then every frame alone: the statement's bits both times, on host and device outputs"""
    import torch
    group = GROUPS[name]
    st = T.precondition_zoom(group)
    be = contexts(group.clip)
    n = len(group.frames)
    order = T.shuffled(n)
    kp, search, frames, rot = group.inputs(order)
    fov, dbg = be.zoom_fovs(kp, search, frames, rotations=rot, debug=True)
    assert warp.last_backend() == "zoom_fovs"
    assert T.same_bits(fov, st["fov"][order]), (name, [group.frames[k]["name"] for j, k in enumerate(order) if not T.same_bits(fov[j:j + 1], st["fov"][k:k + 1])])
    assert T.same_bits(dbg, st["debug"][order]), name
    d_fov, d_dbg = device((n,), torch.float64), device((n, 120, 2), torch.float64)
    assert be.zoom_fovs(kp, search, frames, rotations=rot, out_ptr=d_fov.data_ptr(), debug_ptr=d_dbg.data_ptr()) is None
    assert T.same_bits(d_fov.cpu().numpy(), fov) and T.same_bits(d_dbg.cpu().numpy(), dbg)
    for k in range(n):
        kp, search, one, rot = group.inputs([k])
        f1, d1 = be.zoom_fovs(kp, search, one, rotations=rot, debug=True)
        assert T.same_bits(f1, st["fov"][k:k + 1]) and T.same_bits(d1, st["debug"][k:k + 1]), (name, group.frames[k]["name"])


def test_the_zoom_table_as_a_whole():
    T.precondition_zoom_table(list(GROUPS.values()))


def test_gyro_costs_of_queries_that_are_no_key(contexts):
    import torch
    ranges, cands = T.gyro_nonfinite_case()
    be = contexts(T.TableClip("gyro"))
    got = be.sync_gyro_costs(ranges, cands)
    assert warp.last_backend() == "sync_gyro_costs"
    for i, (e, eh, g, gh) in enumerate(ranges):
        assert G.same_bits(got[i], G.costs(cands[i], e, eh, G.Tree(g, gh))), (i, got[i])
    d_costs = device((sum(len(c) for c in cands),), torch.float64)
    assert be.sync_gyro_costs(ranges, cands, out_ptr=d_costs.data_ptr()) is None
    assert G.same_bits(d_costs.cpu().numpy(), np.concatenate(got))
