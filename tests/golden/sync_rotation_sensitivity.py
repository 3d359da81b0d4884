"""Produces tests/golden/sync_rotation_sensitivity.json: how far the sync search's mapped points and costs move when the f32 rotations it maps the points with move
in their last bits.  Uses only the host statement (tests/_syncstmt.py) and the oracle's point map.

The device evaluates the slerp of a rotation with its own f64 acos / sin, the statement with the host libm's; the project's standing bar for that stage is <= 2 ULP
of f32 per matrix entry (tests/test_gpu_matrix_builder.py).  For every test clip of tests/_synccase.py (the "gpu" ranges, both modes) and every candidate the
statement's search visits (coarse and fine), DRAWS times: every entry of every f32 rotation is displaced by a random -2 .. +2 ULP (_zoomstmt.mapper_for's `perturb`;
seed fixed per clip; a side without rolling shutter has one rotation and one displacement), and the largest change of a mapped point's coordinate (pixels; points the
lens inverse rejects stay (-1e6, -1e6) on both sides) and of a candidate's cost are recorded per clip.  The tests allow twice the recorded maxima.

    python tests/golden/sync_rotation_sensitivity.py        (from the repository root; a few minutes on 8 cores)
"""
import json
import multiprocessing
import os
import sys

os.environ.setdefault("OMP_NUM_THREADS", "1")      # eight workers: numpy keeps to one thread each
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
DRAWS = 2


def measure(case):
    import _synccase as SC
    import _syncstmt as SS
    name, mode = case
    rng, _ = SC.planted(name, "gpu", mode)
    gen = np.random.default_rng(zlib.crc32(("%s/%d" % (name, mode)).encode()))
    st = SC.stored(name, "gpu", mode)
    coarse = SC.stage_candidates(name, "gpu", mode)
    fine = SC.stage_candidates(name, "gpu", mode, coarse[st["coarse_pick"]][0 if mode == 0 else 1])
    worst_pt = worst_cost = 0.0
    moved = 0
    for (offs, readout), base_cost in zip(coarse + fine, st["coarse_costs"] + st["fine_costs"]):
        base = SS.mapped_points(rng, offs, readout)
        assert SS.fold_mapped(rng, base) == base_cost, (case, offs, readout)
        for _ in range(DRAWS):
            m = SS.mapped_points(rng, offs, readout, gen)
            worst_pt = max(worst_pt, float(np.max(np.abs(m - base))))
            c = SS.fold_mapped(rng, m)
            worst_cost = max(worst_cost, abs(c - base_cost))
            moved += c != base_cost
    return name, mode, worst_pt, worst_cost, moved, DRAWS * len(coarse + fine)


if __name__ == "__main__":
    import _synccase as SC
    cases = [(n, m) for m in (1, 0) for n in sorted(SC.CLIPS)]
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        rows = pool.map(measure, cases, chunksize=1)
    out = {}
    for name, mode, pt, cost, moved, draws in rows:
        e = out.setdefault(name, {"point_max_abs_px": 0.0, "cost_max_abs": 0.0, "draws": 0, "draws_with_another_cost": 0})
        e["point_max_abs_px"], e["cost_max_abs"] = max(e["point_max_abs_px"], pt), max(e["cost_max_abs"], cost)
        e["draws"] += draws
        e["draws_with_another_cost"] += int(moved)
    with open(os.path.join(ROOT, "tests", "golden", "sync_rotation_sensitivity.json"), "w") as f:
        json.dump({"ulp": 2, "draws_per_candidate": DRAWS, "clips": out}, f, indent=1, sort_keys=True)
        f.write("\n")
