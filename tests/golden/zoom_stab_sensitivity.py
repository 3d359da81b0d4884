"""Produces tests/golden/zoom_stab_sensitivity.json: tests/golden/zoom_rotation_sensitivity.py's measurement for the statement clips of gfw_zoom_fovs_stab
(tests/_zoomstab.py: per-point IBIS/OIS shifts, per-frame meshes).  Host statement and the oracle's point map only.

For every clip, 10 draws per frame: every entry of every f32 rotation of the frame is displaced by a random -2 .. +2 ULP (seed fixed per clip; a frame without
rolling shutter has one rotation and one displacement), find_fov runs again, and the largest relative change of fov_minimal and the largest absolute change of a
debug-polygon coordinate over the clip's draws are recorded.  tests/test_emu_zoom_stab.py and tests/test_gpu_zoom_stab.py allow twice the recorded maxima.

    python tests/golden/zoom_stab_sensitivity.py        (from the repository root; a few minutes on 8 cores)
"""
import json
import multiprocessing
import os
import sys
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
DRAWS_PER_FRAME = 10


def measure(index):
    import _zoomstab as ZS
    clip = ZS.stab_clips()[index]
    rng = np.random.default_rng(zlib.crc32(clip.name.encode()))
    worst_fov = worst_poly = 0.0
    same = 0
    for k in range(len(clip.timestamps)):
        base, base_dbg = ZS.frame_fov(clip, k)
        for _ in range(DRAWS_PER_FRAME):
            v, dbg = ZS.frame_fov(clip, k, None, rng)
            worst_fov = max(worst_fov, abs(v - base) / base)
            worst_poly = max(worst_poly, float(np.max(np.abs(dbg - base_dbg))))
            same += v == base
    return clip.name, {"fov_max_rel": worst_fov, "polygon_max_abs": worst_poly, "draws": DRAWS_PER_FRAME * len(clip.timestamps), "bit_identical_draws": int(same)}


if __name__ == "__main__":
    import _zoomstab as ZS
    n = len(ZS.stab_clips())
    with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as pool:
        out = dict(pool.map(measure, range(n)))
    with open(os.path.join(ROOT, "tests", "golden", "zoom_stab_sensitivity.json"), "w") as f:
        json.dump({"ulp": 2, "draws_per_frame": DRAWS_PER_FRAME, "clips": out}, f, indent=1, sort_keys=True)
        f.write("\n")
