"""The STMap "undist" map held to its purpose: it is where the render samples.  gfw_stmap_kernel restates the rolling-shutter row pick on its own and the
oracle's gfw_oracle_stmap_undistort is a separate restatement too; the reference's fixture pins only the render.  So: render a frame whose source holds its own
coordinates — pixel (x, y) = (x, y, 0, 1), bilinear — and the render's red / green channels must be the map (oracle against oracle here; libgfwarp's render against
libgfwarp's map in tests/test_gpu_stmap.py).  Bicubic and Lanczos4 stay out: their quantised tap tables do not reproduce a ramp (0.03-0.06 px)."""
import numpy as np
import pytest

import _oracle as O
import _coordcase as K


@pytest.mark.parametrize("name", sorted(K.STATEMENT_CASES))
def test_the_undist_map_is_where_the_render_samples(name):
    """Bound: 1/64 px + 2 ULP(200) = 0.015656 — derived from the sampler (K.map_against_render), not measured.  Seen on the oracle when written
    (share of pixels at least 4 px inside the source / largest difference): fisheye_1.4_rs 0.837 / 0.015625, fisheye_1.4_hrs 0.841 / 0.015625,
    fisheye_0.8_rs 1.000 / 0.015625, sony_mesh 1.000 / 0.015625, digital_stretch 0.999 / 0.015625."""
    fr, mesh = K.ramp_frame(name)
    w, h = K.STATEMENT_W, K.STATEMENT_H
    rg = K.render_rg(fr, O.run_frame(fr, mesh=mesh)[0])
    coords = O.stmap_undistort(K.stmap_params(fr), fr.model, fr.digital, fr.matrices, w, h, mesh=mesh, fill=K.SENTINEL)
    share, worst, bound = K.map_against_render(rg, coords, w, h)
    print("%s: inside share %.3f, max |render.rg - map| %.6f px (bound %.6f)" % (name, share, worst, bound))
    assert share >= K.INSIDE_SHARE, share
    assert worst <= bound, (worst, bound)
