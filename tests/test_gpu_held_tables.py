"""Frames held for a clip launch (GFW_OPT_COALESCE_FRAMES > 1) while the first pass's table is rebuilt under them.

The certified first pass reads a table that lives in ONE buffer per context (d_p1_table): s(rho) for the fisheye, T(r) for GoPro, Sony and the generic polynomial.
A frame whose rho range leaves the band the table was built for (dynamic zoom: a per-frame fov) or whose lens coefficients differ (a keyframed lens) rebuilds it.
Frames held before that keep their own range constants and certificates, so they must leave BEFORE the copy lands; they used to leave after it, read the new
table with the old constants and write wrong pixels (up to 70 % of a luma plane's bytes here; the audit builds, never held, could not see it).  Every frame here is compared bit for bit with the oracle
fed its own parameters; a frame-by-frame control of each schedule shows that the failure would come from holding, and that the schedule really moves the table.
"""
import pytest

from gyroflow_amd import abi, synthetic as S, warp
from test_gpu_coalesce import PlaneLoop
from test_gpu_pass1_radial import CLOSED_FORM_K, GOPRO_K, closed_form_lens, gopro_lens

pytestmark = pytest.mark.gpu

W, H = 384, 216                                  # 16:9; every lens below has f = 0.47 w

# a second coefficient set per model (a keyframed lens): far enough from the first that its table differs everywhere, near enough that it is still certified
SECOND_K = {
    "opencv_fisheye": [0.02, 0.05, -0.03, 0.008],
    "gopro": [0.0, 1.03, 0.0, -0.09, 0.01, 0.012, -0.005],
    "sony": [1.02, 0.0, -0.07, 0.025, 0.002, -0.0015],
    "generic_polynomial": [1.02, 0.0, -0.07, 0.025, 0.002, -0.0015, 0.0004, -0.0001, 0.0001, 0.0, 0.0, 0.00001],
}

# (fov, which coefficient set) per frame.  With device-resident matrices the host bounds the range from fov and f alone (gfw_api_certificate.inc p1_setup):
# fov 1.0 needs rho ~ 4.8 (fisheye table to ~5.6; radial r ~ 2.2, table to ~2.4), 1.3 needs rho ~ 10.3 (above the table: rebuilt larger), 0.5 needs ~1.1 (below half
# the table, or below 0.7 of r_max: rebuilt smaller), 1.05 needs ~5.5 (inside the band: kept).  The frame-by-frame control checks every one of these on the device.
SCHEDULES = {
    "fov_grows": ([(1.0, 0)] * 2 + [(1.3, 0)] * 2 + [(1.0, 0)] * 2, True),
    "fov_shrinks_below_half": ([(1.0, 0)] * 2 + [(0.5, 0)] * 2, True),
    "fov_alternates": ([(1.0, 0), (1.3, 0)] * 3, True),
    "k_changes": ([(1.0, 0)] * 2 + [(1.0, 1)] * 2, True),
    "fov_within_band": ([(1.0, 0)] * 2 + [(1.05, 0)] * 2, False),      # (control: the table stays)
    "long_grow_then_shrink": ([(1.0, 0)] * 4 + [(1.3, 0)] * 4 + [(1.0, 0)] * 4, True),
    "whole_launches": ([(1.0, 0)] * 4 + [(1.3, 0)] * 4, True),
}

CASES = [("opencv_fisheye", fmt, s) for fmt in ("YUV422P16LE", "NV12", "P010LE")
         for s in ("fov_grows", "fov_shrinks_below_half", "fov_alternates", "k_changes", "fov_within_band")]
CASES += [(m, "YUV422P16LE", s) for m in ("gopro", "sony", "generic_polynomial") for s in ("fov_grows", "fov_shrinks_below_half", "k_changes")]


def lens_of(model, second):
    if model == "opencv_fisheye":
        lens = S.gopro_style_lens(W, H)
        if second:
            lens["k"] = SECOND_K[model] + [0.0] * 8
        return lens
    if model == "gopro":
        return gopro_lens(W, H, k=SECOND_K[model] if second else GOPRO_K)
    return closed_form_lens(model, W, H, k=SECOND_K[model] if second else CLOSED_FORM_K[model])


def frames_of(model, fmt, schedule):
    return [S.SyntheticFrame(fmt, W, H, seed=0xB0A1 + j, timestamp_ms=1000.0 + 33.3 * j, fov=fov, lens=lens_of(model, second))
            for j, (fov, second) in enumerate(SCHEDULES[schedule][0])]


def expected_launches(sched, per_launch):
    """Frames with equal parameters share launches of up to `per_launch`; a frame whose parameters differ starts a new one."""
    n, run = 0, 0
    for j, step in enumerate(sched):
        run = run + 1 if j > 0 and step == sched[j - 1] else 1
        n += (run - 1) % per_launch == 0
    return n


def run_schedule(model, fmt, schedule, per_launch, shared_stream=False):
    """The per-plane calls of every frame of the schedule on a context per plane (jit = 2, device-resident tables, GFW_OPT_COALESCE_FRAMES = per_launch).
    Returns (backend after each frame, E after each frame or None, jit state, launches, frames launched, [mismatch messages])."""
    sched = SCHEDULES[schedule][0]
    label = "%s %s %s, %d per launch" % (model, fmt, schedule, per_launch)
    loop = PlaneLoop(frames_of(model, fmt, schedule), jit=2, frames_per_launch=per_launch, shared_stream=shared_stream)
    backends, eps, bad = [], [], []
    try:
        loop.be[0].set_option(abi.OPT_PROFILE, 1)            # the owner context (plane 0) launches every frame: clip_flush counts a launch and its frames there
        for j in range(len(sched)):
            loop.frame(j)
            backends.append(warp.Backend.last_backend_of(loop.be[0]))
            if per_launch == 1:                               # (gfw_get_audit flushes: only where nothing is held.  Word 6 is E of the owner's last frame, a
                eps.append(loop.be[0].get_audit_full()["pass1_eps_px"])   # function of the table and the lens, not of fov: it moves exactly when the table does)
        for be in loop.be:
            be.synchronize()
        _, launches, covered = loop.be[0].get_profile_frames()
        state = loop.be[0].jit_status()[0]
        for j in range(len(sched)):
            try:
                loop.check(j, label)
            except AssertionError as e:
                bad.append(str(e))
    finally:
        loop.close()
    return backends, (eps if per_launch == 1 else None), state, launches, covered, bad


def check_held(model, fmt, schedule, per_launch, shared_stream=False):
    sched = SCHEDULES[schedule][0]
    backends, _, state, launches, covered, bad = run_schedule(model, fmt, schedule, per_launch, shared_stream)
    assert state == 2, state                                  # the specialised kernel served the clip (the radial models' table is read by no other)
    for j in range(len(sched) - 1):
        if sched[j + 1] != sched[j]:                          # held when the table moves, and on the certified pass: the frame the hazard is about
            assert backends[j] == "yuv_fused_p1_jit", (j, backends)
    assert covered == len(sched) and launches == expected_launches(sched, per_launch), (launches, covered, expected_launches(sched, per_launch))
    assert not bad, "%d of %d frames differ from the oracle:\n%s" % (len(bad), len(sched), "\n".join(bad))


@pytest.mark.parametrize("model,fmt,schedule", CASES)
def test_held_frames_read_the_table_they_were_set_up_for(model, fmt, schedule):
    check_held(model, fmt, schedule, 4)


@pytest.mark.parametrize("shared_stream", [False, True])
def test_a_full_clip_launch_held_across_two_rebuilds(shared_stream):
    """GFW_OPT_COALESCE_FRAMES = GFW_CLIP_FRAMES_MAX: four frames held at each fov when the table grows, then shrinks."""
    check_held("opencv_fisheye", "YUV422P16LE", "long_grow_then_shrink", abi.CLIP_MAX, shared_stream)


@pytest.mark.parametrize("model,fmt,schedule", CASES + [("opencv_fisheye", "YUV422P16LE", "long_grow_then_shrink")])
def test_the_same_schedules_frame_by_frame(model, fmt, schedule):
    """The control: nothing held, so no frame can read another frame's table — this passes whether or not held frames are flushed before a rebuild.  It also
    shows that each schedule moves the table where it is meant to (E of the last frame changes exactly at the schedule's steps), and only there."""
    sched, crosses = SCHEDULES[schedule]
    backends, eps, _, launches, covered, bad = run_schedule(model, fmt, schedule, 1)
    assert all(b == "yuv_fused_p1_jit" for b in backends), backends
    moved = [j for j in range(1, len(sched)) if eps[j] != eps[j - 1]]
    steps = [j for j in range(1, len(sched)) if sched[j] != sched[j - 1]]
    assert moved == (steps if crosses else []), (moved, steps, eps)
    assert launches == covered == len(sched), (launches, covered)
    assert not bad, "%d of %d frames differ from the oracle:\n%s" % (len(bad), len(sched), "\n".join(bad))


def test_a_rebuild_between_whole_launches_costs_no_launch():
    """Batching does not get worse: four frames at fov 1.0 fill a launch, four at 1.3 (a larger table) the next — two launches, eight frames."""
    backends, _, _, launches, covered, bad = run_schedule("opencv_fisheye", "YUV422P16LE", "whole_launches", 4)
    assert (launches, covered) == (2, 8), (launches, covered)
    assert backends[3] == "yuv_fused_p1_jit", backends
    assert not bad, "\n".join(bad)
