"""The coordinate kernels of gfw_kernels.hip — STMap "undist" export (stmap.rs:87-109) and the inverse point map `undistort_points`
(cpu_undistort.rs:652-858) — host-interpreted (tests/_emu.py) against the golden maps and the oracle: the CPU-tier twins of tests/test_gpu_stmap.py
and tests/test_gpu_points.py (same inputs, bit-identical results; NaN compares equal to NaN)."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
import make_golden as G  # noqa: E402

from gyroflow_amd import abi, synthetic as S  # noqa: E402
import _emu  # noqa: E402
import _oracle as O  # noqa: E402
import _coordcase as K  # noqa: E402
from test_gpu_lens_models import PHYSICAL, DIGITAL, synthetic_mesh  # noqa: E402
from test_gpu_points import wild_points, same_bits  # noqa: E402
from test_oracle_points import points_params  # noqa: E402

GOLD = json.load(open(os.path.join(HERE, "golden", "golden.json")))


@pytest.mark.parametrize("name", sorted(G.MAP_CASES))
def test_coordinate_kernels_reproduce_the_golden_maps(name):
    case = G.MAP_CASES[name]
    fr, kp, pp, mode = G.map_inputs(case)
    g = GOLD["maps"][name]
    assert zlib.crc32(_emu.stmap_undistort(kp, fr.model, 0, fr.matrices, case["w"], case["h"]).tobytes()) == g["undist"]
    assert zlib.crc32(_emu.undistort_points(pp, fr.model, 0, fr.rotations, grid=(case["w"], case["h"]), index_mode=mode).tobytes()) == g["dist"]


@pytest.mark.parametrize("model", sorted(PHYSICAL))
def test_every_lens_model_both_directions(model):
    w, h = 240, 136
    lens = S.gopro_style_lens(w, h)
    lens["model"] = model
    lens["k"] = PHYSICAL[model] + [0.0] * (12 - len(PHYSICAL[model]))
    if model == "gopro":
        lens["r_limit"] = 2.5
    fr = S.SyntheticFrame("YUV422P16LE", w, h, seed=61, lens=lens, fov=1.3)
    kp = fr.planes[0]["params"].copy()
    kp.flags = 0
    assert same_bits(O.stmap_undistort(kp, fr.model, 0, fr.matrices, w, h), _emu.stmap_undistort(kp, fr.model, 0, fr.matrices, w, h))
    pp = points_params(fr)
    pts = wild_points(w, h, 6000, 7)
    rows = np.nan_to_num(np.clip(np.round(pts[:, 1]), 0, h - 1), nan=0.0, posinf=h - 1, neginf=0).astype(np.int64)
    rot = fr.rotations[rows]
    assert same_bits(O.undistort_points(pp, fr.model, 0, rot, points=pts, index_mode=abi.POINT_INDEX_PER_POINT),
                     _emu.undistort_points(pp, fr.model, 0, rot, points=pts, index_mode=abi.POINT_INDEX_PER_POINT))


@pytest.mark.parametrize("digital", sorted(DIGITAL))
def test_points_digital_lens_refraction_stretch(digital):
    w, h = 256, 144
    lens = S.gopro_style_lens(w, h)
    lens["digital"] = digital
    fr = S.SyntheticFrame("NV12", w, h, seed=67, lens=lens, fov=1.1, base_overrides={"digital_lens_params": DIGITAL[digital]})
    kp = points_params(fr)
    kp.light_refraction_coefficient = 1.33
    kp.input_horizontal_stretch, kp.input_vertical_stretch = 1.2, 0.9
    pts = wild_points(w, h, 5000, 11)
    assert same_bits(O.undistort_points(kp, fr.model, fr.digital, fr.rotations, points=pts, index_mode=abi.POINT_INDEX_SINGLE),
                     _emu.undistort_points(kp, fr.model, fr.digital, fr.rotations, points=pts, index_mode=abi.POINT_INDEX_SINGLE))


@pytest.mark.parametrize("hrs", [False, True])
def test_dist_grid_with_shifts(hrs):
    w, h = 256, 144
    fr = S.SyntheticFrame("YUV422P16LE", w, h, seed=71, fov=1.2, horizontal_rs=hrs)
    kp = points_params(fr)
    t = np.arange(fr.rotations.shape[0], dtype=np.float64)
    shifts = np.stack([1.5 * np.sin(t / 37.0), -0.8 * np.cos(t / 23.0), 0.004 * np.sin(t / 51.0), 0.3 * np.cos(t / 19.0), 0.2 * np.sin(t / 29.0)], axis=1).astype(np.float32)
    mode = abi.POINT_INDEX_PER_COLUMN if hrs else abi.POINT_INDEX_PER_ROW
    for sh in (None, shifts):
        assert same_bits(O.undistort_points(kp, fr.model, 0, fr.rotations, grid=(w, h), shifts=sh, index_mode=mode),
                         _emu.undistort_points(kp, fr.model, 0, fr.rotations, grid=(w, h), shifts=sh, index_mode=mode))


@pytest.mark.parametrize("with_mesh,with_fpd", [(True, True), (False, True)])
def test_points_sony_mesh_f64(with_mesh, with_fpd):
    w, h = 192, 120
    lens = S.gopro_style_lens(w, h)
    lens["model"], lens["k"] = "sony", PHYSICAL["sony"] + [0.0] * 6
    fr = S.SyntheticFrame("YUV422P16LE", w, h, seed=73, lens=lens, fov=1.2)
    kp = points_params(fr)
    mesh = synthetic_mesh(w, h, with_fpd, with_mesh).astype(np.float64)
    mesh[20:40] += 1e-11
    assert same_bits(O.undistort_points(kp, fr.model, 0, fr.rotations, grid=(w, h), index_mode=abi.POINT_INDEX_PER_ROW, mesh=mesh),
                     _emu.undistort_points(kp, fr.model, 0, fr.rotations, grid=(w, h), index_mode=abi.POINT_INDEX_PER_ROW, mesh=mesh))


@pytest.mark.parametrize("model,lca,digital", [("opencv_fisheye", 0.4, None), ("gopro", 0.7, "gopro_superview"), ("poly5", 0.2, None)])
def test_points_lens_correction_branch(model, lca, digital):
    w, h = 200, 120
    lens = S.gopro_style_lens(w, h)
    lens["model"], lens["k"] = model, PHYSICAL[model] + [0.0] * (12 - len(PHYSICAL[model]))
    ov = {"lens_correction_amount": lca}
    if digital:
        lens["digital"] = digital
        ov["digital_lens_params"] = DIGITAL[digital]
    fr = S.SyntheticFrame("YUV422P16LE", w, h, seed=83, lens=lens, fov=1.25, base_overrides=ov)
    kp = points_params(fr)
    kp.lens_correction_amount = lca
    kp.fov = fr.planes[0]["params"].fov
    pts = wild_points(w, h, 3000, 13)
    assert same_bits(O.undistort_points(kp, fr.model, fr.digital, fr.rotations, points=pts, index_mode=abi.POINT_INDEX_SINGLE),
                     _emu.undistort_points(kp, fr.model, fr.digital, fr.rotations, points=pts, index_mode=abi.POINT_INDEX_SINGLE))


# ---- the undist export's case table (tests/_coordcase.py): rejected rays, the block edge, meshes, digital lenses, IBIS rows, one matrix ------------------

@pytest.mark.parametrize("name", K.NAMES)
def test_stmap_case_table_from_a_sentinel(name):
    """Every element starts from a NaN payload and the maps are compared as uint32: what the kernel rejects must keep those bits, what it writes must be
    the oracle's value, and nothing may land in another pixel (203 x 117 and the shapes around one workgroup: the x / y guards fire in both directions)."""
    fr, kp, mesh, w, h = K.case(name)
    ref = K.reference(name)
    got = _emu.stmap_undistort(kp, fr.model, fr.digital, fr.matrices, w, h, mesh=mesh, fill=K.SENTINEL)
    assert np.array_equal(ref.view(np.uint32), got.view(np.uint32))


def test_stmap_ignores_the_fields_the_closure_does_not_read():
    """lens_correction_amount, translation2d, input_rotation and background_mode belong to the render: the map of `unread` is rl_gopro's."""
    assert np.array_equal(K.reference("unread").view(np.uint32), K.reference("rl_gopro").view(np.uint32))


def test_stmap_mesh_reaches_the_oracle():
    """(the helper's `mesh=` is new: a dropped mesh on both sides would compare equal)"""
    fr, kp, mesh, w, h = K.case("mesh_fisheye")
    plain = O.stmap_undistort(kp, fr.model, fr.digital, fr.matrices, w, h, fill=K.SENTINEL)
    assert np.abs(plain - K.reference("mesh_fisheye")).max() > 0.25


@pytest.mark.parametrize("place", ["end", "start"])
def test_stmap_small_shapes_between_guard_pages(place):
    """The shapes around one workgroup with the map, the matrix table and the mesh flush against an inaccessible page (tests/emu/guard_coords.py, one process per
    placement: a store by a lane past the map's edge ends it with SIGSEGV), and the maps still the oracle's."""
    r = subprocess.run([sys.executable, os.path.join(HERE, "emu", "guard_coords.py"), place] + K.SMALL + ["mesh_fisheye"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, "gfw_stmap_kernel touched memory outside its buffers (%s guard): rc %d\n%s" % (place, r.returncode, r.stderr[-1500:])
    assert r.stdout.split() == ["OK"] * (len(K.SMALL) + 1), r.stdout[-500:]


def test_dist_grid_with_fewer_rotations_than_rows():
    """rotation_count = 3 under _PER_ROW on a 203 x 117 grid: rows 3 and above take rotation 0 (`rot_per_point.get(index).unwrap_or(&rr)`), not the last one."""
    fr = K.case("ibis_rs")[0]
    kp = points_params(fr)
    rot = fr.rotations[[0, 58, 116]]
    ref = O.undistort_points(kp, fr.model, 0, rot, grid=(K.W, K.H), index_mode=abi.POINT_INDEX_PER_ROW)
    assert same_bits(ref, _emu.undistort_points(kp, fr.model, 0, rot, grid=(K.W, K.H), index_mode=abi.POINT_INDEX_PER_ROW))
    single = O.undistort_points(kp, fr.model, 0, rot[:1], grid=(K.W, K.H), index_mode=abi.POINT_INDEX_SINGLE)
    assert same_bits(ref[3:], single[3:]) and np.abs(ref[1:3] - single[1:3]).max() > 0.01
    assert np.abs(ref[3:] - O.undistort_points(kp, fr.model, 0, rot[2:], grid=(K.W, K.H), index_mode=abi.POINT_INDEX_SINGLE)[3:]).max() > 0.01
