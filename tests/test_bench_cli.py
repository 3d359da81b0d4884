"""bench.py's command line without a device: a plain run measures the headline only (--full turns on the roofline brackets, the oracle's parity
and the CPU baseline), and --dump-outputs writes float32 arrays within its size budget, sampled at the same positions run after run."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("gfw_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_and_full_command_lines():
    b = _bench()
    plain = b.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5"])
    assert (plain.steps, plain.warmup, plain.full, plain.profile_every, plain.dump_outputs) == (20, 5, False, 0, "")
    full = b.parse_args(["--gpus", "1", "--steps", "20", "--warmup", "5", "--full", "--dump-outputs", "out"])
    assert (full.full, full.profile_every, full.dump_outputs) == (True, 8, "out")
    assert b.parse_args(["--full", "--profile-every", "1"]).profile_every == 1
    assert b.parse_args(["--profile-every", "4"]).profile_every == 4


def test_dump_outputs_small_arrays_are_written_whole(tmp_path):
    b = _bench()
    planes = {"plane0": np.arange(12, dtype=np.uint16).reshape(3, 4), "plane1": np.linspace(-1, 1, 6).astype(np.float16)}
    b.dump_outputs(str(tmp_path), planes)
    assert sorted(os.listdir(tmp_path)) == ["plane0.npy", "plane1.npy"]
    for name, a in planes.items():
        got = np.load(tmp_path / (name + ".npy"))
        assert got.dtype == np.float32 and got.shape == a.shape and np.array_equal(got, a.astype(np.float32))


def test_dump_outputs_large_arrays_are_a_fixed_sample_within_the_budget(tmp_path):
    b = _bench()
    rng = np.random.default_rng(3)
    planes = {"plane0": rng.integers(0, 65536, (216, 384), dtype=np.uint16), "plane1": rng.integers(0, 65536, (216, 192), dtype=np.uint16)}
    budget = 4 * 30000
    for d in ("a", "b"):
        b.dump_outputs(str(tmp_path / d), planes, budget=budget)
    total = 0
    for name, a in planes.items():
        x, y = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert x.dtype == np.float32 and x.ndim == 1 and np.array_equal(x, y)
        assert x.size == a.size * (budget // 4) // sum(p.size for p in planes.values())
        assert np.isin(x, a.reshape(-1).astype(np.float32)).all()
        total += x.nbytes
    assert total <= budget
