"""bench.py --dump-outputs / --full (host logic only, no GPU): the options
parse, the dump is float32 .npy files under the size cap, and an array over
its share is written as the same seeded sample every time."""
import os
import sys

import numpy as np

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)


def test_plain_run_is_the_default_and_full_is_an_option():
    import bench
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = bench.parse(["--full", "--dump-outputs", "somewhere"])
    assert a.full and a.dump_outputs == "somewhere"
    assert bench.DUMP_MAX_VALUES * 4 + 4096 <= 64_000_000  # float32 values and .npy headers within 64 MB


def test_dump_is_float32_whole_when_it_fits(tmp_path):
    import bench
    ok = np.arange(1000) % 3 == 0
    sigs = (np.arange(1000 * 96) % 251).astype(np.uint8).reshape(1000, 96)
    bench.dump_outputs(str(tmp_path / "d"), {"ok": ok, "recovered": sigs})
    got_ok, got = np.load(tmp_path / "d" / "ok.npy"), np.load(tmp_path / "d" / "recovered.npy")
    assert got_ok.dtype == got.dtype == np.float32
    assert np.array_equal(got_ok, ok.astype(np.float32)) and np.array_equal(got, sigs.astype(np.float32))


def test_dump_samples_an_oversized_array_reproducibly(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_VALUES", 5000)
    small, big = np.ones(100, dtype=bool), np.arange(100_000, dtype=np.int64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"small": small, "big": big})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert np.load(tmp_path / "a" / "small.npy").size == 100  # the small array is whole
    assert a.size == 4900 and np.array_equal(a, b)
    assert np.all(np.diff(a) > 0) and set(a.astype(np.int64)) <= set(big.tolist())  # distinct values of the input
