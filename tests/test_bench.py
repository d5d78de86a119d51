"""bench.py's --dump-outputs writer on the CPU: every cloud's rows in cloud order, float32, and above the size cap a fixed,
seeded sample of the rows with their indices (the GPU side: tests/test_gpu_bench.py)."""
import numpy as np

import bench

NAMES = ("normals", "expert", "probs")


def _outs():
    rng = np.random.default_rng(5)
    return [(rng.standard_normal((n, 3)).astype(np.float32), rng.integers(0, 7, n).astype(np.int32),
             rng.random((n, 7)).astype(np.float32)) for n in (300, 200)]


def _load(d):
    return {k: np.load(d / (k + ".npy")) for k in NAMES + (("rows",) if (d / "rows.npy").exists() else ())}


def test_dump_outputs_writes_every_cloud_in_float32(tmp_path):
    outs = _outs()
    bench.dump_outputs(str(tmp_path / "d"), outs)
    got = _load(tmp_path / "d")
    assert set(got) == set(NAMES) and all(a.dtype == np.float32 for a in got.values())
    for i, k in enumerate(NAMES):
        assert np.array_equal(got[k], np.concatenate([o[i] for o in outs]).astype(np.float32)), k


def test_dump_outputs_samples_the_same_rows_above_the_cap(tmp_path, monkeypatch):
    outs = _outs()
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 100 * (4 * (3 + 1 + 7) + 8))      # room for 100 rows and their indices
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), outs)
    a, b = _load(tmp_path / "a"), _load(tmp_path / "b")
    rows = a["rows"]
    assert rows.dtype == np.float64 and len(rows) == 100 and np.all(np.diff(rows) > 0) and rows[-1] < 500
    assert sum(x.nbytes for x in a.values()) <= bench.DUMP_MAX_BYTES
    for i, k in enumerate(NAMES):
        assert a[k].dtype == np.float32
        assert np.array_equal(a[k], np.concatenate([o[i] for o in outs]).astype(np.float32)[rows.astype(np.int64)]), k
    for k in a:
        assert np.array_equal(a[k], b[k]), k
