"""bench.py's own surface: the --dump-outputs sample (no GPU) and a plain run end to end (GPU)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _load(d, name):
    a = np.load(os.path.join(d, name + ".npy"))
    assert a.dtype == np.float64
    return a


def test_dump_outputs_is_a_fixed_sample_under_the_cap(tmp_path):
    import torch

    import bench
    n, k = 400_000, 16
    rng = np.random.default_rng(1)
    neigh = torch.from_numpy(rng.integers(0, n, size=(n, k), dtype=np.int32))
    normals = torch.from_numpy(rng.standard_normal((n, 3)))
    labels = torch.from_numpy(rng.integers(-1, 1000, size=n, dtype=np.int32))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), n, {"neighbours": neigh, "normals": normals, "labels": labels})
    total = sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a"))
    assert total <= 64 << 20
    rows = _load(tmp_path / "a", "rows")
    assert 0 < len(rows) < n and np.all(np.diff(rows) > 0) and rows[-1] < n
    idx = rows.astype(np.int64)
    assert np.array_equal(_load(tmp_path / "a", "neighbours"), neigh.numpy()[idx].astype(np.float64))
    assert np.array_equal(_load(tmp_path / "a", "normals"), normals.numpy()[idx])
    assert np.array_equal(_load(tmp_path / "a", "labels"), labels.numpy()[idx].astype(np.float64))
    for name in ("rows", "neighbours", "normals", "labels"):
        assert np.array_equal(_load(tmp_path / "a", name), _load(tmp_path / "b", name)), name


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_dumps_the_last_step(oracle, tmp_path):
    out = tmp_path / "out"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "plane_cube_100k", "--steps", "2",
                        "--warmup", "1", "--dump-outputs", str(out)], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-3000:]
    d = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["metric"] and d["unit"] == "Mpoints/s" and d["higher_is_better"] is True and d["dtype"]
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["steps"] == 2 and d["warmup"] == 1
    assert not {"cpu_baseline", "secondary", "concurrent_clouds", "audit"} & set(d), "a plain run measured more"
    import bench
    xyz, k = bench.make_cloud("plane_cube_100k")
    rows = _load(out, "rows")
    assert np.array_equal(rows, np.arange(len(xyz)))  # 100 k rows fit under the cap: the whole output
    oneigh, onormals = oracle.knn_normals(xyz, k=k)
    opi, _ = oracle.region_grow(xyz, onormals, oneigh)
    assert np.array_equal(_load(out, "neighbours"), oneigh.astype(np.float64))
    assert np.abs(_load(out, "normals") - onormals).max() <= 1e-5
    assert np.array_equal(_load(out, "labels"), opi.astype(np.float64))
