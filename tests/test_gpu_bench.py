"""GPU: a plain `bench.py` run — the headline line only, exactly --steps timed frames — and `--dump-outputs`, the same arrays on two runs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import ROOT


def _bench(args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1"] + args, env=env, capture_output=True, text=True, timeout=600,
                       cwd=str(ROOT))
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    return json.loads([ln for ln in p.stdout.strip().splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_bench_dumps_the_same_outputs_twice(tmp_path):
    dirs = [tmp_path / "a", tmp_path / "b"]
    lines = [_bench(["--steps", "6", "--warmup", "2", "--dump-outputs", str(d)]) for d in dirs]
    for d in lines:
        assert d["steps"] == 6 and d["warmup"] == 2 and d["ms_per_step"] > 0 and d["value"] > 0 and d["unit"] == "frames/s"
        assert d["higher_is_better"] is True and d["dtype"] == "f32" and d["config"]["full"] is False
        # what --full adds is not run
        assert "cpu_baseline" not in d and d["config"]["frames_per_s_with_S_streams_per_gpu"] is None
        assert d["config"]["frames_per_s_with_mesh_left_in_hbm"] is None
    names = sorted(p.name for p in dirs[0].iterdir())
    assert names == sorted(p.name for p in dirs[1].iterdir())
    for want in ("frame_triangles", "frame_triangle_voxel_ids", "frame_triangle_std", "mesh_triangles", "map_latent_vecs", "map_voxel_pos"):
        assert f"{want}.npy" in names
    total = 0
    for nm in names:
        a, b = np.load(dirs[0] / nm), np.load(dirs[1] / nm)
        assert a.dtype in (np.float32, np.float64), nm
        assert np.array_equal(a, b, equal_nan=True), nm
        total += (dirs[0] / nm).stat().st_size
    assert total <= 64_000_000
    tri, tid, tstd = (np.load(dirs[0] / f"frame_{k}.npy") for k in ("triangles", "triangle_voxel_ids", "triangle_std"))
    assert tri.shape[1:] == (3, 3) and tid.shape == tri.shape[:1] and tstd.shape == (tri.shape[0], 3)
    n = np.load(dirs[0] / "map_latent_vecs.npy").shape[0]
    assert n > 1000 and np.load(dirs[0] / "map_voxel_pos.npy").shape == (n,) and np.load(dirs[0] / "mesh_triangles.npy").shape[0] > 1000
