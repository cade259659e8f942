"""bench.py's plain run and --dump-outputs: the plain line carries the headline fields and leaves the --full side
measurements null; the dumped array is what the timed path assembled (compared entry for entry with the same sharded
step made here on the same seeded inputs); an array above the size budget is written as a fixed seeded sample."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NX, NY = 96, 20      # 3840 triangles = 60 tiles of 64 elements: several workgroups, boundary and interior tiles


def test_dump_outputs_samples_above_the_budget(tmp_path, monkeypatch):
    import torch

    import bench
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 8 * 1000)
    small = torch.arange(300, dtype=torch.float64)      # two arrays, one rank: 500 values each
    large = torch.arange(100003, dtype=torch.float64) * 0.5
    for d in ("a", "b"):
        bench.dump_outputs(torch, str(tmp_path / d), [small, large], 1, 0)
    s0, s1 = np.load(tmp_path / "a" / "stiffness_values_0.npy"), np.load(tmp_path / "a" / "stiffness_values_1.npy")
    assert s0.dtype == np.float64 and np.array_equal(s0, small.numpy())          # under its share: whole
    assert s1.dtype == np.float64 and s1.shape == (500,)
    # the sample: sorted indices over the whole array, the same from run to run
    idx = (s1 * 2).astype(np.int64)
    assert np.all(np.diff(idx) >= 0) and idx[0] < 10000 and idx[-1] > 90000
    assert np.array_equal(large.numpy()[idx], s1)
    assert np.array_equal(s1, np.load(tmp_path / "b" / "stiffness_values_1.npy"))
    # N > 1: one file per rank, the budget shared
    bench.dump_outputs(torch, str(tmp_path / "c"), [large], 2, 1)
    assert np.load(tmp_path / "c" / "stiffness_values_0_rank1.npy").shape == (500,)


@pytest.mark.gpu
@pytest.mark.timeout(120)
def test_plain_bench_line_and_dumped_values(tmp_path):
    import torch

    import hdd_amd as H
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--nx", str(NX), "--ny", str(NY), "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=100, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["full"] is False
    assert d["unit"] == "DoFs/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    dofs = 3 * 2 * NX * NY
    assert d["ms_per_step"] > 0 and abs(d["value"] - dofs / (d["ms_per_step"] * 1e-3)) <= 1e-9 * d["value"]
    assert d["cpu_baseline"] is None and d["roofline"]["attainable"] is None
    assert d["roofline"]["frac_of_torch_copy"] is None and d["roofline"]["frac"] > 0
    assert sorted(os.listdir(tmp_path)) == ["stiffness_values_0.npy"]
    got = np.load(tmp_path / "stiffness_values_0.npy")
    # the same step here: bench.py's single-rank C2 set-up at this size
    ctx = H.Context(0)
    grid = H.Grid.structured(H.SIMPLEX, NX, NY, (0.0, 0.0), (5.0, 1.0), px=1, py=1)
    shard = H.Shard(ctx, grid, 1, 0)
    perm = 10.0 ** np.random.default_rng(10).uniform(-3.0, 3.0, size=2000)
    k = torch.from_numpy(shard.checkerboard((0.0, 0.0), (5.0, 1.0), 100, 20, perm)).cuda()
    pat = shard.pattern(ctx, 0)
    vals = [torch.empty(shard.info.nnz, dtype=torch.float64, device="cuda")]
    H.assemble_sharded(ctx, shard, None, [H.scalar_fn(H.FN_CONST, 1.0)],
                       H.tensor_fn(H.TENSOR_ISO_PER_ELEM, per_elem=k), pat[3], vals)
    torch.cuda.synchronize()
    assert got.dtype == np.float64 and got.shape == (shard.info.nnz,) == (d["config"]["nnz_per_gpu"],)
    assert np.array_equal(got, vals[0].cpu().numpy())
