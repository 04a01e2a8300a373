"""bench.py: the reduction --dump-outputs writes (table_outputs, on the CPU) and a plain one-GPU run end to end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
import bench  # noqa: E402

OUTPUT_NAMES = ["stats", "table_block_sums", "table_sample", "table_sample_pos"]


@pytest.mark.parametrize("cells", [1000, bench.DUMP_CELLS, 3 * bench.DUMP_CELLS + 5])
def test_table_outputs_cover_every_cell_within_the_size_limit(cells):
    t = torch.from_numpy(np.random.default_rng(cells).integers(0, 256, cells + 16, dtype=np.uint8))
    o = bench.table_outputs(torch, t, cells, 7, 9)
    assert sorted(o) == OUTPUT_NAMES
    assert all(a.dtype in (np.float32, np.float64) for a in o.values())
    assert sum(a.nbytes for a in o.values()) <= 64 << 20
    assert list(o["stats"]) == [7, 9]
    sums = o["table_block_sums"]
    assert len(sums) <= bench.DUMP_CELLS and sums.sum() == int(t[:cells].sum())      # every cell of the table, none beyond it
    pos = o["table_sample_pos"].astype(np.int64)
    assert len(pos) <= bench.DUMP_CELLS and pos.max() < cells
    assert np.array_equal(o["table_sample"], t.numpy()[pos].astype(np.float32))
    again = bench.table_outputs(torch, t, cells, 7, 9)
    assert all(np.array_equal(o[k], again[k]) for k in o)


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_the_same_outputs_twice(tmp_path):
    """a plain run: the headline line only (no secondary workloads, CPU baseline or single passes), --steps timed steps, and outputs that
    two runs with the same arguments write identically"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("LIME_")}      # bench.py refuses the test hooks
    lines, dumps = [], []
    for i in range(2):
        d = tmp_path / f"out{i}"
        r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1", "--workload", "c2", "--dump-outputs", str(d)],
                           capture_output=True, timeout=600, env=env, cwd=ROOT)
        assert r.returncode == 0, r.stderr.decode()[-3000:]
        lines.append(json.loads([ln for ln in r.stdout.decode().splitlines() if ln.startswith("{")][-1]))
        dumps.append({n: np.load(d / (n + ".npy")) for n in OUTPUT_NAMES})
    line = lines[0]
    assert line["steps"] == 3 and line["warmup"] == 1 and line["full"] is False and line["value"] > 0 and line["ms_per_step"] > 0
    assert line["unit"] == "symbols/s" and line["higher_is_better"] is True and line["dtype"] == "u8"
    assert "also" not in line and "cpu_baseline" not in line and line["roofline"]["pass_ms_each"] is None
    assert list(dumps[0]["stats"]) == [line["config"]["n_clusters"], line["config"]["max_cluster_len"]]
    assert dumps[0]["table_sample"].max() > 0 and 0 < len(dumps[0]["table_sample_pos"]) <= bench.DUMP_CELLS
    assert all(np.array_equal(dumps[0][n], dumps[1][n]) for n in OUTPUT_NAMES)
