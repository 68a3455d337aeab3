"""bench.py's plain run and `--dump-outputs`: the line of a plain run holds the headline fields
and none of the `--full` measurements, and the dumped files are the oracle's cost tables of the
same seeded frames."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
import oracle_lib as O
from mipgpu import layout
from mipgpu.synth import synth_frames

FULL_ONLY = ("filter", "single_frame_ms", "decisions_device", "cpu_baseline", "reference_gpu", "end_to_end")


def test_dump_positions_are_fixed_sorted_and_in_range():
    small = bench.dump_positions(1000)
    assert np.array_equal(small, np.arange(1000))                      # a small table: every entry
    total = 384 * 135 * layout.COSTS_PER_CTU                           # the default workload: past 2^31
    a, b = bench.dump_positions(total), bench.dump_positions(total)
    assert a.dtype == np.int64 and a.shape == (bench.DUMP_SAMPLE,) and np.array_equal(a, b)
    assert (np.diff(a) >= 0).all() and a[0] >= 0 and a[-1] < total and a[-1] > 2 ** 31
    assert 3 * 8 * bench.DUMP_SAMPLE < 64 << 20                         # sample + index + sums stay small


@pytest.mark.gpu
def test_plain_run_dumps_the_oracles_costs(gpu_available, tmp_path):
    w, h, n, seed = 264, 136, 3, 0xD0
    env = {k: v for k, v in os.environ.items() if not k.startswith("MIPGPU_")
           and k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, bench.__file__, "--gpus", "1", "--steps", "2", "--warmup", "1", "--width", str(w),
                        "--height", str(h), "--frames-per-step", str(n), "--seed", hex(seed),
                        "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stderr
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == 2 and line["warmup"] == 1 and line["n_gpus"] == 1 and line["unit"] == "frames/s"
    assert line["higher_is_better"] is True and line["dtype"] == "int16x2/int32" and line["ms_per_step"] > 0
    assert abs(line["value"] - n / (line["ms_per_step"] * 1e-3)) <= 0.01 * line["value"]
    assert not [k for k in FULL_ONLY if k in line]
    want = np.stack([O.search(f) for f in synth_frames(w, h, n, bench.shard_seed(seed, 0), 0)]).astype(np.int64)
    ctus = layout.num_ctus(w, h)
    got = {k: np.load(tmp_path / "out" / (k + ".npy")) for k in ("cost_ctu_sums", "cost_sample", "cost_sample_index")}
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["cost_sample_index"], np.arange(want.size))   # a small table is dumped whole
    assert np.array_equal(got["cost_sample"], want.reshape(-1))
    assert np.array_equal(got["cost_ctu_sums"], want.reshape(n, ctus, -1).sum(axis=2))
