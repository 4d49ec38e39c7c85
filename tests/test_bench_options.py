"""bench.py's --full / --dump-outputs options, host only: a plain run leaves out
the measurements that take runs of their own, and the dump writer keeps its
format (float32 .npy, a fixed seeded sample above the size limit)."""
import numpy as np
import torch

import bench
from test_bench_dist import _run_bench


def test_plain_run_leaves_out_the_collective_share():
    """Without --full a --tp run stops at the result line of the timed loop
    (test_bench_dist.test_bench_tp_groups_are_replicas is the --full side)."""
    rc, line, err = _run_bench(["--gpus", "2", "--tp", "2", "--plumbing", "--steps", "7"])
    assert rc == 0, err[-2000:]
    assert line["steps"] == 7 and line["ms_per_step"] >= 2.0
    assert "tp_collective" not in line


def test_dump_outputs_float32_and_seeded_sample(tmp_path):
    g = torch.Generator().manual_seed(0)
    small = torch.randn(2, 64, generator=g).bfloat16()
    big = torch.randn(3, 1000, generator=g, dtype=torch.float64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), dict(small=small, big=big), max_bytes=2 * (4 * 500 + 128))
    s, b = np.load(tmp_path / "a" / "small.npy"), np.load(tmp_path / "a" / "big.npy")
    assert s.dtype == np.float32 and s.shape == (2, 64)
    assert np.array_equal(s, small.float().numpy())           # bf16 -> float32 is exact
    # 3,000 elements against a share of 500: a sample of 500 of them, in order, the same in every run
    assert b.dtype == np.float32 and b.shape == (500,)
    flat = big.float().numpy().reshape(-1)
    idx = np.sort(np.random.default_rng(0).choice(flat.size, 500, replace=False))
    assert np.array_equal(b, flat[idx])
    assert np.array_equal(b, np.load(tmp_path / "b" / "big.npy"))
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 2 * (4 * 500 + 128)


def test_dump_limit_is_64_mb():
    assert bench.DUMP_MAX_BYTES <= 64e6
