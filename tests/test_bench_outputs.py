"""bench.py --dump-outputs / --full: a plain run prints the headline line only and can write the
last timed solve's (x, info) as .npy; everything that takes runs of its own sits behind --full."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench

ROOT = os.path.join(os.path.dirname(__file__), "..")
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")
FULL_ONLY = ("true_rel_residual", "spmv", "roofline", "roofline_spmv", "sec8d_reconciliation", "kernels",
             "cpu_baseline", "line_precond_solve")


def test_dump_short_vector_is_written_whole(tmp_path):
    import torch
    x = torch.arange(1000, dtype=torch.float64) * 0.5
    bench.dump_outputs(str(tmp_path / "d"), x, 0, 0, 1)
    got = np.load(tmp_path / "d" / "x.npy")
    assert got.dtype == np.float64 and np.array_equal(got, x.numpy())
    info = np.load(tmp_path / "d" / "info.npy")
    assert info.dtype == np.float64 and info.tolist() == [0.0]


def test_dump_long_vector_is_a_fixed_sorted_sample(tmp_path):
    import torch
    n = bench.DUMP_SAMPLE + 12345
    x = torch.arange(n, dtype=torch.float64)   # value = position
    bench.dump_outputs(str(tmp_path / "a"), x, 1, 0, 1)
    bench.dump_outputs(str(tmp_path / "b"), x, 1, 0, 1)
    a, b = np.load(tmp_path / "a" / "x.npy"), np.load(tmp_path / "b" / "x.npy")
    assert a.dtype == np.float64 and a.shape == (bench.DUMP_SAMPLE,)
    assert np.array_equal(a, b)                              # the same positions in every run
    assert np.all(np.diff(a) >= 0) and a[0] >= 0 and a[-1] < n
    assert a[-1] > bench.DUMP_SAMPLE                          # drawn from the whole vector, not a prefix
    assert a.nbytes + 8 <= 64 * 2**20
    assert np.load(tmp_path / "a" / "info.npy").tolist() == [1.0]


def test_dump_names_per_rank_files(tmp_path):
    import torch
    bench.dump_outputs(str(tmp_path), torch.ones(8, dtype=torch.float64), 0, 1, 2)
    assert sorted(os.listdir(tmp_path)) == ["info_rank1.npy", "x_rank1.npy"]


def test_steps_must_be_positive():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"],
                       capture_output=True, text=True, timeout=60)
    assert p.returncode == 2 and "--steps" in p.stderr


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_the_solution(gpu, vk_lib, tmp_path):
    """One plain C1 run (1M rows): the line holds the headline and nothing that --full measures;
    x.npy is the solution the library returns for the same operator and RHS (two solves of one
    build agree to the parity suite's 1e-9 bar)."""
    vk = vk_lib
    d = tmp_path / "out"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "C1",
                        "--steps", "2", "--warmup", "1", "--dump-outputs", str(d)],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    for k in HEADLINE:
        assert k in out, k
    for k in FULL_ONLY:
        assert k not in out, k
    assert out["full"] is False and out["steps"] == 2 and len(out["info"]) == 2
    assert out["ms_per_step"] > 0 and abs(out["value"] * out["ms_per_step"] / 1e3 - out["inner_iters_per_solve"]) \
        <= 1e-6 * out["inner_iters_per_solve"]
    assert sorted(os.listdir(d)) == ["info.npy", "x.npy"]
    x = np.load(d / "x.npy")
    dim, shape, fp32 = bench.CONFIGS["C1"]
    n = int(np.prod(shape))
    assert x.dtype == np.float64 and x.shape == (n,) and n <= bench.DUMP_SAMPLE
    assert np.load(d / "info.npy").tolist() == [0.0]
    A = vk.vlasov_operator(vk.vlasov_params(dim, shape, fp32=fp32), ctx=gpu)
    M = vk.block_jacobi(A, 8)
    xr, info = vk.gmres(A, vk.rhs_splitmix(n), rtol=1e-8, restart=20, M=M)
    assert info == 0
    assert np.linalg.norm(x - xr) / np.linalg.norm(xr) <= 1e-9
    M.close()
    A.close()
