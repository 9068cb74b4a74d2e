"""bench.py's plain run and `--dump-outputs`: the secondary workloads sit
behind `--full`, and the dump holds what the timed path left in C — whole
when it fits the size budget, else a fixed, seeded sample of its rows."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))


def _parse(argv, monkeypatch):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
    return bench.parse()


def test_plain_run_is_the_default(monkeypatch):
    a = _parse(["--gpus", "1", "--steps", "7", "--warmup", "3"], monkeypatch)
    assert a.full is False and a.dump_outputs is None
    assert (a.steps, a.warmup) == (7, 3)
    a = _parse(["--full", "--dump-outputs", "d"], monkeypatch)
    assert a.full is True and a.dump_outputs == "d"


def test_dump_whole_when_it_fits(tmp_path):
    import bench
    import torch
    C = torch.arange(300 * 200, dtype=torch.float32).reshape(300, 200)
    bench.dump_outputs(torch, tmp_path / "a" / "b", 0, 1, C)
    got = np.load(tmp_path / "a" / "b" / "sgemm_C_rank0.npy")
    assert got.dtype == np.float32 and np.array_equal(got, C.numpy())


@pytest.mark.parametrize("world", [1, 8])
def test_dump_samples_rows_within_the_budget(tmp_path, world):
    import bench
    import torch
    n = 4096
    # row r holds r in every column: the rows kept can be read off the file
    C = torch.arange(n, dtype=torch.float32).reshape(n, 1).expand(n, n).contiguous()
    bench.dump_outputs(torch, tmp_path, 2, world, C)
    f = tmp_path / "sgemm_C_rank2.npy"
    got = np.load(f)
    assert got.dtype == np.float32 and got.shape[1] == n
    assert world * f.stat().st_size <= 64 * 10 ** 6
    rows = got[:, 0].astype(np.int64)
    assert np.all(got == got[:, :1])                      # whole rows
    assert np.all(np.diff(rows) > 0) and rows[-1] < n     # distinct, ascending
    assert len(rows) == bench.DUMP_BUDGET_BYTES // world // (4 * n)
    # the same rows on the next run, whichever rank writes them
    bench.dump_outputs(torch, tmp_path, 0, world, C)
    assert np.array_equal(np.load(tmp_path / "sgemm_C_rank0.npy"), got)


@pytest.mark.gpu
def test_dump_is_the_timed_paths_product(hip, torch_cuda, ora, tmp_path):
    """The dumped C of a small timed run is the oracle's NN product of the
    seeded operands, bit for bit (300 is no multiple of a tile), and a second
    run writes the same file."""
    import bench
    from tensorium_amd.dist import DistCtx
    torch = torch_cuda
    ctx = DistCtx(None, 0, 1, 0, "cuda:0", 0)
    n = 300
    dumps = []
    for d in ("one", "two"):
        wall, mean_ms, min_ms, Cm = bench.bench_sgemm(torch, hip, ctx, 0, n, 3, 2)
        assert wall > 0 and 0 < min_ms <= mean_ms
        bench.dump_outputs(torch, tmp_path / d, 0, 1, Cm)
        dumps.append(np.load(tmp_path / d / "sgemm_C_rank0.npy"))
    A = bench.synthetic(torch, (n, n), 2000).cpu().numpy()
    B = bench.synthetic(torch, (n, n), 2500).cpu().numpy()
    ref = np.zeros((n, n), np.float32)
    ora.sgemm(False, False, n, n, n, 1.0, A, n, B, n, 0.0, ref, n)
    assert dumps[0].dtype == np.float32 and dumps[0].shape == (n, n)
    assert np.array_equal(dumps[0], ref), float(np.abs(dumps[0] - ref).max())
    assert np.array_equal(dumps[0], dumps[1])
