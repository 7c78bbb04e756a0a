"""bench.py --dump-outputs: the last timed step's outputs as float32 / float64 .npy files -- the same seeded
sample of rows in every run, inside the size budget -- and the options a plain / full run is chosen by.
CPU only (the tensors stand in for what ElasticBuffer.combine returned)."""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _outputs(T, H, K):
    g = torch.Generator().manual_seed(5)
    return torch.randn((T, H), generator=g).to(torch.bfloat16), torch.rand((T, K), generator=g)


def test_dump_samples_rows_within_budget(tmp_path, monkeypatch):
    import bench
    T, H, K = 96, 64, 4
    monkeypatch.setattr(bench, 'DUMP_ROWS_BYTES', 40 * H * 4)      # room for 40 of the 96 rows
    x, w = _outputs(T, H, K)
    a, b = tmp_path / 'a', tmp_path / 'b'
    bench._dump_outputs(str(a), 0, 1, x, w)
    bench._dump_outputs(str(b), 0, 1, x, w)
    assert sorted(os.listdir(a)) == ['combined_topk_weights.npy', 'combined_x.npy', 'combined_x_rows.npy']
    got, rows, gw = (np.load(a / f'{n}.npy') for n in ('combined_x', 'combined_x_rows', 'combined_topk_weights'))
    assert got.dtype == np.float32 and rows.dtype == np.float64 and gw.dtype == np.float32
    assert got.shape == (40, H) and got.nbytes <= 40 * H * 4
    idx = rows.astype(np.int64)
    assert len(set(idx.tolist())) == 40 and np.array_equal(idx, np.sort(idx)) and 0 <= idx[0] and idx[-1] < T
    assert np.array_equal(got, x.float().numpy()[idx])              # bf16 -> float32 is exact
    assert np.array_equal(gw, w.numpy())
    for n in os.listdir(a):                                        # the same rows from run to run
        assert np.array_equal(np.load(a / n), np.load(b / n))


def test_dump_whole_output_when_it_fits_and_per_rank_names(tmp_path):
    import bench
    x, w = _outputs(33, 16, 2)
    bench._dump_outputs(str(tmp_path), 1, 2, x, None)
    assert sorted(os.listdir(tmp_path)) == ['combined_x_rank1.npy', 'combined_x_rows_rank1.npy']
    assert np.array_equal(np.load(tmp_path / 'combined_x_rank1.npy'), x.float().numpy())
    assert np.array_equal(np.load(tmp_path / 'combined_x_rows_rank1.npy'), np.arange(33, dtype=np.float64))


def test_default_budget_is_under_64_mb():
    import bench
    T, H, K = 8192, 7168, 8                                         # the flagship batch
    n = min(T, bench.DUMP_ROWS_BYTES // (H * 4))
    assert n * H * 4 + n * 8 + T * K * 4 + 3 * 128 <= 64 * 10 ** 6


def test_options_listed_and_steps_checked():
    bench = os.path.join(ROOT, 'bench.py')
    r = subprocess.run([sys.executable, bench, '--help'], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and '--full' in r.stdout and '--dump-outputs DIR' in r.stdout
    r = subprocess.run([sys.executable, bench, '--steps', '0'], capture_output=True, text=True, timeout=120)
    assert r.returncode == 3 and '--steps must be >= 1' in r.stderr
