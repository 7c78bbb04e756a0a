"""A plain `bench.py --gpus 1` run on the GPU: the line holds the headline (`value`, `ms_per_step`, the steps it
was asked for) and none of the measurements that belong to --full, and --dump-outputs writes the last timed
step's outputs.  One small batch, one child process (bench.py is the thing under test)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, 'bench.py')

pytestmark = pytest.mark.gpu


def test_plain_run_line_and_dump(tmp_path):
    T, H, K, E = 160, 1024, 8, 32
    r = subprocess.run([sys.executable, BENCH, '--gpus', '1', '--steps', '3', '--warmup', '1', '--tokens', str(T),
                        '--hidden', str(H), '--topk', str(K), '--experts', str(E), '--dump-outputs', str(tmp_path)],
                       capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    assert line['steps'] == 3 and line['warmup'] == 1 and line['full'] is False
    assert line['unit'] == 'GB/s' and line['higher_is_better'] is True and line['dtype'] == 'bf16'
    assert line['value'] > 0 and line['ms_per_step'] > 0
    for moved in ('roofline', 'cpu_baseline', 'cpu_torch', 'loopback', 'dispatch', 'phases', 'single_reduction'):
        assert line[moved] is None, moved
    x, rows, w = (np.load(tmp_path / f'{n}.npy') for n in ('combined_x', 'combined_x_rows', 'combined_topk_weights'))
    assert x.dtype == np.float32 and x.shape == (T, H) and w.shape == (T, K)
    assert np.array_equal(rows, np.arange(T, dtype=np.float64))
    assert np.isfinite(x).all() and np.abs(x).max() > 0
    assert ((w > 0) & (w < 1)).all()                    # the routing weights, passed through
