"""Driver-contract guard: `python bench.py` must emit ONE JSON line with
the agreed fields (the round driver parses this output verbatim), and
`--dump-outputs DIR` must write the last timed round's outputs as
reproducible .npy files.  Runs the real benchmark on CPU at minimum size."""

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

REPO = Path(__file__).resolve().parents[1]


def _run_bench(*extra):
    out = subprocess.run(
        [sys.executable, str(REPO / 'bench.py'), '--steps', '1',
         '--warmup', '0', '--agents_per_gpu', '1', *extra],
        capture_output=True, text=True, timeout=600, cwd=str(REPO))
    assert out.returncode == 0, out.stderr[-2000:]
    json_lines = [l for l in out.stdout.splitlines()
                  if l.startswith('{') and l.endswith('}')]
    assert len(json_lines) == 1, out.stdout[-2000:]
    return json.loads(json_lines[0])


@pytest.fixture(scope='module')
def plain_run(tmp_path_factory):
    d = tmp_path_factory.mktemp('plain')
    return _run_bench('--dump-outputs', str(d)), d


def test_bench_json_contract(plain_run):
    d, _ = plain_run
    for field in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup',
                  'ms_per_step', 'higher_is_better', 'scaling',
                  'vs_baseline', 'dtype', 'data', 'config'):
        assert field in d, field
    assert d['metric'] == 'fl_rounds_per_sec'
    assert d['n_gpus'] == 1 and d['steps'] == 1 and d['warmup'] == 0
    assert d['higher_is_better'] is True and d['scaling'] == 'weak'
    assert d['dtype'] == 'fp32' and d['data'] == 'synthetic'
    assert d['value'] > 0 and d['ms_per_step'] > 0
    assert abs(d['value'] * d['ms_per_step'] - 1000.0) < 1e-6 * 1000.0
    cfg = d['config']
    assert cfg['model'] and 'global_batch' in cfg and 'parallelism' in cfg


def test_bench_dump_outputs(plain_run, tmp_path):
    """The dump holds the global model after the last timed round, as
    finite fp32/fp64 arrays; a second run with the same arguments (here
    with --full as well) starts from identical inputs, so on the CPU path
    it reproduces them bit for bit."""
    from rlr_amd.models import CNN_MNIST
    _, d0 = plain_run
    d1 = _run_bench('--full', '--dump-outputs', str(tmp_path))
    assert d1['metric'] == 'fl_rounds_per_sec' and d1['steps'] == 1
    names = sorted(p.name for p in d0.iterdir())
    assert names == ['global_params.npy', 'sampled_agents.npy']
    assert sorted(p.name for p in tmp_path.iterdir()) == names
    n_params = sum(p.numel() for p in CNN_MNIST().parameters())
    total = 0
    for name in names:
        a, b = np.load(d0 / name), np.load(tmp_path / name)
        assert a.dtype in (np.float32, np.float64)
        assert np.isfinite(a).all()
        assert a.dtype == b.dtype and np.array_equal(a, b), name
        total += a.nbytes
    assert total <= 64 * 2 ** 20
    params = np.load(d0 / 'global_params.npy')
    assert params.shape == (n_params,) and params.dtype == np.float32
    assert params.std() > 0
    assert np.load(d0 / 'sampled_agents.npy').tolist() == [0.0]
