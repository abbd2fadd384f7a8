"""Driver-contract tests for bench.py: single-process CPU run and the
torchrun multi-rank launch path (gloo backend, 127.0.0.1 rendezvous)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

TINY = ['--dim', '32', '--depth', '1', '--crop-len', '32',
        '--msa-depth', '4', '--batch', '1', '--dtype', 'fp32',
        '--steps', '2', '--warmup', '1']


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _parse_last_json(out):
    for line in reversed(out.strip().splitlines()):
        if line.startswith('{'):
            return json.loads(line)
    raise AssertionError(f'no JSON line in output:\n{out}')


@pytest.mark.timeout(300)
def test_bench_single_process_cpu():
    out = subprocess.run(
        [sys.executable, 'bench.py'] + TINY,
        cwd=ROOT, capture_output=True, text=True, timeout=280)
    assert out.returncode == 0, out.stderr[-2000:]
    d = _parse_last_json(out.stdout)
    assert d['n_gpus'] == 1
    assert d['value'] > 0
    assert d['config']['global_batch'] == 1
    assert d['metric'].startswith('training samples/sec')
    assert d['scaling'] == 'weak'
    assert d['data'] == 'synthetic'


@pytest.mark.timeout(300)
def test_bench_dump_outputs_reproducible(tmp_path):
    """--dump-outputs writes the last timed step's loss and logits as
    float32 .npy files within the byte budget, and two runs with the same
    arguments (one of them --full) write identical arrays."""
    import numpy as np

    def run(name, extra):
        d = tmp_path / name
        out = subprocess.run(
            [sys.executable, 'bench.py'] + TINY
            + ['--dump-outputs', str(d)] + extra,
            cwd=ROOT, capture_output=True, text=True, timeout=140)
        assert out.returncode == 0, out.stderr[-2000:]
        res = _parse_last_json(out.stdout)
        assert res['steps'] == 2 and res['ms_per_step'] > 0
        assert res['value'] == pytest.approx(1e3 / res['ms_per_step'])
        return {f: np.load(d / f) for f in sorted(os.listdir(d))}

    a = run('a', [])
    b = run('b', ['--full'])
    assert sorted(a) == ['distance_logits.npy', 'loss.npy']
    assert a['distance_logits.npy'].shape == (1, 32, 32, 37)
    assert np.isfinite(a['loss.npy']).all()
    assert sum(v.nbytes for v in a.values()) <= 64 * 10**6
    for f in a:
        assert a[f].dtype == np.float32
        np.testing.assert_array_equal(a[f], b[f])


def test_bench_dump_outputs_budget(tmp_path):
    """An array larger than its share of the budget is stored as a
    fixed sample: same indices every time, sorted, within the budget."""
    import importlib.util

    import numpy as np
    import torch
    spec = importlib.util.spec_from_file_location(
        'bench', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)

    big = torch.arange(1000, dtype=torch.float64).reshape(10, 100)
    small = torch.ones(3, dtype=torch.bfloat16)
    for name in ('x', 'y'):
        bench.dump_outputs(str(tmp_path / name), {'big': big, 'small': small},
                           budget=412)
    x_big = np.load(tmp_path / 'x' / 'big.npy')
    assert np.load(tmp_path / 'x' / 'small.npy').tolist() == [1.0] * 3
    assert x_big.dtype == np.float32 and x_big.shape == (100,)
    assert (np.diff(x_big) > 0).all()          # distinct, sorted indices
    np.testing.assert_array_equal(x_big, np.load(tmp_path / 'y' / 'big.npy'))


@pytest.mark.timeout(300)
def test_bench_torchrun_two_ranks_cpu():
    env = dict(os.environ)
    env['MASTER_ADDR'] = '127.0.0.1'
    out = subprocess.run(
        [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1',
         '--nproc-per-node', '2', '--master-addr', '127.0.0.1',
         '--master-port', str(_free_port()), 'bench.py', '--gpus', '2'] + TINY,
        cwd=ROOT, capture_output=True, text=True, timeout=280, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    d = _parse_last_json(out.stdout)
    assert d['n_gpus'] == 2
    assert d['config']['global_batch'] == 2
    assert d['config']['parallelism'] == 'dp2'
