"""bench.py's options: a plain run times the steps and nothing else, --full adds the other legs, --dump-outputs writes what
the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

LEG_KEYS = ('exact_f32_mfma_path', 'bf16x6_path', 'strict_precision', 'upr', 'dpp', 'shard64', 'autograd_loop', 'ese',
            'ese_replicas', 'cpu_baseline')


def test_bench_help_names_full_and_dump_outputs():
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--help'], cwd=ROOT, capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    assert '--full' in res.stdout and '--dump-outputs' in res.stdout


class _Step:
    """what dump_outputs reads of a TrainStep: the flat weights, the flat gradient and the model's buffers"""

    def __init__(self, n):
        g = torch.Generator().manual_seed(0)
        self.flat = torch.rand(n, generator=g)
        self.grad = torch.rand(n, generator=g)
        self.model = torch.nn.BatchNorm2d(5)
        self.model.running_mean.uniform_(generator=g)


def test_dump_outputs_writes_float32_arrays(tmp_path):
    import bench
    step = _Step(1000)
    loss = torch.tensor(0.25)
    sizes = bench.dump_outputs(str(tmp_path / 'out'), step, loss)
    assert sizes == {'loss': 1, 'params': 1000, 'grad': 1000, 'bn_buffers': 10}
    got = {k: np.load(str(tmp_path / 'out' / f'{k}.npy')) for k in sizes}
    assert all(a.dtype == np.float32 for a in got.values())
    assert got['loss'][0] == np.float32(0.25)
    np.testing.assert_array_equal(got['params'], step.flat.numpy())
    np.testing.assert_array_equal(got['grad'], step.grad.numpy())
    np.testing.assert_array_equal(got['bn_buffers'], np.concatenate([step.model.running_mean.numpy(),
                                                                     step.model.running_var.numpy()]))


def test_dump_outputs_samples_within_the_budget(tmp_path, monkeypatch):
    """past the byte budget an array is replaced by a fixed, seeded sample of its elements: the same one on every run"""
    import bench
    monkeypatch.setattr(bench, 'DUMP_BYTES', 4 * 1000)
    step = _Step(5000)
    a = bench.dump_outputs(str(tmp_path / 'a'), step, torch.tensor(1.0))
    b = bench.dump_outputs(str(tmp_path / 'b'), step, torch.tensor(1.0))
    assert a == b and sum(a.values()) * 4 <= 4 * 1000 and a['loss'] == 1
    total = 0
    for k in a:
        x, y = np.load(str(tmp_path / 'a' / f'{k}.npy')), np.load(str(tmp_path / 'b' / f'{k}.npy'))
        np.testing.assert_array_equal(x, y)
        total += x.nbytes
    assert total <= 4 * 1000
    assert np.isin(np.load(str(tmp_path / 'a' / 'params.npy')), step.flat.numpy()).all()


@pytest.mark.gpu
def test_bench_plain_run_times_the_steps_and_dumps_them(tmp_path):
    """a plain run prints the headline line without the --full legs, and --dump-outputs writes the last timed step's loss,
    weights, gradient and BatchNorm buffers"""
    import bench
    from mmlf_amd.feed_forward import FeedForward
    out = tmp_path / 'outputs'
    cmd = [sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--global-batch', '4', '--patch', '32',
           '--steps', '3', '--warmup', '1', '--dump-outputs', str(out)]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and lines[0].startswith('{'), res.stdout[-1500:]
    line = json.loads(lines[0])
    for k in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert k in line, k
    assert line['steps'] == 3 and line['ms_per_step'] > 0 and line['value'] > 0 and line['config']['full'] is False
    assert not [k for k in LEG_KEYS if k in line]
    n = sum(p.numel() for p in FeedForward(**bench.BASE_KW).parameters())
    got = {k: np.load(str(out / f'{k}.npy')) for k in ('loss', 'params', 'grad', 'bn_buffers')}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in got.values())
    assert got['params'].shape == (n,) and got['grad'].shape == (n,) and got['bn_buffers'].size > 0
    assert abs(float(got['loss'][0]) - line['config']['loss']) <= 1e-6 * max(1.0, abs(line['config']['loss']))
    assert sum(os.path.getsize(str(out / f)) for f in os.listdir(str(out))) <= 64 * 10 ** 6
