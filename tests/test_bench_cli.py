"""bench.py's command line and --dump-outputs writer (host only; the timed path itself is GPU)."""
import sys
import types

import numpy as np
import torch

import bench


def _parse(monkeypatch, *argv):
    monkeypatch.setattr(sys, 'argv', ['bench.py', *argv])
    return bench.parse()


def test_plain_and_full_options(monkeypatch):
    a = _parse(monkeypatch, '--gpus', '1', '--steps', '7', '--warmup', '2')
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    a = _parse(monkeypatch, '--full', '--dump-outputs', 'd', '--no-cpu-baseline')
    assert a.full and a.dump_outputs == 'd' and a.no_cpu_baseline and not a.no_precise


def test_dump_outputs_samples_large_arrays_at_fixed_positions(monkeypatch, tmp_path):
    monkeypatch.setattr(bench, 'DUMP_SAMPLE', 64)
    data = torch.arange(1000, dtype=torch.float32)
    vq = types.SimpleNamespace(codebook=torch.ones(8, 8), state=types.SimpleNamespace(last_indices=torch.arange(10)))
    model = types.SimpleNamespace(visual_transformer=types.SimpleNamespace(vq=vq))
    trainer = types.SimpleNamespace(norm=torch.tensor([3.0, 0.5]), flat=types.SimpleNamespace(data=data), m=-data)
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), torch.tensor(1.5), trainer, model)
    got = {f.stem: np.load(f) for f in (tmp_path / 'a').iterdir()}
    assert sorted(got) == ['adam_m', 'grad_norm_clip_coef', 'loss', 'params', 'vq_codebook', 'vq_indices']
    assert all(v.dtype == np.float32 and v.ndim == 1 for v in got.values())
    assert got['loss'].tolist() == [1.5] and got['grad_norm_clip_coef'].tolist() == [3.0, 0.5]
    assert got['vq_codebook'].shape == (64,) and got['vq_indices'].tolist() == list(range(10))
    # the sample: DUMP_SAMPLE sorted positions, the same for both arrays of that size and for every run
    p = got['params']
    assert p.shape == (64,) and (np.diff(p) >= 0).all() and (got['adam_m'] == -p).all()
    assert (np.load(tmp_path / 'b' / 'params.npy') == p).all()
