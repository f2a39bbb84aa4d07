"""Golden vectors for the evaluation loader and the validation metrics, produced by the
REFERENCE's own code on CPU.  Run in the build container only (needs /root/reference, sklearn,
pandas):
    python tests/golden/make_golden_eval.py

  * loader: ``CTReportDatasetinfer.nii_img_to_tensor`` (ct_clip/data_inference.py:78-122) called as
    is on synthetic npz files, at its own target (480, 480, 240).  Stored shapes below the target
    on every axis, and above it on d, h and w in turn (odd differences: the floor divisions are
    asymmetric); f32 and f64 sources; values beyond both clip bounds.  The fixture stores the input,
    the non-pad box (offset + contents); everything else of the (240, 480, 480) output is -1
    (asserted here).
  * metrics: ``evaluate_internal`` (ct_clip/evaluate.py:160-207) on the whole sample and on the
    resamples of ``bootstrap``'s loop (evaluate.py:325-336; that function itself calls an
    ``evaluate`` the module does not define, so its loop is restated around evaluate_internal),
    ``compute_cis`` (evaluate.py:272-303), and the trainer's micro-F1 / flat accuracy
    (CTCLIPTrainer.py:434-445).  N = 61, P = 5, S = 64; probabilities quantised to 1/16 (ties);
    label 1 has 2 positives (one-class resamples -> NaN), label 2 is perfectly separated, label 3
    inverted.

Plotting imports that are not installed (h5py, seaborn) are stubbed at import."""
from __future__ import annotations

import os
import sys
import tempfile
import types
import warnings

import numpy as np
import torch
from safetensors.torch import save_file

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (stubs + reference path)

LOADER_SHAPES = [(13, 21, 18), (250, 6, 9), (5, 491, 7), (3, 7, 483)]     # stored (a0, a1, a2) = (d, h, w)
N, P, S = 61, 5, 64


def loader_cases(out):
    import ct_clip.data_inference as DI
    with tempfile.TemporaryDirectory() as tmp:
        for k, shape in enumerate(LOADER_SHAPES):
            # f64 sources where the dtype can matter (the w axis: padded, cropped); the d / h crops only
            # pick other rows, and their f64 copies would put the fixture near the 1 MiB file limit
            for dt in (np.float32, np.float64) if k in (0, 3) else (np.float32,):
                name = f'vol{k}_{np.dtype(dt).name}'
                g = np.random.default_rng(100 + 2 * k + (dt is np.float64))
                scan = (g.random(shape) * 1.8 - 1.3).astype(dt)           # x 1000: [-1300, 500]
                path = os.path.join(tmp, name + '.npz')
                np.savez(path, scan)
                t = DI.CTReportDatasetinfer.nii_img_to_tensor(None, path, None)
                assert t.shape == (1, 240, 480, 480) and t.dtype == torch.float32
                t = t[0]
                d, h, w = shape
                lo = [max((240 - d) // 2, 0), max((480 - h) // 2, 0), max((480 - w) // 2, 0)]
                ext = [min(d, 240), min(h, 480), min(w, 480)]
                box = t[lo[0]:lo[0] + ext[0], lo[1]:lo[1] + ext[1], lo[2]:lo[2] + ext[2]].contiguous()
                assert int((t != -1).sum()) == int((box != -1).sum())      # nothing but -1 outside the box
                v = scan * 1000
                assert v.min() < -1000 and v.max() > 200
                out[f'{name}.scan'] = torch.from_numpy(scan)
                out[f'{name}.box_lo'] = torch.tensor(lo, dtype=torch.int64)
                out[f'{name}.box'] = box
                print(name, shape, 'box at', lo, 'extent', ext)


def metric_cases(out):
    sys.modules.setdefault('h5py', types.ModuleType('h5py'))
    sys.modules.setdefault('seaborn', types.ModuleType('seaborn'))
    import pandas as pd
    from sklearn.metrics import accuracy_score, f1_score
    from sklearn.utils import resample
    import ct_clip.evaluate as E
    g = np.random.default_rng(7)
    y = np.zeros((N, P), dtype=np.uint8)
    y[:, 0] = g.random(N) < 0.4
    y[g.choice(N, 2, replace=False), 1] = 1
    y[:, 2] = g.random(N) < 0.5
    y[:, 3] = g.random(N) < 0.3
    y[:, 4] = g.random(N) < 0.6
    q = g.integers(0, 17, size=(N, P))                                      # sixteenths
    q[:, 2] = np.where(y[:, 2] == 1, g.integers(9, 17, N), g.integers(0, 8, N))      # separated
    q[:, 3] = np.where(y[:, 3] == 1, g.integers(0, 6, N), g.integers(6, 17, N))      # inverted
    probs = (q / 16).astype(np.float32)
    names = [f'label{j}' for j in range(P)]
    real = y.astype(np.float64)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        devnull = open(os.devnull, 'w')
        stdout, sys.stdout = sys.stdout, devnull                             # evaluate_internal prints shapes
        try:
            point = E.evaluate_internal(probs, real, names, None)
            idx = np.arange(len(real))
            rows, stats = [], []
            for i in range(S):
                sample = resample(idx, replace=True, random_state=i)
                rows.append(sample)
                stats.append(E.evaluate_internal(probs[sample], real[sample], names, None))
        finally:
            sys.stdout = stdout
    boot = pd.concat(stats)
    cis = E.compute_cis(boot)
    assert list(cis.index) == ['mean', 'lower', 'upper']
    b = boot.to_numpy(dtype=np.float64)
    assert np.isnan(b[:, 1]).any() and not np.isnan(b[:, [0, 2, 3, 4]]).any()
    pt = point.to_numpy(dtype=np.float64)[0]
    assert pt[2] == 1.0 and pt[3] == 0.0
    real_i, pred_i = np.rint(real).astype(int), np.rint(probs).astype(int)
    out['met.probs'] = torch.from_numpy(probs)
    out['met.labels'] = torch.from_numpy(y)
    out['met.indices'] = torch.from_numpy(np.stack(rows).astype(np.int32))
    out['met.boot_auroc'] = torch.from_numpy(b)
    out['met.auroc'] = torch.from_numpy(pt)
    out['met.cis'] = torch.from_numpy(cis.to_numpy(dtype=np.float64))       # rows mean, lower, upper
    out['met.f1_micro'] = torch.tensor([f1_score(real_i, pred_i, average='micro')], dtype=torch.float64)
    out['met.flat_accuracy'] = torch.tensor([accuracy_score(real_i.flatten(), pred_i.flatten())],
                                            dtype=torch.float64)
    print('point AUROC', pt, 'NaN resamples of label 1:', int(np.isnan(b[:, 1]).sum()))
    print(cis)


def main():
    make_golden.install_stubs()
    sys.path.insert(0, make_golden.REF)
    out = {}
    loader_cases(out)
    metric_cases(out)
    path = os.path.join(HERE, 'golden_eval.safetensors')
    save_file({k: v.contiguous() for k, v in out.items()}, path, metadata={'generator': 'tests/golden/make_golden_eval.py',
                                   'reference': 'sharonct/CTPA-CLIP @ 2025-06-20 (ct_clip/data_inference.py:78-122, '
                                                'ct_clip/evaluate.py:160-207,272-337, '
                                                'ct_clip/CTCLIPTrainer.py:434-445)'})
    print('->', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
