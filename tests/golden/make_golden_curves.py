"""Golden vectors for the operating point and the precision-recall sums, produced by the REFERENCE's
own code and the sklearn it calls, on CPU.  Run in the build container only (needs /root/reference,
sklearn):
    python tests/golden/make_golden_curves.py

Per label the fixture holds what ``evaluate_internal`` (ct_clip/evaluate.py:160-207) computes beside
the AUROC: ``choose_operating_point(*roc_curve(y, p))`` (evaluate.py:104-113), ``auc(recall,
precision)`` of ``precision_recall_curve(y, p)`` (``plot_pr``, evaluate.py:116-118) and sklearn's
``average_precision_score``; for the whole sample and for the 64 resamples of ``bootstrap``'s loop
(evaluate.py:325-336).  ``choose_operating_point`` returns no threshold: the threshold stored is the
``roc_curve`` threshold at the position its loop stops at (the loop is restated here with the
position kept, and asserted to give the function's own sens / spec).

Cases: four tables ``c0`` .. ``c3`` of N = Pos + Neg rows with class counts (Pos, Neg) = (64, 128),
(128, 64), (32, 32), (16, 256); each has four labels, scores quantised to 4, 16, 64 levels and
unquantised.  Per table: ``probs`` / ``labels`` [N, 4], ``indices`` [64, N] (``resample(arange(N),
random_state=i)``), ``point`` [4, 5] and ``boot`` [64, 4, 5] with columns sensitivity, specificity,
threshold, pr_auc, average_precision.  Power-of-two class counts make tpr and fpr exact in f64, so
the reference's floating ``tpr - fpr > J`` decides as exact integers do on the point estimates; the
resamples have arbitrary counts (tests/test_curves_cpu.py audits those).  No label and no resample
is one-class (asserted).  ``sklearn_version`` records the sklearn that ran."""
from __future__ import annotations

import os
import sys
import types
import warnings

import numpy as np
import torch
from safetensors.torch import save_file

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden  # noqa: E402  (stubs + reference path)

COUNTS = [(64, 128), (128, 64), (32, 32), (16, 256)]
LEVELS = [4, 16, 64, 0]                                     # 0: unquantised
S = 64


def one(E, y, p):
    """sens, spec, threshold, pr_auc, average_precision of one label by the reference / sklearn."""
    from sklearn.metrics import auc, average_precision_score, precision_recall_curve, roc_curve
    fpr, tpr, thr = roc_curve(y, p)
    sens, spec = E.choose_operating_point(fpr, tpr, thr)
    at, J = -1, 0                                            # the same loop, keeping the position
    for k, (_fpr, _tpr) in enumerate(zip(fpr, tpr)):
        if _tpr - _fpr > J:
            at, J = k, _tpr - _fpr
    assert at >= 0 and sens == tpr[at] and spec == 1 - fpr[at]
    precision, recall, _ = precision_recall_curve(y, p)
    return [float(sens), float(spec), float(thr[at]), float(auc(recall, precision)),
            float(average_precision_score(y, p))]


def main():
    make_golden.install_stubs()
    sys.path.insert(0, make_golden.REF)
    sys.modules.setdefault('h5py', types.ModuleType('h5py'))
    sys.modules.setdefault('seaborn', types.ModuleType('seaborn'))
    import sklearn
    from sklearn.utils import resample
    import ct_clip.evaluate as E
    warnings.simplefilter('ignore')
    g = np.random.default_rng(22)
    out = {}
    for c, (pos, neg) in enumerate(COUNTS):
        m = pos + neg
        probs = np.zeros((m, len(LEVELS)), dtype=np.float32)
        labels = np.zeros((m, len(LEVELS)), dtype=np.uint8)
        indices = np.stack([resample(np.arange(m), replace=True, random_state=i) for i in range(S)]).astype(np.int32)
        point = np.zeros((len(LEVELS), 5))
        boot = np.zeros((S, len(LEVELS), 5))
        for j, lv in enumerate(LEVELS):
            y = g.permutation(np.r_[np.ones(pos), np.zeros(neg)]).astype(np.uint8)
            x = np.clip(0.5 + 0.25 * g.standard_normal(m) + 0.2 * (y - 0.5), 0.0, 1.0)     # overlapping classes
            x = (np.minimum(np.floor(x * lv), lv - 1) / lv if lv else x).astype(np.float32)
            assert lv // 2 < len(np.unique(x)) <= lv if lv else len(np.unique(x)) > m // 2
            probs[:, j], labels[:, j] = x, y
            point[j] = one(E, y.astype(np.float64), x)
            for i, rows in enumerate(indices):
                assert 0 < y[rows].sum() < m                 # never one class
                boot[i, j] = one(E, y[rows].astype(np.float64), x[rows])
            print(f'Pos {pos} Neg {neg} levels {lv or "none"}: point', point[j])
        assert np.isfinite(point).all() and np.isfinite(boot).all()
        for k, v in dict(probs=probs, labels=labels, indices=indices, point=point, boot=boot).items():
            out[f'c{c}.{k}'] = torch.from_numpy(v)
    out['counts'] = torch.tensor(COUNTS, dtype=torch.int64)
    out['levels'] = torch.tensor(LEVELS, dtype=torch.int64)
    out['sklearn_version'] = torch.tensor([int(v) for v in sklearn.__version__.split('.')[:3]], dtype=torch.int64)
    path = os.path.join(HERE, 'golden_curves.safetensors')
    save_file({k: v.contiguous() for k, v in out.items()}, path,
              metadata={'generator': 'tests/golden/make_golden_curves.py', 'sklearn': sklearn.__version__,
                        'columns': 'sensitivity, specificity, threshold, pr_auc, average_precision',
                        'reference': 'sharonct/CTPA-CLIP @ 2025-06-20 (ct_clip/evaluate.py:104-118,160-207,325-336)'})
    print('->', path, os.path.getsize(path), 'bytes; sklearn', sklearn.__version__)


if __name__ == '__main__':
    main()
