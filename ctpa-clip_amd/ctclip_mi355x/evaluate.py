"""Zero-shot validation metrics on the HIP path: what the reference's trainer computes every
``save_results_every`` steps (``ct_clip/CTCLIPTrainer.py:356-454``) from the zero-shot scores --
per-pathology AUROC (``ct_clip/evaluate.py:160-207``: ``roc_curve`` + ``auc``), micro-F1 and flat
accuracy of the rounded predictions (``CTCLIPTrainer.py:434-445``) -- and the bootstrap confidence
intervals of ``ct_clip/evaluate.py:272-337`` (``bootstrap`` / ``compute_cis``).

The reference's bootstrap is 1,000 resamples x 18 ``roc_curve`` calls on the host.  Here each
label is sorted once (``torch.sort``) and one kernel (``ctclip_auroc_boot``, csrc/metrics.hip)
walks that order for every (resample, label) with the resample's row multiplicities as weights:
the tie-aware Mann-Whitney count in 64-bit integers, one f64 division.  The resamples are the
reference's own (``sklearn.utils.resample(idx, replace=True, random_state=i)``), drawn with numpy.

A second kernel (``ctclip_curve_boot``) walks the same order for what ``evaluate_internal`` computes
beside the AUROC and drops: the Youden operating point (``choose_operating_point``,
evaluate.py:104-113) with its threshold, and the area under the precision-recall curve
(``plot_pr``, evaluate.py:116-118), plus sklearn's average precision -- ``curve_metrics`` /
``bootstrap_curve_metrics``, opt-in through ``ZeroShotEvaluator.evaluate(..., curves=True)``.
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import call, ptr, stream_ptr

MAX_ROWS = 8192          # the cap of ctclip_auroc_boot / ctclip_curve_boot (LDS): more rows raise KernelError (CT_ESHAPE)


def bootstrap_indices(n, n_samples):
    """[n_samples, n] int32: row i is ``sklearn.utils.resample(np.arange(n), replace=True,
    random_state=i)`` (evaluate.py:329), i.e. ``RandomState(i).randint(0, n, size=n)``."""
    out = np.empty((n_samples, n), dtype=np.int32)
    for i in range(n_samples):
        out[i] = np.random.RandomState(i).randint(0, n, size=n)
    return out


def _labels_u8(labels, device):
    y = torch.as_tensor(labels).to(device)
    if y.is_floating_point():
        y = torch.round(y)
    return (y != 0).to(torch.uint8).contiguous()


CURVE_KEYS = ('sensitivity', 'specificity', 'threshold', 'pr_auc', 'average_precision')


def _sorted_scores(probs, labels):
    """The part of a metric call that does not depend on the resamples: argument checks, the f32
    scores [N, P] with signed zero canonicalised, the uint8 labels and the ascending order [P, N]
    (one ``torch.sort`` per label) -- made once, walked by both kernels."""
    if probs.ndim != 2:
        raise ValueError(f'evaluate: probs must be a tensor [N, P], got {tuple(probs.shape)} on {probs.device}')
    N, P = probs.shape
    y = _labels_u8(labels, probs.device)
    if tuple(y.shape) != (N, P):
        raise ValueError(f'evaluate: labels {tuple(y.shape)} do not match probs {(N, P)}')
    # + 0.0: -0.0 and 0.0 sort as equal, so they must also be one tie group (groups are bit-equal runs)
    s = (probs.detach().float() + 0.0).contiguous()
    order = torch.sort(s.t(), dim=1).indices.to(torch.int32).contiguous()          # [P, N], ascending
    return s, y, order


def _auroc_host(s, y, rows):
    """``ctclip_auroc_boot``'s count restated in torch for HOST tensors (the linear probe's CPU path and its
    tests; device tensors always take the kernel): per (resample, label) the tie-aware Mann-Whitney count in
    64-bit integers -- pairs (positive above negative) + half the tied pairs, doubled -- and one f64 division;
    NaN for one class only."""
    N, P = s.shape
    S = rows.shape[0]
    mult = torch.zeros(S, N, dtype=torch.int64)
    mult.scatter_add_(1, rows.long(), torch.ones(S, N, dtype=torch.int64))
    out = torch.empty(S, P, dtype=torch.float64)
    for p in range(P):
        _, inv = torch.unique(s[:, p], sorted=True, return_inverse=True)          # tie groups, ascending
        G = int(inv.max()) + 1
        yp = y[:, p].long()
        pos = torch.zeros(S, G, dtype=torch.int64).index_add_(1, inv, mult * yp)
        neg = torch.zeros(S, G, dtype=torch.int64).index_add_(1, inv, mult * (1 - yp))
        below = torch.cumsum(neg, 1) - neg
        u2 = (pos * (2 * below + neg)).sum(1)
        den = 2 * pos.sum(1) * neg.sum(1)
        out[:, p] = torch.where(den > 0, u2.double() / den.clamp(min=1).double(), torch.full((), float('nan'),
                                                                                           dtype=torch.float64))
    return out


def _walk(symbol, width, sorted_scores, rows):
    """``symbol`` (ctclip_auroc_boot / ctclip_curve_boot) on the resamples ``rows`` [S, N] of row
    indices: [S, P] + ``width`` f64."""
    s, y, order = sorted_scores
    N, P = s.shape
    rows = torch.as_tensor(rows).to(device=s.device, dtype=torch.int32).contiguous()
    if rows.ndim != 2 or rows.shape[1] != N:
        raise ValueError(f'evaluate: resample indices must be [S, {N}], got {tuple(rows.shape)}')
    S = rows.shape[0]
    if not s.is_cuda:
        if symbol != 'ctclip_auroc_boot':
            raise ValueError(f'evaluate: {symbol} runs on device tensors only, got scores on {s.device}')
        return _auroc_host(s, y, rows)
    out = torch.empty((S, P) + width, device=s.device, dtype=torch.float64)
    call(symbol, ptr(s), ptr(y), ptr(order), ptr(rows), N, P, S, ptr(out), stream_ptr())
    return out


def _auroc_rows(probs, labels, rows, sorted_scores=None):
    """AUROC [S, P] f64 of the resamples ``rows`` [S, N] (row indices) of probs / labels [N, P]."""
    return _walk('ctclip_auroc_boot', (), sorted_scores or _sorted_scores(probs, labels), rows)


def _curve_rows(probs, labels, rows, sorted_scores=None):
    """``ctclip_curve_boot`` on the resamples ``rows`` [S, N]: a dict of [S, P] f64 per CURVE_KEYS."""
    out = _walk('ctclip_curve_boot', (len(CURVE_KEYS),), sorted_scores or _sorted_scores(probs, labels), rows)
    return {k: out[..., i].contiguous() for i, k in enumerate(CURVE_KEYS)}


def _identity(probs):
    return torch.arange(probs.shape[0], dtype=torch.int32, device=probs.device)[None]


def auroc(probs, labels):
    """Per-label AUROC [P] f64 (evaluate.py:160-207 ``evaluate_internal``); NaN for a label with
    one class only.  probs: device tensor [N, P] (a host tensor takes ``_auroc_host``, the same integer
    count in torch); labels: [N, P] of 0 / 1."""
    return _auroc_rows(probs, labels, _identity(probs))[0]


def bootstrap_auroc(probs, labels, n_samples=1000):
    """[n_samples, P] f64: the AUROCs of the reference's bootstrap resamples (evaluate.py:305-336);
    a resample that draws one class only gives NaN, as ``roc_curve`` + ``auc`` do."""
    return _auroc_rows(probs, labels, bootstrap_indices(probs.shape[0], n_samples))


def curve_metrics(probs, labels):
    """Per label, [P] f64 device tensors under CURVE_KEYS: ``sensitivity`` / ``specificity`` at the
    Youden point of the ROC curve (evaluate.py:104-113 ``choose_operating_point`` over ``roc_curve``:
    the highest-scoring point of maximal tpr - fpr, decided on exact integers; 0 / 0 when no point
    is above the diagonal), the score ``threshold`` that realises it (NaN then), ``pr_auc`` =
    ``auc(recall, precision)`` of ``precision_recall_curve`` (evaluate.py:116-118) and sklearn's
    ``average_precision``.  All NaN for a label with one class only."""
    return {k: v[0] for k, v in _curve_rows(probs, labels, _identity(probs)).items()}


def bootstrap_curve_metrics(probs, labels, n_samples=1000):
    """``curve_metrics`` of the reference's bootstrap resamples (``bootstrap_indices``): the same
    keys, [n_samples, P] f64 each; a scored row a resample did not draw is no curve point."""
    return _curve_rows(probs, labels, bootstrap_indices(probs.shape[0], n_samples))


def compute_cis(boot, confidence_level=0.05):
    """``compute_cis`` (evaluate.py:272-303): [3, P] f64, rows (mean, lower, upper), per label of the
    bootstrap table [S, P]: sorted with NaN last (pandas ``sort_values``), the reference's two
    integer indices (a negative one counts from the end, as ``iloc`` does), the mean skips NaN,
    all rounded to 4 places."""
    b = boot.detach().cpu().numpy() if isinstance(boot, torch.Tensor) else np.asarray(boot)
    b = np.sort(b.astype(np.float64), axis=0)                     # NaN last
    S = b.shape[0]
    lower_index = int(confidence_level / 2 * S) - 1
    upper_index = int((1 - confidence_level / 2) * S) - 1
    cnt = (~np.isnan(b)).sum(0)
    mean = np.where(cnt > 0, np.nansum(b, 0) / np.maximum(cnt, 1), np.nan)
    return torch.from_numpy(np.round(np.stack([mean, b[lower_index], b[upper_index]]), 4))


def _rounded(probs, labels):
    p = torch.as_tensor(probs).detach()
    y = torch.as_tensor(labels).to(p.device)
    p = torch.round(p.double()).long()                            # np.rint: half to even, :434-435
    y = torch.round(y.double()).long()
    return p, y


def micro_f1(probs, labels):
    """``f1_score(rint(labels), rint(probs), average='micro')`` (CTCLIPTrainer.py:437-440)."""
    p, y = _rounded(probs, labels)
    tp = int(((p == 1) & (y == 1)).sum())
    den = int((p == 1).sum()) + int((y == 1).sum())
    return 2 * tp / den if den else 0.0


def flat_accuracy(probs, labels):
    """``accuracy_score`` of the flattened rounded labels / predictions (CTCLIPTrainer.py:441-445)."""
    p, y = _rounded(probs, labels)
    return int((p == y).sum()) / p.numel()


class ZeroShotEvaluator:
    """The trainer's validation pass (CTCLIPTrainer.py:356-454) around a ``ZeroShotClassifier``
    whose prompts are set: ``evaluate`` scores the volumes and reports the reference's numbers."""

    def __init__(self, classifier):
        self.classifier = classifier

    def evaluate(self, volumes, labels, n_boot=0, batch_size=8, curves=False):
        """volumes: an (N, 1, D, H, W) tensor or an iterable of such batches; labels [N, P] of 0 / 1.
        Returns ``probs`` [N, P] f32 (device), ``auroc`` [P] f64 (device), ``ci`` (None, or with
        n_boot > 0 the [3, P] mean / lower / upper table of ``compute_cis`` over n_boot resamples),
        ``f1_micro`` and ``flat_accuracy`` (floats).  With ``curves=True`` also ``curves``
        (``curve_metrics``' dict) and, with n_boot > 0, ``curves_ci``: one ``compute_cis`` table
        [3, P] per metric over the same resamples."""
        zs = self.classifier
        if isinstance(volumes, torch.Tensor):
            probs = zs.predict(volumes, batch_size=batch_size)[0]
        else:
            probs = torch.cat([zs.predict(v, batch_size=batch_size)[0] for v in volumes])
        ss = _sorted_scores(probs, labels)                            # one sort for every table below
        rows = bootstrap_indices(probs.shape[0], n_boot) if n_boot else None
        ci = compute_cis(_auroc_rows(probs, labels, rows, ss)) if n_boot else None
        res = dict(probs=probs, auroc=_auroc_rows(probs, labels, _identity(probs), ss)[0], ci=ci,
                   f1_micro=micro_f1(probs, labels), flat_accuracy=flat_accuracy(probs, labels))
        if curves:
            res['curves'] = {k: v[0] for k, v in _curve_rows(probs, labels, _identity(probs), ss).items()}
            if n_boot:
                res['curves_ci'] = {k: compute_cis(v) for k, v in _curve_rows(probs, labels, rows, ss).items()}
        return res


__all__ = ['bootstrap_indices', 'auroc', 'bootstrap_auroc', 'curve_metrics', 'bootstrap_curve_metrics', 'compute_cis',
           'micro_f1', 'flat_accuracy', 'ZeroShotEvaluator', 'MAX_ROWS', 'CURVE_KEYS']
