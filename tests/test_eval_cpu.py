"""Host side of the zero-shot validation loop (ct_clip/CTCLIPTrainer.py:356-454,
ct_clip/evaluate.py:160-207,272-337, ct_clip/data_inference.py:78-122) against fixtures made by the
reference's own code (tests/golden/make_golden_eval.py): the bootstrap resamples, compute_cis,
micro-F1 / flat accuracy, the validation prompts and the evaluation loader's crop / pad geometry.

``auroc_table`` below restates the tie-aware AUROC in numpy, in exact integers up to one division:
it is checked against sklearn's numbers here (1e-12: sklearn's f64 trapezoid is within O(N 2^-53) of
the exact ratio) and is the GPU tests' reference on shapes the fixture does not hold."""
import os

import numpy as np
import pytest
import torch
from safetensors.torch import load_file

G = load_file(os.path.join(os.path.dirname(__file__), 'golden', 'golden_eval.safetensors'))
LOADER_CASES = ['vol0_float32', 'vol0_float64', 'vol1_float32', 'vol2_float32', 'vol3_float32', 'vol3_float64']
TARGET = (480, 480, 240)          # (h, w, d), data_inference.py:90


def auroc_1(scores, labels, mult=None):
    """Tie-aware Mann-Whitney AUROC of one label: sum_g pos_g (2 neg_below_g + neg_g) / (2 Pos Neg)
    over groups g of equal scores, rows weighted by ``mult``; NaN when one class is absent."""
    scores, labels = np.asarray(scores), np.asarray(labels).astype(np.int64)
    mult = np.ones(len(scores), dtype=np.int64) if mult is None else np.asarray(mult).astype(np.int64)
    order = np.argsort(scores, kind='stable')
    s, pos, neg = scores[order], (labels * mult)[order], ((1 - labels) * mult)[order]
    starts = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]]))
    pos_g, neg_g = np.add.reduceat(pos, starts), np.add.reduceat(neg, starts)
    below = np.cumsum(neg_g) - neg_g
    count = int((pos_g * (2 * below + neg_g)).sum())
    den = 2 * int(pos.sum()) * int(neg.sum())
    return count / den if den else float('nan')


def auroc_table(probs, labels, rows):
    """[S, P] f64: ``auroc_1`` of every label on every resample ``rows`` [S, N] of row indices."""
    probs, labels, rows = np.asarray(probs), np.asarray(labels), np.asarray(rows)
    N, P = probs.shape
    out = np.empty((rows.shape[0], P), dtype=np.float64)
    for i, r in enumerate(rows):
        mult = np.bincount(r, minlength=N)
        for j in range(P):
            out[i, j] = auroc_1(probs[:, j], labels[:, j], mult)
    return out


def same_with_nan(a, b, tol=0.0):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    m = ~np.isnan(a)
    return bool((np.abs(a[m] - b[m]) <= tol).all())


def test_bootstrap_indices_are_the_reference_resamples():
    from ctclip_mi355x.evaluate import bootstrap_indices
    ref = G['met.indices'].numpy()
    got = bootstrap_indices(ref.shape[1], ref.shape[0])
    assert got.dtype == np.int32 and np.array_equal(got, ref)


def test_restatement_matches_sklearn():
    probs, labels = G['met.probs'].numpy(), G['met.labels'].numpy()
    boot = auroc_table(probs, labels, G['met.indices'].numpy())
    ref = G['met.boot_auroc'].numpy()
    assert np.isnan(ref).any()                       # the one-class resamples are in the fixture
    assert same_with_nan(boot, ref, 1e-12)
    point = auroc_table(probs, labels, np.arange(len(probs))[None])[0]
    assert same_with_nan(point, G['met.auroc'].numpy(), 1e-12)
    assert point[2] == 1.0 and point[3] == 0.0       # separated / inverted labels


def test_compute_cis_matches_reference():
    from ctclip_mi355x.evaluate import compute_cis
    cis = compute_cis(G['met.boot_auroc'])
    assert cis.shape == (3, 5) and cis.dtype == torch.float64
    assert same_with_nan(cis.numpy(), G['met.cis'].numpy())
    assert same_with_nan(compute_cis(G['met.boot_auroc'].numpy()).numpy(), G['met.cis'].numpy())


def test_f1_and_accuracy_match_reference():
    from ctclip_mi355x.evaluate import micro_f1, flat_accuracy
    probs, labels = G['met.probs'], G['met.labels']
    assert micro_f1(probs, labels) == G['met.f1_micro'].item()
    assert flat_accuracy(probs, labels) == G['met.flat_accuracy'].item()
    assert micro_f1(torch.zeros(4, 2), torch.zeros(4, 2)) == 0.0        # nothing positive: sklearn gives 0


def test_validation_prompts():
    from ctclip_mi355x.zero_shot import (prompts, PATHOLOGIES, VALIDATION_PATHOLOGIES, VALIDATION_TEMPLATE)
    assert prompts(['Cardiomegaly']) == ['Cardiomegaly is present.', 'Cardiomegaly is not present.']
    assert prompts()[:2] == ['Medical material is present.', 'Medical material is not present.']
    assert len(prompts()) == 36
    v = prompts(VALIDATION_PATHOLOGIES, template=VALIDATION_TEMPLATE)
    assert len(v) == 36
    assert v[:2] == ['There is Medical material.', 'There is no Medical material.']
    assert v[22:24] == ['There is Pulmonary fibrotic sequela.', 'There is no Pulmonary fibrotic sequela.']
    diff = [i for i, (a, b) in enumerate(zip(PATHOLOGIES, VALIDATION_PATHOLOGIES)) if a != b]
    assert diff == [11] and PATHOLOGIES[11] == 'Pulmonary Embolism'


@pytest.mark.parametrize('name', LOADER_CASES)
def test_loader_geometry_matches_reference(name):
    from ctclip_mi355x.preprocess import crop_pad
    a0, a1, a2 = G[f'{name}.scan'].shape            # read as (h, w, d) = (a1, a2, a0)
    lo, ext = G[f'{name}.box_lo'].tolist(), G[f'{name}.box'].shape
    th, tw, td = TARGET
    for n, t, l0, e in zip((a0, a1, a2), (td, th, tw), lo, ext):        # box axes are (d, h, w)
        start, pad = crop_pad(n, t)
        assert pad == l0 and min(n - start, t) == e


def test_loader_rejects_other_dtypes():
    from ctclip_mi355x.preprocess import eval_volume_to_tensor
    with pytest.raises(ValueError):
        eval_volume_to_tensor(torch.zeros(3, 4, 5, dtype=torch.int16))
    with pytest.raises(ValueError):
        eval_volume_to_tensor(torch.zeros(4, 5))
