"""The operating point and the precision-recall sums (ct_clip/evaluate.py:104-118) restated in numpy,
against the fixture the reference's own code and its sklearn wrote
(tests/golden/make_golden_curves.py).

``curve_table`` follows the definitions of ctclip_curve_boot (include/ctclip_hip.h): a point is a
group of equal scores with weight > 0 in the resample, the operating point is decided on the exact
integer J = tp Neg - fp Pos, first maximiser in descending score order, reported only if J > 0.  It
is the GPU tests' reference on shapes the fixture does not hold.

Tolerance of the two PR sums: each has at most N non-zero terms that total at most 1, a term takes
at most four roundings and every accumulation adds one, on the fixture's side as on ours:
2 (N + 4) 2^-53."""
import os

import numpy as np
from safetensors.torch import load_file

C = load_file(os.path.join(os.path.dirname(__file__), 'golden', 'golden_curves.safetensors'))
KEYS = ('sensitivity', 'specificity', 'threshold', 'pr_auc', 'average_precision')
N_TABLES = 4


def pr_tol(N):
    return 2 * (N + 4) * 2.0 ** -53


def curve_points(scores, labels, mult):
    """The points of one label in descending score order: (score, tp, fp) cumulative down to and
    including each point, and the class totals.  Groups of weight 0 are dropped."""
    scores = np.asarray(scores) + np.float32(0.0)                      # -0.0 and 0.0: one group
    labels, mult = np.asarray(labels).astype(np.int64), np.asarray(mult).astype(np.int64)
    order = np.argsort(-scores.astype(np.float64), kind='stable')
    s, pos, neg = scores[order], (labels * mult)[order], ((1 - labels) * mult)[order]
    starts = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]]))
    pos_g, neg_g = np.add.reduceat(pos, starts), np.add.reduceat(neg, starts)
    keep = pos_g + neg_g > 0
    return s[starts][keep], np.cumsum(pos_g[keep]), np.cumsum(neg_g[keep]), int(pos.sum()), int(neg.sum())


def curve_1(scores, labels, mult=None):
    """[5] f64 of one label: sensitivity, specificity, threshold, pr_auc, average_precision."""
    mult = np.ones(len(scores), dtype=np.int64) if mult is None else mult
    thr, tp, fp, Pos, Neg = curve_points(scores, labels, mult)
    if Pos == 0 or Neg == 0:
        return np.full(5, np.nan)
    J = tp * Neg - fp * Pos                                            # int64, exact
    k = int(np.argmax(J))                                              # the first maximiser
    if J[k] > 0:
        op = [float(tp[k]) / Pos, 1.0 - float(fp[k]) / Neg, float(thr[k])]
    else:
        op = [0.0, 0.0, np.nan]
    precision = np.concatenate([[1.0], tp / (tp + fp).astype(np.float64)])
    width = np.diff(np.concatenate([[0], tp])) / float(Pos)            # recall_k - recall_{k-1}, one rounding
    pr_auc = float(np.sum(width * ((precision[1:] + precision[:-1]) * 0.5)))
    ap = float(np.sum(width * precision[1:]))
    return np.array(op + [pr_auc, ap])


def curve_table(probs, labels, rows):
    """[S, P, 5] f64: ``curve_1`` of every label on every resample ``rows`` [S, N] of row indices."""
    probs, labels, rows = np.asarray(probs), np.asarray(labels), np.asarray(rows)
    N, P = probs.shape
    out = np.empty((rows.shape[0], P, 5), dtype=np.float64)
    for i, r in enumerate(rows):
        mult = np.bincount(r, minlength=N)
        for j in range(P):
            out[i, j] = curve_1(probs[:, j], labels[:, j], mult)
    return out


def same_bits(a, b):
    """Equal as f64 bit patterns up to the NaN payload (NaN only where the other is NaN)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def test_fixture_holds_the_cases():
    assert C['sklearn_version'].tolist() == [1, 7, 2]
    assert C['counts'].tolist() == [[64, 128], [128, 64], [32, 32], [16, 256]]
    assert C['levels'].tolist() == [4, 16, 64, 0]
    for c in range(N_TABLES):
        pos, neg = C['counts'][c].tolist()
        y, x = C[f'c{c}.labels'].numpy(), C[f'c{c}.probs'].numpy()
        assert y.shape == (pos + neg, 4) and (y.sum(0) == pos).all()
        assert [len(np.unique(x[:, j])) <= lv for j, lv in enumerate((4, 16, 64))] == [True] * 3
        assert C[f'c{c}.indices'].shape == (64, pos + neg) and C[f'c{c}.boot'].shape == (64, 4, 5)


def test_bootstrap_indices_are_the_fixture_resamples():
    from ctclip_mi355x.evaluate import bootstrap_indices
    for c in range(N_TABLES):
        ref = C[f'c{c}.indices'].numpy()
        assert np.array_equal(bootstrap_indices(ref.shape[1], ref.shape[0]), ref)


def test_point_estimates_match_reference():
    for c in range(N_TABLES):
        x, y = C[f'c{c}.probs'].numpy(), C[f'c{c}.labels'].numpy()
        N = len(x)
        got = curve_table(x, y, np.arange(N)[None])[0]
        ref = C[f'c{c}.point'].numpy()
        assert same_bits(got[:, :3], ref[:, :3]), (c, got[:, :3], ref[:, :3])       # the operating point: bit-equal
        err = np.abs(got[:, 3:] - ref[:, 3:]).max()
        print(f'table {c}: N = {N}, max |pr_auc, ap - sklearn| = {err:.3e}, bound {pr_tol(N):.3e}')
        assert err <= pr_tol(N)


def test_resampled_pr_sums_match_reference():
    for c in range(N_TABLES):
        x, y, rows = C[f'c{c}.probs'].numpy(), C[f'c{c}.labels'].numpy(), C[f'c{c}.indices'].numpy()
        N = len(x)
        got = curve_table(x, y, rows)
        ref = C[f'c{c}.boot'].numpy()
        err = np.abs(got[..., 3:] - ref[..., 3:]).max()
        print(f'table {c}: N = {N}, 64 resamples, max |pr_auc, ap - sklearn| = {err:.3e}, bound {pr_tol(N):.3e}')
        assert err <= pr_tol(N)


def test_resampled_operating_points_differ_only_on_exact_ties():
    """Resampled class counts are arbitrary, so tpr and fpr are rounded and the reference's f64
    ``tpr - fpr > J`` can break an exact tie between two points either way.  Wherever its operating
    point is not ours, its point must have OUR integer J: the same Youden index, another maximiser."""
    differ = total = 0
    for c in range(N_TABLES):
        x, y, rows = C[f'c{c}.probs'].numpy(), C[f'c{c}.labels'].numpy(), C[f'c{c}.indices'].numpy()
        got, ref = curve_table(x, y, rows), C[f'c{c}.boot'].numpy()
        for i, r in enumerate(rows):
            mult = np.bincount(r, minlength=len(x))
            for j in range(x.shape[1]):
                total += 1
                if same_bits(got[i, j, :3], ref[i, j, :3]):
                    continue
                differ += 1
                thr, tp, fp, Pos, Neg = curve_points(x[:, j], y[:, j], mult)
                J = tp * Neg - fp * Pos
                k = np.flatnonzero(thr == np.float32(ref[i, j, 2]))
                assert len(k) == 1, 'the reference threshold is not one of our points'
                assert J[k[0]] == J.max() > 0
                assert ref[i, j, 0] == tp[k[0]] / Pos and ref[i, j, 1] == 1 - fp[k[0]] / Neg
    print(f'{differ} of {total} resampled operating points differ from the reference, all exact ties in J')


def test_restatement_corners():
    y = np.array([1, 0, 1, 0, 0, 1], dtype=np.uint8)
    flat = curve_1(np.full(6, 0.25, dtype=np.float32), y)               # one point, J = 0
    assert flat[0] == 0.0 and flat[1] == 0.0 and np.isnan(flat[2]) and flat[3] == (1 + 0.5) / 2 and flat[4] == 0.5
    sep = curve_1(np.array([.9, .1, .8, .2, .3, .7], dtype=np.float32), y)
    assert sep[:2].tolist() == [1.0, 1.0] and sep[2] == np.float32(.7) and sep[3] == 1.0 and sep[4] == 1.0
    inv = curve_1(np.array([.1, .9, .2, .8, .7, .3], dtype=np.float32), y)
    assert inv[:2].tolist() == [0.0, 0.0] and np.isnan(inv[2])
    # the highest score is never drawn: it is no point, and no threshold
    x = np.array([.99, .5, .6, .4, .3, .2], dtype=np.float32)
    got = curve_1(x, np.array([0, 1, 1, 0, 0, 0]), np.array([0, 2, 1, 1, 1, 1]))
    assert got[:2].tolist() == [1.0, 1.0] and got[2] == np.float32(.5) and got[3] == 1.0
    assert np.isnan(curve_1(x, np.ones(6, dtype=np.uint8))).all()       # one class
    z = curve_1(np.array([0.0, -0.0, -1.0, 1.0], dtype=np.float32), np.array([1, 0, 0, 1]))
    assert z[:3].tolist() == [0.5, 1.0, 1.0]                            # {0.0, -0.0}: one group, a tie
