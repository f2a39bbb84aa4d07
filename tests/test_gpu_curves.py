"""ctclip_curve_boot on the GPU: operating point, threshold, PR-AUC and average precision of
(resample, label) pairs, against the numpy restatement ``test_curves_cpu.curve_table`` and the
reference's fixture, then through ZeroShotEvaluator and CTClipTrainer.validate.

sensitivity, specificity and threshold are decided on integers and divided once: bit-equal.  The two
PR sums are f64 sums of at most N terms in another order than numpy's: 2 (N + 4) 2^-53
(``test_curves_cpu.pr_tol``)."""
import numpy as np
import pytest
import torch

from test_curves_cpu import C, KEYS, N_TABLES, curve_table, pr_tol, same_bits
from test_gpu_eval import _case, tiny  # noqa: F401  (tiny: the module-scoped model fixture)

pytestmark = pytest.mark.gpu


def _kernel(probs, labels, rows):
    """[S, P, 5] f64 from ctclip_curve_boot through evaluate._curve_rows."""
    from ctclip_mi355x.evaluate import _curve_rows
    out = _curve_rows(torch.as_tensor(probs).cuda(), torch.as_tensor(labels), rows)
    torch.cuda.synchronize()
    assert tuple(out) == KEYS
    return np.stack([out[k].cpu().numpy() for k in KEYS], axis=-1)


def _check(got, ref, N):
    assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref))
    assert same_bits(got[..., :3], ref[..., :3])
    err = np.nan_to_num(np.abs(got[..., 3:] - ref[..., 3:])).max()
    print(f'N = {N}: max |pr_auc, ap - restatement| = {err:.3e}, bound {pr_tol(N):.3e}')
    assert err <= pr_tol(N)


# N: as test_gpu_eval.test_auroc_matches_restatement
@pytest.mark.parametrize('N', [1, 2, 63, 64, 65, 300, 2048, 2049])
def test_curves_match_restatement(N):
    probs, labels, rows = _case(N, 3, 5, seed=N, levels=8)
    _check(_kernel(probs, labels, rows), curve_table(probs, labels, rows), N)
    probs, labels, rows = _case(N, 3, 5, seed=N + 1)          # continuous scores: (almost) no ties
    _check(_kernel(probs, labels, rows), curve_table(probs, labels, rows), N)


def test_curves_largest_size_with_ties():
    probs, labels, rows = _case(8192, 2, 3, seed=5, levels=7)
    assert len(np.unique(probs)) == 7
    got = _kernel(probs, labels, rows)
    _check(got, curve_table(probs, labels, rows), 8192)
    assert not np.isnan(got[..., [0, 1, 3, 4]]).any()


def test_undrawn_top_group_is_no_point():
    N = 70
    g = np.random.default_rng(3)
    probs = (g.integers(0, 6, (N, 2)) / 8).astype(np.float32)
    probs[:3] = 0.875                                         # the highest group: rows 0..2, all negative
    labels = (g.random((N, 2)) < 0.5).astype(np.uint8)
    labels[:3] = 0
    rows = g.integers(3, N, (2, N)).astype(np.int32)          # never drawn
    got = _kernel(probs, labels, rows)
    _check(got, curve_table(probs, labels, rows), N)
    thr = got[..., 2]
    assert (thr[~np.isnan(thr)] < 0.875).all()
    for s in range(2):
        for p in range(2):
            assert np.isnan(thr[s, p]) or thr[s, p] in probs[rows[s], p]


def test_flat_scores_give_one_point():
    N = 257
    probs, labels, rows = _case(N, 3, 4, seed=9)
    flat = np.full_like(probs, 0.5)
    got = _kernel(flat, labels, rows)
    assert (got[..., :2] == 0.0).all() and np.isnan(got[..., 2]).all()
    for s in range(4):
        prev = labels[rows[s]].sum(0) / N                    # prevalence in the resample
        assert np.abs(got[s, :, 3] - (1 + prev) / 2).max() <= pr_tol(N)
        assert np.abs(got[s, :, 4] - prev).max() <= pr_tol(N)
    _check(got, curve_table(flat, labels, rows), N)


def test_separated_and_inverted_labels():
    N = 300
    g = np.random.default_rng(11)
    y = (g.random(N) < 0.3).astype(np.uint8)
    hi, lo = g.integers(9, 17, N) / 16, g.integers(0, 8, N) / 16
    probs = np.stack([np.where(y == 1, hi, lo), np.where(y == 1, lo, hi)], 1).astype(np.float32)
    labels = np.stack([y, y], 1)
    rows = g.integers(0, N, (3, N)).astype(np.int32)
    rows[0] = np.arange(N)
    got = _kernel(probs, labels, rows)
    _check(got, curve_table(probs, labels, rows), N)
    assert (got[:, 0, :2] == 1.0).all() and (got[:, 0, 3:] == 1.0).all()          # separated
    assert got[0, 0, 2] == probs[y == 1, 0].min()                                 # the lowest positive score
    assert (got[:, 1, :2] == 0.0).all() and np.isnan(got[:, 1, 2]).all()          # inverted: no point above the diagonal


def test_highest_score_wins_among_equal_j():
    # Pos = Neg = 4; points (descending): 0.9 -> (tp 1, fp 0), 0.8 -> (1, 1), 0.7 -> (2, 1), 0.6 -> (2, 2), 0.5 -> (3, 2),
    # 0.1 -> (4, 4): J = 4 (tp - fp) is 4 at 0.9, 0.7 and 0.5
    probs = np.array([.9, .8, .7, .6, .5, .1, .1, .1], dtype=np.float32)[:, None]
    labels = np.array([1, 0, 1, 0, 1, 1, 0, 0], dtype=np.uint8)[:, None]
    rows = np.stack([np.arange(8), np.arange(8)[::-1]]).astype(np.int32)
    got = _kernel(probs, labels, rows)
    _check(got, curve_table(probs, labels, rows), 8)
    assert (got[:, 0, 0] == 0.25).all() and (got[:, 0, 1] == 1.0).all() and (got[:, 0, 2] == np.float32(.9)).all()


def test_one_class_and_one_row_are_nan():
    N = 257
    probs, labels, rows = _case(N, 3, 4, seed=9)
    one = np.full((2, N), 17, dtype=np.int32)                 # one row drawn N times: one class
    one[1] = N - 1
    assert np.isnan(_kernel(probs, labels, one)).all()
    probs, labels, rows = _case(1, 3, 4, seed=0)
    assert np.isnan(_kernel(probs, labels, rows)).all()


def test_signed_zeros_are_one_group():
    probs = np.array([0.0, -0.0, -1.0, 1.0, -0.0, 0.0], dtype=np.float32)[:, None]
    labels = np.array([1, 0, 0, 1, 1, 0], dtype=np.uint8)[:, None]
    rows = np.arange(6, dtype=np.int32)[None]
    got = _kernel(probs, labels, rows)
    _check(got, curve_table(probs, labels, rows), 6)
    # points: 1.0 -> (1, 0), {+-0.0} -> (3, 2), -1.0 -> (3, 3); J = 3 tp - 3 fp = 3 at both of the first two
    assert got[0, 0, :3].tolist() == [1 / 3, 1.0, 1.0]


def test_fixture_point_estimates():
    from ctclip_mi355x.evaluate import curve_metrics
    for c in range(N_TABLES):
        x, y = C[f'c{c}.probs'], C[f'c{c}.labels']
        res = curve_metrics(x.cuda(), y)
        assert tuple(res) == KEYS and all(v.shape == (4,) and v.dtype == torch.float64 and v.is_cuda for v in res.values())
        got = np.stack([res[k].cpu().numpy() for k in KEYS], -1)
        ref = C[f'c{c}.point'].numpy()
        assert same_bits(got[:, :3], ref[:, :3])
        err = np.abs(got[:, 3:] - ref[:, 3:]).max()
        print(f'table {c}: max |pr_auc, ap - sklearn| = {err:.3e}, bound {pr_tol(len(x)):.3e}')
        assert err <= pr_tol(len(x))


def test_fixture_resamples():
    from ctclip_mi355x.evaluate import bootstrap_curve_metrics
    for c in range(N_TABLES):
        x, y = C[f'c{c}.probs'], C[f'c{c}.labels']
        res = bootstrap_curve_metrics(x.cuda(), y, n_samples=64)
        got = np.stack([res[k].cpu().numpy() for k in KEYS], -1)
        assert got.shape == (64, 4, 5)
        _check(got, curve_table(x.numpy(), y.numpy(), C[f'c{c}.indices'].numpy()), len(x))
        assert np.abs(got[..., 3:] - C[f'c{c}.boot'].numpy()[..., 3:]).max() <= pr_tol(len(x))


def test_curves_are_reproducible():
    probs, labels, rows = _case(1500, 4, 16, seed=3, levels=16)
    a, b = _kernel(probs, labels, rows), _kernel(probs, labels, rows)
    assert np.array_equal(a.view(np.int64), b.view(np.int64))


def test_curves_reject_more_than_8192_rows():
    from ctclip_mi355x._lib import KernelError
    probs, labels, rows = _case(8193, 1, 1, seed=1)
    with pytest.raises(KernelError, match='1003'):            # CT_ESHAPE
        _kernel(probs, labels, rows)


# --------------------------------------------------------------------------- evaluator and trainer
def test_evaluator_curves(tiny):  # noqa: F811
    from ctclip_mi355x.evaluate import ZeroShotEvaluator
    cfg, model, zs, video, labels = tiny
    ev = ZeroShotEvaluator(zs)
    res = ev.evaluate(video, labels, n_boot=8, batch_size=2, curves=True)
    probs = res['probs'].cpu().numpy()
    ref = curve_table(probs, labels.numpy(), np.arange(4)[None])[0]
    got = np.stack([res['curves'][k].cpu().numpy() for k in KEYS], -1)
    _check(got, ref, 4)
    assert tuple(res['curves_ci']) == KEYS
    assert all(t.shape == (3, 3) and t.dtype == torch.float64 for t in res['curves_ci'].values())
    plain = ev.evaluate(video, labels, n_boot=8, batch_size=2)
    assert set(plain) == {'probs', 'auroc', 'ci', 'f1_micro', 'flat_accuracy'}             # exactly today's keys
    assert torch.equal(plain['auroc'], res['auroc']) and same_bits(plain['ci'].numpy(), res['ci'].numpy())
    assert 'curves_ci' not in ev.evaluate(video, labels, batch_size=2, curves=True)


def test_validate_with_curves_owns_its_status_bits(tiny):  # noqa: F811
    import types
    from oracle import weights as W
    from ctclip_mi355x import kernels as K
    from ctclip_mi355x.trainer import CTClipTrainer, EvalGuardError
    cfg, model, zs, video, labels = tiny
    ids, mask = W.make_text(2, 32, cfg.bert.vocab_size, ragged=True)
    text = types.SimpleNamespace(input_ids=ids.cuda(), attention_mask=mask.cuda())
    K.reset_ln_status()
    tr = CTClipTrainer(model, lr=1e-3)
    tr.train_step(text, video[:2])
    tr.check()
    word = K.status_word(video.device)
    snap = word.clone()
    res = tr.validate(video, labels, classifier=zs, curves=True)
    assert tuple(res['curves']) == KEYS and 'curves_ci' not in res
    ref = curve_table(res['probs'].cpu().numpy(), labels.numpy(), np.arange(4)[None])[0]
    _check(np.stack([res['curves'][k].cpu().numpy() for k in KEYS], -1), ref, 4)
    assert model.training and torch.equal(word, snap)
    bad = video[:2].clone()
    bad[1, 0, 17, 33, 71] = float('nan')
    with pytest.raises(EvalGuardError) as ei:
        tr.validate(bad, labels[:2], curves=True)
    assert ei.value.bits != 0 and torch.equal(word, snap) and model.training
    before = tr.flat.data.clone()
    loss = tr.train_step(text, video[:2])
    tr.check()                                                # not blamed for the validation's bits
    assert torch.isfinite(loss) and not torch.equal(before, tr.flat.data)
