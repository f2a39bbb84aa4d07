"""The linear probe on the host: ``probe.step_reference`` (the torch restatement of ctclip_probe_step and the
oracle of tests/test_gpu_probe.py) against torch autograd of ``F.binary_cross_entropy_with_logits`` in
float64, ``LinearProbe.fit`` on a separable problem, and the evaluator's result layout.

step_reference and autograd compute the same sums in float64 in different orders: a few hundred terms of
magnitude O(1), so 1e-12 relative (norm-wise) leaves four digits of slack over 2^-53 * terms."""
import pytest
import torch
import torch.nn.functional as F

from ctclip_mi355x import evaluate as E
from ctclip_mi355x import probe as PR

F64 = torch.float64


def _case(N, D, P, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(N, D, generator=g, dtype=F64)
    W = torch.randn(P, D, generator=g, dtype=F64) * scale
    b = torch.randn(P, generator=g, dtype=F64)
    Y = (torch.rand(N, P, generator=g) < 0.4).to(torch.uint8)
    pw = torch.rand(P, generator=g, dtype=F64) * 3 + 0.25
    return X, W, b, Y, pw


def _autograd(X, W, b, Y, pw, idx=None):
    """torch's loss and gradient over the counted entries of the rows idx (masked before the call)."""
    W, b = W.clone().requires_grad_(), b.clone().requires_grad_()
    if idx is not None:
        X, Y = X[idx.long()], Y[idx.long()]
    Z = X @ W.t() + b
    keep = Y != 255
    pwf = None if pw is None else pw.expand_as(Z)[keep]
    loss = F.binary_cross_entropy_with_logits(Z[keep], Y[keep].to(F64), pos_weight=pwf, reduction='mean')
    loss.backward()
    return loss.detach(), W.grad, b.grad


def _rel(a, b):
    return float((a - b).norm() / b.norm().clamp(min=1e-300))


def _check(res, ref):
    loss, dW, db = ref
    assert abs(float(res['loss']) - float(loss)) <= 1e-12 * max(1.0, abs(float(loss)))
    assert _rel(res['dW'], dW) <= 1e-12 and _rel(res['db'], db) <= 1e-12


@pytest.mark.parametrize('with_pw', [False, True])
def test_step_reference_matches_autograd(with_pw):
    X, W, b, Y, pw = _case(57, 32, 5, seed=1)
    pw = pw if with_pw else None
    res = PR.step_reference(X, W, b, Y, pos_weight=pw)
    assert int(res['count']) == 57 * 5
    _check(res, _autograd(X, W, b, Y, pw))
    # 255s: both sides on the same subset
    Y2 = Y.clone()
    Y2[torch.rand(57, 5, generator=torch.Generator().manual_seed(2)) < 0.3] = 255
    Y2[7] = 255                                                     # a row with nothing counted
    res = PR.step_reference(X, W, b, Y2, pos_weight=pw)
    assert int(res['count']) == int((Y2 != 255).sum())
    _check(res, _autograd(X, W, b, Y2, pw))
    # rows through idx: repeats, out of order
    idx = torch.tensor([5, 3, 3, 56, 0, 5, 41], dtype=torch.int32)
    res = PR.step_reference(X, W, b, Y2, idx=idx, pos_weight=pw)
    assert res['Z'].shape == (7, 5)
    _check(res, _autograd(X, W, b, Y2, pw, idx=idx))


def test_step_reference_extreme_logits_are_finite():
    X, W, b, Y, pw = _case(40, 16, 3, seed=3)
    X = X / X.norm(dim=1, keepdim=True)
    W = 80.0 * torch.sign(torch.randn(3, 1, dtype=F64, generator=torch.Generator().manual_seed(4))) * X[0]
    b = torch.zeros(3, dtype=F64)
    res = PR.step_reference(X, W, b, Y, pos_weight=pw)
    assert float(res['Z'].abs().max()) >= 80.0 - 1e-9
    assert all(bool(torch.isfinite(res[k]).all()) for k in ('loss', 'dW', 'db'))
    _check(res, _autograd(X, W, b, Y, pw))
    f32 = PR.step_reference(X.float(), W.float(), b.float(), Y, pos_weight=pw.float())
    assert all(bool(torch.isfinite(f32[k]).all()) for k in ('loss', 'dW', 'db'))


def test_uncounted_entries_contribute_nothing():
    X, W, b, Y, pw = _case(33, 16, 4, seed=5)
    Y[:, 2] = 255                                                   # an all-255 column
    res = PR.step_reference(X, W, b, Y, pos_weight=pw)
    keep = [0, 1, 3]
    sub = PR.step_reference(X, W[keep], b[keep], Y[:, keep].contiguous(), pos_weight=pw[keep])
    assert int(res['count']) == 33 * 3 == int(sub['count'])
    assert torch.equal(res['dW'][2], torch.zeros(16, dtype=F64)) and float(res['db'][2]) == 0.0
    assert abs(float(res['loss']) - float(sub['loss'])) <= 1e-12 * max(1.0, abs(float(sub['loss'])))
    assert _rel(res['dW'][keep], sub['dW']) <= 1e-12 and _rel(res['db'][keep], sub['db']) <= 1e-12
    # nothing counted at all: loss 0, zero gradients, no NaN
    res = PR.step_reference(X, W, b, torch.full_like(Y, 255), pos_weight=pw)
    assert int(res['count']) == 0 and float(res['loss']) == 0.0
    assert not res['dW'].any() and not res['db'].any()


def _separable(dtype=F64):
    g = torch.Generator().manual_seed(11)
    X = torch.randn(200, 64, generator=g, dtype=F64)
    Y = (X @ torch.randn(64, 3, generator=g, dtype=F64) > 0).to(torch.uint8)
    return X.to(dtype), Y


def test_fit_lowers_the_loss_and_separates():
    X, Y = _separable()
    pr = PR.LinearProbe(64, 3, dtype=F64)
    assert not pr.weight.any() and not pr.bias.any() and set(pr.state_dict()) == {'weight', 'bias'}
    head = pr.fit(X, Y, steps=20, lr=1e-2)
    assert head.shape == (20,) and abs(float(head[0]) - 0.6931471805599453) < 1e-12          # zero init: log 2
    assert bool((head[1:] < head[:-1]).all()), head
    pr.fit(X, Y, steps=480, lr=1e-2)
    auc = E.auroc(pr.predict_proba(X), Y)
    assert auc.dtype == F64 and bool((auc == 1.0).all()), auc
    assert torch.equal(pr.predict_proba(X), torch.sigmoid(pr(X)))


def test_fit_options():
    X, Y = _separable()
    # AdamW decays the weight only: with a gradient-free problem (nothing counted) the bias must not move
    pr = PR.LinearProbe(64, 3, dtype=F64)
    with torch.no_grad():
        pr.weight.fill_(1.0)
        pr.bias.fill_(1.0)
    pr.fit(X, torch.full_like(Y, 255), steps=3, lr=1e-2, wd=0.1)
    assert torch.equal(pr.bias.detach(), torch.ones(3, dtype=F64))
    assert torch.allclose(pr.weight.detach(), torch.full((3, 64), (1 - 1e-3) ** 3, dtype=F64), rtol=1e-12)
    # 'balanced': n_neg / n_pos over the counted rows, 1 for a label with one class only
    Y2 = Y.clone()
    Y2[:, 1] = 0
    Y2[:50, 0] = 255
    pw = PR.balanced_pos_weight(Y2, dtype=F64)
    n1, n0 = int((Y2[:, 0] == 1).sum()), int((Y2[:, 0] == 0).sum())
    assert float(pw[0]) == n0 / n1 and float(pw[1]) == 1.0
    rows = torch.arange(0, 200, 2)
    a = PR.LinearProbe(64, 3, dtype=F64)
    la = a.fit(X, Y2, steps=5, pos_weight='balanced', rows=rows)
    b = PR.LinearProbe(64, 3, dtype=F64)
    lb = b.fit(X[rows], Y2[rows], steps=5, pos_weight=PR.balanced_pos_weight(Y2[rows], dtype=F64))
    assert torch.equal(la, lb) and torch.equal(a.weight, b.weight)
    with pytest.raises(PR.NonFiniteLossError):
        PR.LinearProbe(64, 3, dtype=F64).fit(X * float('nan'), Y, steps=2)
    with pytest.raises(ValueError):
        PR.LinearProbe(64, 3, dtype=F64).fit(X, Y[:, :2], steps=2)


def test_host_auroc_counts_ties_and_resamples():
    s = torch.tensor([[0.1], [0.4], [0.4], [0.8], [0.4]])
    y = torch.tensor([[0], [0], [1], [1], [1]], dtype=torch.uint8)
    # pairs (pos, neg): 0.4>0.1, 0.4=0.4 (half), 0.8>0.1, 0.8>0.4, 0.4>0.1, 0.4=0.4 (half) -> 5 / 6
    assert float(E.auroc(s, y)[0]) == 5 / 6
    rows = torch.tensor([[0, 0, 3, 3, 3], [2, 3, 4, 2, 2]])
    out = E._auroc_rows(s, y, rows)
    assert float(out[0, 0]) == 1.0 and bool(torch.isnan(out[1, 0]))


def test_evaluator_layout_matches_zero_shot():
    X, Y = _separable(torch.float32)

    class Stub:                                                     # a classifier with fixed scores
        @staticmethod
        def predict(v, batch_size=8):
            return torch.sigmoid(v[:, :3]), None
    ref = E.ZeroShotEvaluator(Stub).evaluate(X, Y)

    class Encoder(PR.LinearProbeEvaluator):                         # a stub encoder: "volumes" are [N, 1, 64]
        def encode(self, volumes, batch_size=8):
            return volumes[:, 0].contiguous()
    ev = Encoder(model=None, pathologies=('a', 'b', 'c'))
    with pytest.raises(RuntimeError):
        ev.evaluate(X, Y)
    loss = ev.fit(X[:, None], Y, steps=30)
    res = ev.evaluate(X[:, None], Y)
    assert loss.shape == (30,) and list(res) == list(ref)
    assert list(res) == ['probs', 'auroc', 'ci', 'f1_micro', 'flat_accuracy']
    for k in res:
        assert type(res[k]) is type(ref[k]), k
    assert res['probs'].shape == ref['probs'].shape and res['auroc'].shape == ref['auroc'].shape == (3,)
    assert res['auroc'].dtype == ref['auroc'].dtype and res['ci'] is None
    assert torch.equal(ev.evaluate(X, Y)['probs'], res['probs'])    # latents pass through
