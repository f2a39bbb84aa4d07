"""The validation loop on the GPU: the evaluation loader kernel (ctclip_eval_volume), the bootstrap
AUROC kernel (ctclip_auroc_boot), ZeroShotEvaluator and CTClipTrainer.validate's status guard.

Loader: bit-equal to the reference's nii_img_to_tensor (tests/golden/make_golden_eval.py): every
operation is one IEEE rounding in numpy's type, so there is no tolerance.  AUROC: the kernel's value
is an exact integer ratio divided once in f64; sklearn's f64 trapezoid (the fixture) is within
O(N 2^-53) of it -> 1e-9 absolute; the numpy restatement (test_eval_cpu.auroc_table) divides the
same two integers, so it must agree to the last bit (asserted at 1e-15)."""
import types

import numpy as np
import pytest
import torch

from oracle import ctclip_oracle as O
from oracle import weights as W
from test_eval_cpu import G, LOADER_CASES, auroc_table, same_with_nan

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------ loader
def _expected(name):
    exp = torch.full((1, 240, 480, 480), -1.0, device='cuda')
    lo, box = G[f'{name}.box_lo'].tolist(), G[f'{name}.box']
    exp[0, lo[0]:lo[0] + box.shape[0], lo[1]:lo[1] + box.shape[1], lo[2]:lo[2] + box.shape[2]] = box.cuda()
    return exp


@pytest.mark.parametrize('name', LOADER_CASES)
def test_loader_matches_reference(name):
    from ctclip_mi355x.preprocess import eval_volume_to_tensor
    out = eval_volume_to_tensor(G[f'{name}.scan'].cuda())
    assert out.shape == (1, 240, 480, 480) and out.dtype == torch.float32
    assert torch.equal(out, _expected(name))         # the box, and -1 everywhere else


def test_loader_writes_a_batch_row():
    from ctclip_mi355x.preprocess import eval_volume_to_tensor
    batch = torch.full((2, 1, 240, 480, 480), 7.0, device='cuda')
    ret = eval_volume_to_tensor(G['vol3_float64.scan'].cuda(), out=batch[1])
    assert ret.data_ptr() == batch[1].data_ptr()
    assert torch.equal(batch[1], _expected('vol3_float64'))
    assert bool((batch[0] == 7.0).all())
    with pytest.raises(ValueError):
        eval_volume_to_tensor(G['vol0_float32.scan'].cuda(), out=batch[:, 0])     # not a (1, D, H, W) row


def _torch_loader(scan, target):
    """data_inference.py:78-122 in torch on the host (f32 / f64 IEEE arithmetic, one op at a time)."""
    x = scan.permute(1, 2, 0) * 1000
    x = ((x.clamp(-1000, 200) + 400) / 600).float()
    for ax, t in enumerate(target):
        n = x.shape[ax]
        start = max((n - t) // 2, 0)
        x = x.narrow(ax, start, min(start + t, n) - start)
    pads = []
    for ax in (2, 1, 0):
        before = (target[ax] - x.shape[ax]) // 2
        pads += [before, target[ax] - x.shape[ax] - before]
    return torch.nn.functional.pad(x, pads, value=-1.0).permute(2, 0, 1)[None].contiguous()


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('target', [(8, 12, 6), (8, 10, 6)])
@pytest.mark.parametrize('shape', [(5, 9, 7), (7, 6, 15), (9, 8, 12)])
def test_loader_small_targets(shape, target, dtype):
    """Rows shorter than a wave: a box whose w extent is no multiple of 4 inside 16-byte rows
    (w = 12), rows that are not 16-byte multiples (w = 10: the scalar store path), odd crop / pad
    offsets on every axis, and a scan that is not contiguous along w (strided scalar loads)."""
    from ctclip_mi355x.preprocess import eval_volume_to_tensor
    g = torch.Generator().manual_seed(sum(shape) + target[1])
    scan = (torch.rand(shape, generator=g, dtype=torch.float64) * 1.8 - 1.3).to(dtype)
    ref = _torch_loader(scan, target)
    out = eval_volume_to_tensor(scan.cuda(), target_shape=target)
    assert out.shape == (1, target[2], target[0], target[1])
    assert torch.equal(out.cpu(), ref)
    strided = scan.cuda().permute(2, 0, 1).contiguous().permute(1, 2, 0)
    assert strided.stride(2) != 1
    assert torch.equal(eval_volume_to_tensor(strided, target_shape=target).cpu(), ref)


# ------------------------------------------------------------------------------------------- AUROC
def _kernel(probs, labels, rows):
    from ctclip_mi355x.evaluate import _auroc_rows
    out = _auroc_rows(torch.as_tensor(probs).cuda(), torch.as_tensor(labels), rows)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_auroc_matches_sklearn_fixture():
    from ctclip_mi355x.evaluate import auroc, bootstrap_auroc
    probs, labels = G['met.probs'].cuda(), G['met.labels']
    boot = bootstrap_auroc(probs, labels, n_samples=64).cpu().numpy()
    ref = G['met.boot_auroc'].numpy()
    assert np.isnan(ref).any()
    print('max |kernel - sklearn|', np.nanmax(np.abs(boot - ref)))
    assert same_with_nan(boot, ref, 1e-9)
    assert same_with_nan(_kernel(G['met.probs'], labels, G['met.indices'].numpy()), ref, 1e-9)
    assert same_with_nan(auroc(probs, labels).cpu().numpy(), G['met.auroc'].numpy(), 1e-9)


def _case(N, P, S, seed, levels=None):
    g = np.random.default_rng(seed)
    probs = (g.integers(0, levels, (N, P)) / levels if levels else g.random((N, P))).astype(np.float32)
    labels = (g.random((N, P)) < 0.4).astype(np.uint8)
    rows = g.integers(0, N, (S, N)).astype(np.int32)
    rows[0] = np.arange(N)
    return probs, labels, rows


# N: one row, two, around a wave, more than one position per thread (300), both sides of the
# switch between the two LDS sizes (2048 / 2049)
@pytest.mark.parametrize('N', [1, 2, 63, 64, 65, 300, 2048, 2049])
def test_auroc_matches_restatement(N):
    probs, labels, rows = _case(N, 3, 5, seed=N, levels=8)
    assert same_with_nan(_kernel(probs, labels, rows), auroc_table(probs, labels, rows), 1e-15)
    probs, labels, rows = _case(N, 2, 3, seed=N + 1)          # continuous scores: (almost) no ties
    assert same_with_nan(_kernel(probs, labels, rows), auroc_table(probs, labels, rows), 1e-15)


def test_auroc_one_row_is_nan():
    probs, labels, rows = _case(1, 3, 4, seed=0)
    assert np.isnan(_kernel(probs, labels, rows)).all()


def test_auroc_largest_size_with_ties():
    probs, labels, rows = _case(8192, 2, 3, seed=5, levels=7)
    assert len(np.unique(probs)) == 7
    got = _kernel(probs, labels, rows)
    assert same_with_nan(got, auroc_table(probs, labels, rows), 1e-15) and not np.isnan(got).any()


def test_auroc_degenerate_inputs():
    N = 257
    probs, labels, rows = _case(N, 3, 4, seed=9)
    flat = np.full_like(probs, 0.5)                           # one tie group: 0.5 exactly
    got = _kernel(flat, labels, rows)
    assert (got == 0.5).all() and same_with_nan(got, auroc_table(flat, labels, rows), 0.0)
    ident = np.arange(N, dtype=np.int32)[None]                # S = 1, the point estimate
    assert same_with_nan(_kernel(probs, labels, ident), auroc_table(probs, labels, ident), 1e-15)
    one = np.full((2, N), 17, dtype=np.int32)                 # one row drawn N times: one class
    one[1] = N - 1
    assert np.isnan(_kernel(probs, labels, one)).all()


def test_auroc_rejects_more_than_8192_rows():
    from ctclip_mi355x._lib import KernelError
    probs, labels, rows = _case(8193, 1, 1, seed=1)
    with pytest.raises(KernelError, match='1003'):            # CT_ESHAPE
        _kernel(probs, labels, rows)


def test_auroc_is_reproducible():
    probs, labels, rows = _case(1500, 4, 16, seed=3, levels=16)
    a, b = _kernel(probs, labels, rows), _kernel(probs, labels, rows)
    assert np.array_equal(a.view(np.int64), b.view(np.int64))


# --------------------------------------------------------------------------- evaluator and trainer
@pytest.fixture(scope='module')
def tiny():
    from test_gpu_model import build, cfg_small
    from ctclip_mi355x.zero_shot import ZeroShotClassifier, PATHOLOGIES
    from ctclip_mi355x import kernels as K
    torch.manual_seed(0)
    cfg = cfg_small()
    model = build(cfg)
    P = 3
    pids, pmask = W.make_text(2 * P, 32, cfg.bert.vocab_size, seed=99, ragged=True)
    zs = ZeroShotClassifier(model, pathologies=PATHOLOGIES[:P])
    zs.set_prompts(types.SimpleNamespace(input_ids=pids.cuda(), attention_mask=pmask.cuda()))
    video = O.normalize_hu(W.make_hu(4, cfg.vit)).cuda()
    labels = torch.tensor([[1, 0, 1], [0, 1, 0], [1, 1, 0], [0, 0, 0]], dtype=torch.uint8)
    K.reset_ln_status()
    return cfg, model, zs, video, labels


def test_evaluator_matches_classifier(tiny):
    from ctclip_mi355x.evaluate import ZeroShotEvaluator
    cfg, model, zs, video, labels = tiny
    ev = ZeroShotEvaluator(zs)
    res = ev.evaluate(video, labels, n_boot=8, batch_size=2)
    probs = zs.predict(video, batch_size=2)[0]
    assert torch.equal(res['probs'], probs)
    ident = np.arange(4)[None]
    assert same_with_nan(res['auroc'].cpu().numpy(), auroc_table(probs.cpu().numpy(), labels.numpy(), ident)[0], 1e-15)
    assert res['ci'].shape == (3, 3) and 0.0 <= res['f1_micro'] <= 1.0 and 0.0 <= res['flat_accuracy'] <= 1.0
    # an iterable of batches: the same forwards, the same numbers
    res2 = ev.evaluate([video[:2], video[2:]], labels, batch_size=2)
    assert torch.equal(res2['probs'], probs) and res2['ci'] is None


def test_validate_owns_its_status_bits(tiny):
    from ctclip_mi355x import kernels as K
    from ctclip_mi355x.trainer import CTClipTrainer, EvalGuardError, StepGuardError
    cfg, model, zs, video, labels = tiny
    ids, mask = W.make_text(2, 32, cfg.bert.vocab_size, ragged=True)
    text = types.SimpleNamespace(input_ids=ids.cuda(), attention_mask=mask.cuda())
    K.reset_ln_status()
    tr = CTClipTrainer(model, lr=1e-3)
    tr.train_step(text, video[:2])
    tr.check()
    word = K.status_word(video.device)
    snap = word.clone()
    bad = video[:2].clone()
    bad[1, 0, 17, 33, 71] = float('nan')
    assert model.training
    with pytest.raises(EvalGuardError) as ei:
        tr.validate(bad, labels[:2], classifier=zs)
    assert isinstance(ei.value, StepGuardError) and ei.value.bits != 0
    print('flagged validation:', ei.value)
    assert torch.equal(word, snap) and model.training
    before = tr.flat.data.clone()
    loss = tr.train_step(text, video[:2])
    tr.check()                                                # not blamed for the validation's bits
    assert torch.isfinite(loss) and not torch.equal(before, tr.flat.data)
    res = tr.validate(video[:2], labels[:2])                  # the classifier passed before
    assert bool(torch.isfinite(res['auroc']).all()) and bool(torch.isfinite(res['probs']).all())
    assert model.training and torch.equal(word, snap)
    model.eval()
    tr.validate(video[:2], labels[:2])
    assert not model.training
    model.train()
