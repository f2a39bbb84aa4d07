"""The pairwise sigmoid (SigLIP) contrastive loss on the GPU (csrc/loss_sigmoid.hip, ctclip_sigmoid_loss;
DESIGN.md §30) against the torch restatement of sigmoid_loss_common.py evaluated in float64, and the
option through the autograd Function, the custom op, CTCLIP.forward, the trainer, the chunked step, the
checkpoint and the evaluators.

Tolerances are the project's own for its losses (test_gpu_loss_tiled.py): loss 1e-5 max(1, |ref|), every
gradient, d loss / d log-temp and d loss / d bias 1e-4 relative (norm of the difference over the norm of
the reference).  Tile sizes of the kernels: 64 rows / columns (logits and gradient rows), 128 latent
columns per gradient tile, K steps of 16, workspace rows padded to 4 -- hence Bg 63 / 64 / 65 / 127 / 128 /
129 and Dl 2 / 100 / 127 / 129 below."""
import math

import pytest
import torch

from sigmoid_loss_common import (B_PAPER, LT_PAPER, TEMP_BIAS, batch, build, cfg_small, check, ref64, rel,
                                 sigmoid_loss)

pytestmark = pytest.mark.gpu
dev = 'cuda'
LR = 1e-3


@pytest.fixture(scope='module')
def K():
    from ctclip_mi355x import kernels
    return kernels


def _inputs(Bg, Dl, seed=0):
    g = torch.Generator(device=dev).manual_seed(1000 * Bg + Dl + seed)
    return torch.randn(Bg, Dl, device=dev, generator=g), torch.randn(Bg, Dl, device=dev, generator=g)


def _scalars(lt, b):
    return torch.tensor([lt], device=dev), torch.tensor([b], device=dev)


# ------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize('Dl', [2, 64, 100, 127, 129, 512])
@pytest.mark.parametrize('Bg', [1, 2, 3, 8, 63, 64, 65, 127, 128, 129, 257, 300])
def test_kernel_matches_float64(K, Bg, Dl):
    """One tile, the tile edges +-1, several ragged tiles in both directions, the K / Dl tails; the paper's
    initialisation, (1, 0) and (log 1/0.07, -3) on the same latents."""
    t, i = _inputs(Bg, Dl)
    for lt, b in TEMP_BIAS:
        ltt, bt = _scalars(lt, b)
        check(K.sigmoid_loss(t, i, ltt, bt), ref64(t, i, ltt, bt), f'Bg {Bg} Dl {Dl} ({lt:.3f}, {b})')


@pytest.mark.parametrize('lt,b', TEMP_BIAS)
def test_kernel_matches_float64_1024(K, lt, b):
    t, i = _inputs(1024, 512)
    ltt, bt = _scalars(lt, b)
    check(K.sigmoid_loss(t, i, ltt, bt), ref64(t, i, ltt, bt), f'Bg 1024 ({lt:.3f}, {b})')


@pytest.mark.parametrize('lt,b', [(math.log(40.0), 0.0), (math.log(30.0), -10.0), (math.log(30.0), 10.0)])
def test_saturation_on_both_signs(K, lt, b):
    """Latents arranged so that the cosines reach +1 and -1 on and off the diagonal: |x| reaches 40 on both
    signs for positives and negatives.  exp(-|u|) never overflows, so nothing is inf or inf * 0; loss and
    gradients stay finite and within the tolerances."""
    Bg, Dl = 70, 96
    t, i = _inputs(Bg, Dl, seed=3)
    i[0:20] = 2.0 * t[0:20]                    # positives with cos = +1
    i[20:40] = -0.5 * t[20:40]                 # positives with cos = -1
    i[40:50] = t[50:60]                        # negatives with cos = +1 ...
    i[60:70] = -t[40:50]                       # ... and -1
    ltt, bt = _scalars(lt, b)
    ref = ref64(t, i, ltt, bt)
    tn, inn = torch.nn.functional.normalize(t.double(), dim=-1), torch.nn.functional.normalize(i.double(), dim=-1)
    x = math.exp(lt) * (tn @ inn.t()) + b
    print(f'x in [{x.min().item():.2f}, {x.max().item():.2f}], diagonal [{x.diag().min().item():.2f}, '
          f'{x.diag().max().item():.2f}]')
    assert x.abs().max().item() >= 39.9 and x.min().item() < -19.9 and x.max().item() > 19.9
    out = K.sigmoid_loss(t, i, ltt, bt)
    assert all(torch.isfinite(o).all() for o in out)
    check(out, ref, 'saturated')


def test_zero_norm_rows_give_finite_gradients(K):
    """A zero latent row (norm below 1e-12) takes the g / max(n, 1e-12) branch of the l2norm backward, as in
    the InfoNCE kernels: everything stays finite and the loss is the restatement's."""
    t, i = _inputs(130, 64, seed=9)
    t[1] = 0
    i[129] = 0
    ltt, bt = _scalars(LT_PAPER, B_PAPER)
    out = K.sigmoid_loss(t, i, ltt, bt)
    assert all(torch.isfinite(x).all() for x in out)
    ref = ref64(t, i, ltt, bt)
    assert abs(out[0].item() - ref[0].item()) < 1e-5 * max(1.0, abs(ref[0].item()))


def test_bit_reproducible(K):
    t, i = _inputs(300, 512, seed=5)
    ltt, bt = _scalars(LT_PAPER, B_PAPER)
    a = K.sigmoid_loss(t, i, ltt, bt)
    b = K.sigmoid_loss(t, i, ltt, bt)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_row_ranges_give_the_bits_of_the_full_call(K):
    """A row's gradient does not depend on the range it was asked in; the scalars are always global."""
    Bg = 300
    t, i = _inputs(Bg, 512, seed=6)
    ltt, bt = _scalars(math.log(1 / 0.07), -3.0)
    full = K.sigmoid_loss(t, i, ltt, bt)
    check(full, ref64(t, i, ltt, bt))
    for row0, n in [(0, Bg), (37, 16), (Bg - 1, 1), (128, 128)]:
        out = K.sigmoid_loss(t, i, ltt, bt, rows=(row0, n))
        assert torch.equal(out[0], full[0]) and torch.equal(out[3], full[3]) and torch.equal(out[4], full[4])
        for g, f in zip(out[1:3], full[1:3]):
            assert g.shape == (n, f.shape[1])
            assert torch.equal(g, f[row0:row0 + n]), (row0, n)


def test_refusals(K):
    """Host-side checks of the wrapper and the C entry point: nothing is launched."""
    from ctclip_mi355x import _lib
    from ctclip_mi355x._lib import KernelError
    t, i = _inputs(8, 64)
    ltt, bt = _scalars(1.0, 0.0)
    for rows in [(0, 9), (8, 1), (-1, 2), (3, 0)]:
        with pytest.raises(ValueError, match='rows'):
            K.sigmoid_loss(t, i, ltt, bt, rows=rows)
    with pytest.raises(ValueError, match='f32'):
        K.sigmoid_loss(t.double(), i.double(), ltt, bt)
    with pytest.raises(ValueError, match='f32'):
        K.sigmoid_loss(t, i, ltt, bt.half())
    with pytest.raises(ValueError, match='contiguous'):
        K.sigmoid_loss(t.t().contiguous().t(), i, ltt, bt)
    with pytest.raises(ValueError, match='latent sets'):
        K.sigmoid_loss(t, i[:7], ltt, bt)
    with pytest.raises(ValueError, match='latent sets'):
        K.sigmoid_loss(t[None], i[None], ltt, bt)
    z = lambda *s: torch.zeros(*s, device=dev)
    with pytest.raises(KernelError, match='1003'):        # CT_ESHAPE
        K.sigmoid_loss(z(8193, 4), z(8193, 4), ltt, bt)
    with pytest.raises(KernelError, match='1003'):
        K.sigmoid_loss(z(2, 8193), z(2, 8193), ltt, bt)
    o = [torch.empty_like(t) for _ in range(2)]
    s = [torch.empty(1, device=dev) for _ in range(3)]
    ws = torch.empty(1 << 16, device=dev)

    def args(**kw):
        a = _lib.SigmoidLossArgs(t_raw=t.data_ptr(), i_raw=i.data_ptr(), log_temp=ltt.data_ptr(), bias=bt.data_ptr(),
                                 Bg=8, Dl=64, grad_row0=0, grad_rows=8, loss=s[0].data_ptr(), dt_raw=o[0].data_ptr(),
                                 di_raw=o[1].data_ptr(), dlogtemp=s[1].data_ptr(), dbias=s[2].data_ptr(),
                                 ws=ws.data_ptr(), ws_bytes=4 * ws.numel())
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    call = lambda a: _lib.lib().ctclip_sigmoid_loss(_lib.ctypes.byref(a), _lib.stream_ptr())
    nbytes = lambda a: _lib.lib().ctclip_sigmoid_loss_ws_bytes(_lib.ctypes.byref(a))
    assert call(args(grad_row0=1)) == 1001
    assert call(args(grad_rows=0)) == 1001
    assert call(args(ws_bytes=64)) == 1001
    assert call(args(bias=None)) == 1001 and call(args(dbias=None)) == 1001
    assert call(args(Bg=8193)) == 1003 and call(args(Dl=0)) == 1003
    assert call(args(ws=ws.data_ptr() + 4)) == 1002
    assert nbytes(args(Bg=8193)) == 0
    assert 0 < nbytes(args()) <= 4 * ws.numel() and call(args()) == 0
    # the stored gradient matrix of the largest batch does not fit 32 bits
    assert nbytes(args(Bg=8192, Dl=512)) > 2 ** 28
    assert _lib.lib().ctclip_version() == 2


# ------------------------------------------------------------------------------ autograd Function, custom op
def _leaves(*xs):
    return [x.detach().clone().requires_grad_(True) for x in xs]


@pytest.mark.parametrize('Bg', [8, 130])
def test_function_backward_is_the_kernel_outputs_times_the_upstream_gradient(K, Bg):
    """``SigmoidLossFn.backward`` under a non-unit upstream gradient: the kernel's outputs scaled (bit for
    bit: one f32 product each), and the float64 gradient of 2.5 L within the tolerances."""
    from ctclip_mi355x import functional as Fn
    t, i = _inputs(Bg, 512, seed=12)
    lt0, b0 = torch.tensor(LT_PAPER, device=dev), torch.tensor(B_PAPER, device=dev)
    a = _leaves(t, i, lt0, b0)
    loss = Fn.SigmoidLossFn.apply(*a)
    (2.5 * loss).backward()
    out = K.sigmoid_loss(t, i, lt0.reshape(1), b0.reshape(1))
    assert torch.equal(loss.detach().reshape(1), out[0])
    for x, g in zip(a, out[1:]):
        assert x.grad.shape == x.shape and torch.equal(x.grad, (g * 2.5).reshape(x.shape))
    r = _leaves(*[x.double().cpu() for x in (t, i, lt0, b0)])
    (2.5 * sigmoid_loss(*r)).backward()
    for x, y in zip(a, r):
        assert rel(x.grad, y.grad) < 1e-4
    # all rows from the one call, for the chunked step
    allrows = Fn.sigmoid_loss_all_rows(t, i, lt0, b0)
    for x, y in zip(allrows, out):
        assert torch.equal(x, y)


def test_custom_op(K):
    from torch._subclasses.fake_tensor import FakeTensorMode
    from ctclip_mi355x import ops
    t, i = _inputs(130, 512, seed=14)
    ltt, bt = _scalars(math.log(1 / 0.07), -3.0)
    a = _leaves(t, i, ltt, bt)
    loss = ops.sigmoid_loss(*a)
    r = _leaves(*[x.double().cpu() for x in (t, i, ltt, bt)])
    rl = sigmoid_loss(*r)
    assert abs(loss.item() - rl.item()) < 1e-5 * max(1.0, abs(rl.item()))
    (2.0 * loss).backward()
    (2.0 * rl).backward()
    for x, y in zip(a, r):
        assert x.grad.shape == x.shape and rel(x.grad, y.grad) < 1e-4
    utils = ('test_schema', 'test_faketensor', 'test_autograd_registration')
    torch.library.opcheck(torch.ops.ctclip.sigmoid_loss, (t, i, ltt, bt), test_utils=utils)
    with FakeTensorMode():
        ft, fs = torch.empty(8, 512, device=dev), torch.empty(1, device=dev)
        out = torch.ops.ctclip.sigmoid_loss(ft, ft, fs, fs)
        assert out[0].shape == () and out[1].shape == out[2].shape == ft.shape and out[3].shape == out[4].shape == (1,)
    with pytest.raises(Exception):      # registered for the HIP device only
        torch.ops.ctclip.sigmoid_loss(t.cpu(), i.cpu(), ltt.cpu(), bt.cpu())


# ------------------------------------------------------------------------------ model level
def _trainer(K, seed=0, **options):
    from ctclip_mi355x.trainer import CTClipTrainer
    K.reset_ln_status()
    torch.manual_seed(0)
    return CTClipTrainer(build(cfg_small(), seed=seed, sigmoid_loss=True, **options), lr=LR)


def _raw_latents(model, text, hu):
    """The raw latents of a train-mode forward at the current weights (dropout is 0 in ``build``), codebook
    EMA withheld, no graph: what the next ``train_step`` on the same batch feeds to the loss."""
    model.train()
    old = model.set_ema_mode('skip')
    try:
        with torch.no_grad():
            _, _, t_raw, i_raw = model.encode(text, hu)
    finally:
        model.set_ema_mode(old)
    return t_raw.clone(), i_raw.clone()


def test_forward_loss_and_scores():
    """``forward(return_loss=True)`` is the restatement (float64) on the latents ``return_latents`` gives
    (l2-normalised already: normalising again changes nothing); the keyword is not swallowed -- the value is
    not InfoNCE's.  Without ``return_loss`` the scores are ``clip_scores + logit_bias``."""
    from ctclip_mi355x import kernels as K
    cfg = cfg_small()
    model = build(cfg, sigmoid_loss=True)
    with torch.no_grad():
        model.temperature.fill_(LT_PAPER)       # the paper's initialisation (the seeded state_dict holds 1)
    hu, text = batch(cfg, 4)
    model.eval()
    with torch.no_grad():
        loss = model(text, hu, return_loss=True)
        tn, inn, tokens = model(text, hu, return_latents=True)
        enc_text, pooled = model(text, hu, return_encodings=True)
        scores = model(text, hu)
    assert enc_text.shape[0] == 4 and pooled.shape[0] == 4 and tokens.shape[0] == 4
    lt, b = model.temperature.detach(), model.logit_bias.detach()
    assert abs(lt.item() - LT_PAPER) < 1e-6 and b.item() == B_PAPER
    ref = sigmoid_loss(tn.double().cpu(), inn.double().cpu(), lt.double().cpu(), b.double().cpu()).item()
    plain = K.clip_loss(tn.contiguous(), inn.contiguous(), lt.reshape(1))[0].item()
    print(f'loss {loss.item():.7f} restatement {ref:.7f} (InfoNCE on the same latents {plain:.7f})')
    assert abs(loss.item() - ref) < 1e-5 * max(1.0, abs(ref))
    assert abs(loss.item() - plain) > 1e-2
    want = K.clip_scores(tn.contiguous(), inn.contiguous(), lt.reshape(1)) + b
    assert scores.shape == (4,) and (scores - want).abs().max().item() < 1e-5 * max(1.0, want.abs().max().item())
    assert (scores - lt.exp() * (tn * inn).sum(-1) - b).abs().max().item() < 1e-4


@pytest.fixture(scope='module')
def steps(K, tmp_path_factory):
    """Two ``train_step``s of a sigmoid model on two batches (run A), and the same stopped after the first:
    saved, loaded into a stranger (other weights, other bias, another seed) and continued (run B)."""
    from test_gpu_checkpoint import snapshot
    cfg = cfg_small()
    data = [batch(cfg, 2, seed=s) for s in range(2)]
    out = {}
    tr = _trainer(K)
    model = tr.model
    named = dict(model.named_parameters())
    assert named['logit_bias'].requires_grad and any(p is model.logit_bias for p in tr.flat.params)
    hu, text = data[0]
    out['latents'] = _raw_latents(model, text, hu)
    out['p0'] = (model.temperature.detach().clone(), model.logit_bias.detach().clone())
    out['hyper'] = (tr.lr, tr.betas, tr.eps)
    out['loss1'] = tr.train_step(text, hu).reshape(1).clone()
    tr.flush()
    torch.cuda.synchronize()
    out['p1'] = (model.temperature.detach().clone(), model.logit_bias.detach().clone())
    out['norm'] = tr.norm.clone()
    out['loss2'] = tr.train_step(data[1][1], data[1][0]).reshape(1).clone()
    out['A'] = snapshot(tr)
    del tr, model
    # run B
    path = str(tmp_path_factory.mktemp('ck') / 'sigmoid.pt')
    tr = _trainer(K)
    tr.train_step(data[0][1], data[0][0])
    tr.save(path)
    del tr
    from ctclip_mi355x.trainer import CTClipTrainer
    torch.manual_seed(77)
    tr = CTClipTrainer(build(cfg, seed=7, sigmoid_loss=True, sigmoid_bias_init=-3.0), lr=LR)
    out['load'] = tr.load(path)
    out['loaded_bias'] = tr.model.logit_bias.detach().clone()
    out['loss2_resumed'] = tr.train_step(data[1][1], data[1][0]).reshape(1).clone()
    out['B'] = snapshot(tr)
    out['path'] = path
    del tr
    return out


def test_train_step_moves_bias_and_temperature_by_the_predicted_adam_update(steps):
    """Step 1 of Adam moves a parameter by -lr g c / (|g c| + eps) (c the clip coefficient): with g the
    FLOAT64 gradient of the restatement on the step's own raw latents, ``logit_bias`` and ``temperature``
    land there within 1e-5 lr plus one f32 ulp of the parameter (the allowance of test_gpu_chunked_step.py).
    The loss of the step is the restatement's."""
    t_raw, i_raw = steps['latents']
    lt0, b0 = steps['p0']
    rl, _, _, rdlt, rdb = ref64(t_raw, i_raw, lt0.reshape(1), b0.reshape(1))
    loss = steps['loss1'].item()
    print(f'step loss {loss:.7f} restatement {rl.item():.7f}; f64 dlt {rdlt.item():.6e} dbias {rdb.item():.6e}; '
          f'grad norm {steps["norm"][0].item():.4e} clip {steps["norm"][1].item():.4e}')
    assert abs(loss - rl.item()) < 1e-5 * max(1.0, abs(rl.item()))
    lr, _, eps = steps['hyper']
    coef = steps['norm'][1].double().item()
    for name, p0, p1, g in (('temperature', lt0, steps['p1'][0], rdlt), ('logit_bias', b0, steps['p1'][1], rdb)):
        gc = g.item() * coef
        want = p0.double().item() - lr * gc / (abs(gc) + eps)
        err = abs(p1.double().item() - want)
        print(f'{name}: {p0.item():.7f} -> {p1.item():.7f}, predicted {want:.7f}, |d| {err:.2e}')
        assert p1.item() != p0.item() and abs(gc) > 1e3 * eps
        assert err <= 1e-5 * lr + abs(want) * 2.0 ** -23, name


def test_save_load_step_gives_the_bits_of_the_uninterrupted_run(steps):
    from test_gpu_checkpoint import assert_same
    res = steps['load']
    assert res['step'] == 1 and not res['missing_keys'] and not res['unexpected_keys'] and res['hyper_mismatch'] == {}
    assert torch.equal(steps['loaded_bias'], steps['p1'][1]) and steps['loaded_bias'].item() != -3.0
    ck = torch.load(steps['path'], map_location='cpu', weights_only=True)
    assert torch.equal(ck['model']['logit_bias'], steps['p1'][1].cpu())
    assert 'logit_bias' in ck['optim']['exp_avg'] and 'logit_bias' in ck['optim']['exp_avg_sq']
    assert torch.equal(steps['loss2_resumed'], steps['loss2'])
    assert 'logit_bias' in steps['A']['param'] and 'logit_bias' in steps['A']['m']
    assert_same(steps['A'], steps['B'])


def test_plain_checkpoint_into_a_sigmoid_model_reports_the_bias_missing(K, tmp_path):
    from ctclip_mi355x.trainer import CTClipTrainer
    cfg = cfg_small(layers=1)
    K.reset_ln_status()
    plain = CTClipTrainer(build(cfg), lr=LR)
    path = str(tmp_path / 'plain.pt')
    plain.save(path)
    assert 'logit_bias' not in torch.load(path, map_location='cpu', weights_only=True)['model']
    del plain
    tr = CTClipTrainer(build(cfg, seed=7, sigmoid_loss=True), lr=LR)
    with pytest.raises(Exception, match='logit_bias'):
        tr.load(path)                                   # strict: the moments and the key are missing
    bare = str(tmp_path / 'bare.pt')
    torch.save(torch.load(path, map_location='cpu', weights_only=True)['model'], bare)
    res = tr.load(bare, strict=False)
    assert res['missing_keys'] == ['logit_bias'] and not res['unexpected_keys']
    assert tr.model.logit_bias.item() == B_PAPER


def test_chunked_step_matches_train_step(K):
    """Bg = 4: ``train_step_chunked(chunk=2)`` against ``train_step`` from the same state -- the loss within
    1e-5 max(1, |loss|) (the project's loss tolerance) -- and the same bits on repeat (loss, parameters,
    moments).  The bias gets its gradient once: it moves by the one-shot step's update."""
    cfg = cfg_small()
    hu, text = batch(cfg, 4)
    runs = []
    for chunk in (2, 2, None):
        tr = _trainer(K)
        b0 = tr.model.logit_bias.item()
        loss = tr.train_step_chunked(text, hu, 2) if chunk else tr.train_step(text, hu)
        tr.flush()
        torch.cuda.synchronize()
        assert torch.isfinite(loss) and tr.steps == 1 and tr.model.logit_bias.item() != b0
        runs.append((loss.reshape(1).clone(), tr.flat.data.clone(), tr.m.clone(), tr.v.clone(),
                     tr.model.logit_bias.detach().clone(), tr.model.temperature.detach().clone()))
        del tr
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    chunked, one = runs[0][0].item(), runs[2][0].item()
    print(f'loss: chunked {chunked:.7f} one-shot {one:.7f} |d| {abs(chunked - one):.2e}; bias {runs[0][4].item():.7f} '
          f'/ {runs[2][4].item():.7f}; temperature {runs[0][5].item():.7f} / {runs[2][5].item():.7f}')
    assert abs(chunked - one) < 1e-5 * max(1.0, abs(one))
    # step 1 of Adam moves a scalar by lr (its sign): added once, not once per chunk
    for k in (4, 5):
        assert abs(runs[0][k].item() - runs[2][k].item()) <= 1e-5 * LR + abs(runs[2][k].item()) * 2.0 ** -23


def test_evaluators_do_not_see_the_bias():
    """The bias cancels in the zero-shot softmax over a prompt pair and does not move a retrieval rank:
    probabilities and ranks are the same bits with ``logit_bias`` -10 and +3."""
    from ctclip_mi355x.retrieval import RetrievalEvaluator
    from ctclip_mi355x.zero_shot import ZeroShotClassifier
    cfg = cfg_small(layers=1)
    model = build(cfg, sigmoid_loss=True)
    hu, text = batch(cfg, 4)
    res = []
    for b in (-10.0, 3.0):
        with torch.no_grad():
            model.logit_bias.fill_(b)
        zs = ZeroShotClassifier(model, pathologies=('a', 'b')).set_prompts(text)
        probs, scores = zs.predict(hu)
        ev = RetrievalEvaluator(model).evaluate(hu, text)
        with torch.no_grad():
            model.eval()
            logits = model(text, hu)
        res.append((probs.clone(), scores.clone(), ev['report_to_volume']['ranks'].clone(),
                    ev['volume_to_report']['ranks'].clone(), logits.clone()))
    for a, b in zip(res[0][:4], res[1][:4]):
        assert torch.equal(a, b)
    assert res[0][0].shape == (4, 2) and res[0][2].shape == (4,)
    assert (res[1][4] - res[0][4] - 13.0).abs().max().item() < 1e-4      # the logits themselves do move
