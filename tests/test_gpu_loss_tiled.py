"""The tiled MFMA contrastive loss on the GPU (csrc/loss_tiled.hip, ctclip_clip_loss_tiled) against the
torch restatement of test_loss_options_cpu.py evaluated in float64, and its dispatch through the
autograd Functions, the custom ops and the trainer (functional.set_loss_tiled).

Tolerances are the project's own for this loss (test_gpu_loss_options.py): loss and pair losses
1e-5 max(1, |ref|), every gradient and d loss / d log-temp 1e-4 relative (norm of the difference over
the norm of the reference).  Tile sizes of the kernels: 64 rows / columns (logits and gradient rows),
128 latent columns per gradient tile, K steps of 16 -- hence Bg 63 / 64 / 65 and Dl 127 / 129 below."""
import math

import pytest
import torch

from test_loss_options_cpu import general_loss, loss_and_grads

pytestmark = pytest.mark.gpu
dev = 'cuda'
LT = math.log(1 / 0.07)          # exp(S) stays finite with unit latents (|S| <= 14.3)


@pytest.fixture(scope='module')
def K():
    from ctclip_mi355x import kernels
    return kernels


@pytest.fixture()
def Fn():
    from ctclip_mi355x import functional
    old = functional.loss_tiled_mode()
    try:
        yield functional
    finally:
        functional.set_loss_tiled(old)


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _inputs(Bg, Dl, Vi, extra, seed=0):
    g = torch.Generator(device=dev).manual_seed(1000 * Bg + Dl + 7 * Vi + seed)
    r = lambda v: torch.randn(v, Bg, Dl, device=dev, generator=g)
    t, i = r(1), r(Vi)
    tx, ix = (r(1), r(Vi)) if extra else (None, None)
    return t, i, tx, ix, torch.tensor([LT], device=dev)


def _weights(Vi):
    return (0.9, 0.1) if Vi > 1 else (1.0, 0.0)


def _f64(*xs):
    return [None if x is None else x.double() for x in xs]


def _ref(t, i, lt, tx, ix, dcl, w_main, w_mv):
    """The restatement on float64 copies of the inputs (it follows the input dtype)."""
    return loss_and_grads(*_f64(t, i, lt, tx, ix), dcl, w_main, w_mv)


def _check(out, ref, extra, what=''):
    loss, dt, di, dtx, dix, dlt, pair = out
    rl, rdt, rdi, rdtx, rdix, rdlt, rpair = ref
    print(f'{what} loss {loss.item():.7f} ref {rl.item():.7f}; rel dt {rel(dt, rdt):.2e} di {rel(di, rdi):.2e} '
          f'dlt {rel(dlt, rdlt):.2e}')
    assert abs(loss.item() - rl.item()) < 1e-5 * max(1.0, abs(rl.item()))
    assert pair.shape == rpair.shape
    for a, b in zip(pair.tolist(), rpair.tolist()):
        assert abs(a - b) < 1e-5 * max(1.0, abs(b))
    assert rel(dt, rdt) < 1e-4 and rel(di, rdi) < 1e-4 and rel(dlt, rdlt) < 1e-4
    if extra:
        assert rel(dtx, rdtx) < 1e-4 and rel(dix, rdix) < 1e-4
    else:
        assert dtx is None and dix is None


# ------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize('extra', [False, True])
@pytest.mark.parametrize('dcl', [False, True])
@pytest.mark.parametrize('P', [1, 3])
@pytest.mark.parametrize('Dl', [64, 100, 512])
@pytest.mark.parametrize('Bg', [2, 3, 8, 63, 64, 65, 127, 128, 129, 257, 300])
def test_kernel_matches_float64(K, Bg, Dl, P, dcl, extra):
    """One tile, the tile edge +-1, several ragged tiles in both directions; Dl = 100: the K tail."""
    t, i, tx, ix, lt = _inputs(Bg, Dl, P, extra)
    w_main, w_mv = _weights(P)
    out = K.clip_loss_tiled(t, i, lt, tx, ix, dcl, w_main, w_mv)
    _check(out, _ref(t, i, lt, tx, ix, dcl, w_main, w_mv), extra)


@pytest.mark.parametrize('Dl', [2, 127, 129, 258])
def test_latent_width_around_the_gradient_chunk(K, Dl):
    """Dl not a multiple of 4 (the padded workspace rows) and +-1 around the 128-column gradient tile."""
    t, i, tx, ix, lt = _inputs(65, Dl, 3, True, seed=2)
    out = K.clip_loss_tiled(t, i, lt, tx, ix, True, 0.9, 0.1)
    _check(out, _ref(t, i, lt, tx, ix, True, 0.9, 0.1), True)


def test_kernel_matches_float64_1024(K):
    t, i, tx, ix, lt = _inputs(1024, 512, 1, False)
    out = K.clip_loss_tiled(t, i, lt)
    _check(out, _ref(t, i, lt, None, None, False, 1.0, 0.0), False)


@pytest.mark.parametrize('Bg', [8, 128])
def test_agrees_with_one_workgroup_kernel(K, Bg):
    """Where both run: within the tolerances above (the summation order differs, so not bitwise)."""
    t, i, tx, ix, lt = _inputs(Bg, 512, 3, True, seed=4)
    new = K.clip_loss_tiled(t, i, lt, tx, ix, True, 0.9, 0.1)
    old = K.clip_loss_ex(t, i, lt, tx, ix, True, 0.9, 0.1)
    _check(new, old, True, 'vs clip_loss_ex')
    t2, i2 = t[0].contiguous(), i[0].contiguous()
    loss, dt, di, _, _, dlt, _ = K.clip_loss_tiled(t2[None], i2[None], lt)
    l0, dt0, di0, dlt0 = K.clip_loss(t2, i2, lt)[:4]
    assert abs(loss.item() - l0.item()) < 1e-5 * max(1.0, abs(l0.item()))
    assert rel(dt[0], dt0) < 1e-4 and rel(di[0], di0) < 1e-4 and rel(dlt, dlt0) < 1e-4


def test_bit_reproducible(K):
    t, i, tx, ix, lt = _inputs(300, 512, 3, True, seed=5)
    a = K.clip_loss_tiled(t, i, lt, tx, ix, True, 0.9, 0.1)
    b = K.clip_loss_tiled(t, i, lt, tx, ix, True, 0.9, 0.1)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_row_ranges_give_the_bits_of_the_full_call(K):
    """A row's gradient does not depend on the range it was asked in; the scalars are always global."""
    Bg = 300
    t, i, tx, ix, lt = _inputs(Bg, 512, 3, True, seed=6)
    full = K.clip_loss_tiled(t, i, lt, tx, ix, True, 0.9, 0.1)
    _check(full, _ref(t, i, lt, tx, ix, True, 0.9, 0.1), True)
    for row0, n in [(0, 300), (37, 16), (299, 1), (128, 128)]:
        out = K.clip_loss_tiled(t, i, lt, tx, ix, True, 0.9, 0.1, rows=(row0, n))
        assert torch.equal(out[0], full[0]) and torch.equal(out[5], full[5]) and torch.equal(out[6], full[6])
        for g, f in zip(out[1:5], full[1:5]):
            assert g.shape == (f.shape[0], n, f.shape[2])
            assert torch.equal(g, f[:, row0:row0 + n]), (row0, n)


def test_zero_norm_rows_give_finite_gradients(K):
    """A zero latent row (norm below 1e-12) takes the g / max(n, 1e-12) branch of the l2norm backward, as
    in the one-workgroup kernels: everything stays finite."""
    t, i, tx, ix, lt = _inputs(130, 64, 2, True, seed=9)
    t[0, 1] = 0
    i[1, 3] = 0
    tx[0, 0] = 0
    ix[0, 129] = 0
    out = K.clip_loss_tiled(t, i, lt, tx, ix, True, 0.9, 0.1)
    assert all(torch.isfinite(x).all() for x in out)
    ref = _ref(t, i, lt, tx, ix, True, 0.9, 0.1)
    assert abs(out[0].item() - ref[0].item()) < 1e-5 * max(1.0, abs(ref[0].item()))


def test_refusals(K):
    """Host-side checks of the C entry point and the wrapper: nothing is launched."""
    from ctclip_mi355x._lib import KernelError
    lt = torch.tensor([LT], device=dev)
    z = lambda *s: torch.zeros(*s, device=dev)
    with pytest.raises(KernelError, match='1003'):        # CT_ESHAPE
        K.clip_loss_tiled(z(1, 8193, 4), z(1, 8193, 4), lt)
    with pytest.raises(KernelError, match='1003'):
        K.clip_loss_tiled(z(1, 2, 8193), z(1, 2, 8193), lt)
    with pytest.raises(KernelError, match='1003'):
        K.clip_loss_tiled(z(1, 2, 4), z(65, 2, 4), lt)
    t, i, tx, ix, lt = _inputs(8, 64, 1, True)
    for rows in [(0, 9), (8, 1), (-1, 2), (3, 0)]:
        with pytest.raises((ValueError, KernelError)):
            K.clip_loss_tiled(t, i, lt, rows=rows)
    with pytest.raises((ValueError, KernelError)):
        K.clip_loss_tiled(t, i, lt, tx, None)
    # the C entry point itself: a row range past Bg and half an extra pair are CT_EINVAL
    from ctclip_mi355x import _lib
    o = [torch.empty_like(t) for _ in range(4)]
    s = [torch.empty(1, device=dev) for _ in range(3)]
    ws = torch.empty(1 << 20, device=dev)

    def args(**kw):
        a = _lib.ClipLossTiledArgs(t_raw=t.data_ptr(), i_raw=i.data_ptr(), log_temp=lt.data_ptr(), Vt=1, Vi=1, Bg=8,
                                   Dl=64, w_main=1.0, loss=s[0].data_ptr(), pair_loss=s[1].data_ptr(),
                                   dlogtemp=s[2].data_ptr(), dt_raw=o[0].data_ptr(), di_raw=o[1].data_ptr(),
                                   dt_extra=o[2].data_ptr(), di_extra=o[3].data_ptr(), ws=ws.data_ptr(),
                                   ws_bytes=4 * ws.numel(), grad_row0=0, grad_rows=8)
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    call = lambda a: _lib.lib().ctclip_clip_loss_tiled(_lib.ctypes.byref(a), _lib.stream_ptr())
    assert call(args(grad_row0=1)) == 1001
    assert call(args(grad_rows=0)) == 1001
    assert call(args(t_extra=tx.data_ptr())) == 1001
    assert call(args(ws_bytes=64)) == 1001
    assert call(args(loss=None)) == 1001
    assert call(args(Bg=8193)) == 1003
    assert _lib.lib().ctclip_clip_loss_tiled_ws_bytes(_lib.ctypes.byref(args(Bg=8193))) == 0
    need = _lib.lib().ctclip_clip_loss_tiled_ws_bytes(_lib.ctypes.byref(args()))
    assert 0 < need <= 4 * ws.numel() and call(args()) == 0
    # the workspace of the largest shape does not fit 32 bits
    assert _lib.lib().ctclip_clip_loss_tiled_ws_bytes(_lib.ctypes.byref(args(Bg=8192, Vi=64))) > 2 ** 33


# ------------------------------------------------------------------------------ autograd Functions
def _leaves(*xs):
    return [None if x is None else x.detach().clone().requires_grad_(True) for x in xs]


def test_autograd_functions_over_128_rows(Fn):
    """Bg = 130 (world 1) under 'auto': the plain and the general Function take the tiled kernels."""
    assert Fn.loss_tiled_mode() == 'auto'
    t, i, tx, ix, lt = _inputs(130, 512, 2, True, seed=12)
    lt0 = lt.reshape(())
    # ClipLossFn: 2-D latents
    a = _leaves(t[0], i[0], lt0)
    loss = Fn.ClipLossFn.apply(*a)
    r = _leaves(*_f64(t[:1], i[:1], lt0))
    rl, _ = general_loss(*r)
    assert abs(loss.item() - rl.item()) < 1e-5 * max(1.0, abs(rl.item()))
    (2.0 * loss).backward()
    (2.0 * rl).backward()
    assert rel(a[0].grad, r[0].grad[0]) < 1e-4 and rel(a[1].grad, r[1].grad[0]) < 1e-4
    assert rel(a[2].grad, r[2].grad) < 1e-4
    # ClipLossExFn: view stacks, every option
    a = _leaves(t, i, tx, ix, lt0)
    loss = Fn.ClipLossExFn.apply(*a, True, 0.9, 0.1)
    r = _leaves(*_f64(t, i, tx, ix, lt0))
    rl, _ = general_loss(r[0], r[1], r[4], r[2], r[3], True, 0.9, 0.1)
    assert abs(loss.item() - rl.item()) < 1e-5 * max(1.0, abs(rl.item()))
    (2.0 * loss).backward()
    (2.0 * rl).backward()
    for x, y in zip(a, r):
        assert x.grad.shape == y.grad.shape and rel(x.grad, y.grad) < 1e-4


def test_autograd_functions_always_against_never(Fn):
    t, i, tx, ix, lt = _inputs(8, 512, 2, True, seed=13)
    lt0 = lt.reshape(())
    res = {}
    for mode in ('never', 'always'):
        Fn.set_loss_tiled(mode)
        a = _leaves(t[0], i[0], lt0)
        plain = Fn.ClipLossFn.apply(*a)
        plain.backward()
        b = _leaves(t, i, tx, ix, lt0)
        gen = Fn.ClipLossExFn.apply(*b, True, 0.9, 0.1)
        gen.backward()
        res[mode] = (plain.item(), gen.item(), [x.grad for x in a + b])
    for k in (0, 1):
        assert abs(res['always'][k] - res['never'][k]) < 1e-5 * max(1.0, abs(res['never'][k]))
    for x, y in zip(res['always'][2], res['never'][2]):
        assert rel(x, y) < 1e-4
    assert not all(torch.equal(x, y) for x, y in zip(res['always'][2], res['never'][2]))   # another kernel ran


# ------------------------------------------------------------------------------ torch.library ops
def test_custom_ops_over_128_rows(Fn):
    from ctclip_mi355x import ops
    t, i, tx, ix, lt = _inputs(130, 512, 2, True, seed=14)
    a = _leaves(t, i, lt, tx, ix)
    loss = ops.clip_infonce_ex(*a, decoupled=True, w_main=0.9, w_multiview=0.1)
    r = _leaves(*_f64(t, i, lt, tx, ix))
    rl, _ = general_loss(r[0], r[1], r[2], r[3], r[4], True, 0.9, 0.1)
    assert abs(loss.item() - rl.item()) < 1e-5 * max(1.0, abs(rl.item()))
    (2.0 * loss).backward()
    (2.0 * rl).backward()
    for x, y in zip(a, r):
        assert rel(x.grad, y.grad) < 1e-4
    utils = ('test_schema', 'test_faketensor', 'test_autograd_registration')
    torch.library.opcheck(torch.ops.ctclip.clip_infonce_ex, (t, i, lt, tx, ix, True, 0.9, 0.1), test_utils=utils)
    torch.library.opcheck(torch.ops.ctclip.clip_infonce_ex, (t, i, lt, None, None, False, 1.0, 0.0), test_utils=utils)
    # the plain op
    a = _leaves(t[0], i[0], lt)
    loss = ops.clip_infonce(*a)
    r = _leaves(*_f64(t[:1], i[:1], lt))
    rl, _ = general_loss(*r)
    assert abs(loss.item() - rl.item()) < 1e-5 * max(1.0, abs(rl.item()))
    loss.backward()
    rl.backward()
    assert rel(a[0].grad, r[0].grad[0]) < 1e-4 and rel(a[1].grad, r[1].grad[0]) < 1e-4
    assert rel(a[2].grad, r[2].grad) < 1e-4
    torch.library.opcheck(torch.ops.ctclip.clip_infonce, (t[0], i[0], lt), test_utils=utils)


# ------------------------------------------------------------------------------ trainer
def test_train_step_on_the_tiled_loss(Fn):
    """One CTClipTrainer step (B = 2, DCL + extra projection + one augmented view) with the loss forced
    onto the tiled kernels: two identical steps from the same state give the same bits, and the loss is
    that of the one-workgroup kernel within 1e-5 max(1, |loss|)."""
    from ctclip_mi355x.trainer import CTClipTrainer
    from test_gpu_loss_options import _batch, build, cfg_small
    cfg = cfg_small(layers=1)
    hu, aug, ids, mask, text = _batch(cfg)
    runs = []
    for mode in ('always', 'always', 'never'):
        Fn.set_loss_tiled(mode)
        torch.manual_seed(0)
        model = build(cfg, decoupled_contrastive_learning=True, extra_latent_projection=True)
        tr = CTClipTrainer(model, lr=1e-4)
        loss = tr.train_step(text, hu.cuda(), aug_image=aug.cuda())
        tr.flush()
        torch.cuda.synchronize()
        assert torch.isfinite(loss) and tr.norm[0].item() > 0
        runs.append((loss.detach().clone(), tr.flat.data.clone(), tr.m.clone(), tr.v.clone()))
        del model, tr
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    tiled, never = runs[0][0].item(), runs[2][0].item()
    print(f'train step loss: tiled {tiled:.7f} one-workgroup {never:.7f}')
    assert abs(tiled - never) < 1e-5 * max(1.0, abs(never))
