"""The SimSiam visual self-supervision head on the GPU (csrc/ssl.hip): the three kernels per
element against the float64 restatements and bounds of visual_ssl_common.py, the autograd Functions, the custom
ops, and ``CTCLIP(visual_ssl=VisualSSLHead(...))`` through forward, the trainer and the checkpoint.

Shapes (G, R, K, N) of the fused Linear + BatchNorm kernel: one group of two rows with K, N tails
(1, 2, 40, 72); K = 516 = 16 steps of 32 + 4, past the 4-step load ring (2, 3, 516, 72); N = 4 below the
16-feature strip (2, 8, 512, 4); the 128-row limit, all eight row blocks, N = 130 = 8 strips + 2
(2, 64, 64, 130).  The three launch variants (<= 32, <= 64, <= 128 rows) are all among them."""
import types

import pytest
import torch

from sigmoid_loss_common import batch, cfg_small
from visual_ssl_common import (EPS, FLAGS, MOM, SHAPES, U, bn_bwd_bounds, bn_bwd_ref, head_ref64, linear_bn_bounds,
                               linear_bn_ref, make_inputs, simsiam_ref_grads, worst)

pytestmark = pytest.mark.gpu
dev = 'cuda'
GUARD, FILL = 64, -777.0
LR = 1e-3


@pytest.fixture(scope='module')
def K():
    from ctclip_mi355x import kernels
    return kernels


def _to_dev(inp):
    """The inputs on the device; X as a view of a NaN-filled buffer with a row stride of K + 4."""
    d = {k: (None if v is None else v.to(dev)) for k, v in inp.items() if k != 'X'}
    M, Kd = inp['X'].shape
    buf = torch.full((M + 2, Kd + 4), float('nan'), device=dev)
    buf[1:M + 1, :Kd] = inp['X'].to(dev)
    d['X'] = buf[1:M + 1, :Kd]
    assert d['X'].stride(0) == Kd + 4 and torch.equal(d['X'].cpu(), inp['X'])
    return d


def _guarded(*shape):
    """A contiguous output view with FILL-valued guard bands on both sides."""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + 2 * GUARD,), FILL, device=dev)
    return flat, flat[GUARD:GUARD + n].view(*shape)


def _guards_intact(flat):
    return bool((flat[:GUARD] == FILL).all() and (flat[-GUARD:] == FILL).all())


def _launch(K, d, G, relu, use_running=False, guarded=False):
    M, N = d['X'].shape[0], d['W'].shape[0]
    rm, rv = d['running_mean'].clone(), d['running_var'].clone()
    outs = [_guarded(M, N), _guarded(M, N), _guarded(G, N)] if guarded else [(None, None)] * 3
    out, xhat, rstd = K.ssl_linear_bn(d['X'], d['W'], rm, rv, groups=G, bias=d['bias'], gamma=d['gamma'],
                                      beta=d['beta'], relu=relu, eps=EPS, momentum=MOM, use_running=use_running,
                                      out=outs[0][1], xhat=outs[1][1], rstd=outs[2][1])
    if guarded:
        assert all(_guards_intact(f) for f, _ in outs)
    return dict(out=out, xhat=xhat, rstd=rstd, running_mean=rm, running_var=rv)


# ------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize('affine,relu,bias', FLAGS)
@pytest.mark.parametrize('G,R,K_,N', SHAPES)
def test_linear_bn_forward(K, G, R, K_, N, affine, relu, bias):
    inp = make_inputs(G, R, K_, N, affine, bias)
    d = _to_dev(inp)
    ref = linear_bn_ref(inp, G, relu)
    bound = linear_bn_bounds(inp, ref, G)
    got = _launch(K, d, G, relu, guarded=True)
    for k in ('out', 'xhat', 'rstd'):
        w = worst(got[k], ref[k], bound[k])
        print(f'{k}: worst |d| / bound {w:.3f}')
        assert w <= 1.0, k
    # running statistics: G successive float64 BatchNorm1d calls on the float64 y.  Bounds: the group mean is
    # within bc / 2 = max_r bound_y, its variance within 2 bc sqrt(var) (visual_ssl_common), both plus the
    # (R + 8) u of the f32 sums, each entering with the momentum; 8 u of the result for the update itself
    bn = torch.nn.BatchNorm1d(N, eps=EPS, momentum=MOM, affine=False).double()
    bn.running_mean.copy_(inp['running_mean'])
    bn.running_var.copy_(inp['running_var'])
    yg = ref['y'].view(G, R, N)
    for g in range(G):
        bn(yg[g])
    by = 4 * K_ * U * (inp['X'].double().abs() @ inp['W'].double().abs().t()) + U * ref['y'].abs()
    bc = 2 * by.view(G, R, N).amax(1)
    var = yg.var(1, unbiased=False)
    acc = (R + 8) * U
    b_rm = MOM * (bc / 2 + acc * yg.abs().mean(1)).sum(0) + 8 * U * bn.running_mean.abs()
    b_rv = MOM * ((2 * bc * var.sqrt() + acc * var) * R / (R - 1)).sum(0) + 8 * U * bn.running_var.abs()
    assert worst(got['running_mean'], bn.running_mean, b_rm) <= 1.0
    assert worst(got['running_var'], bn.running_var, b_rv) <= 1.0
    assert not torch.equal(got['running_mean'], d['running_mean'])
    # two launches, the same bits
    again = _launch(K, d, G, relu)
    assert all(torch.equal(got[k], again[k]) for k in got)
    # eval mode: the running statistics normalise, nothing is updated
    ref_e = linear_bn_ref(inp, G, relu, use_running=True)
    bound_e = linear_bn_bounds(inp, ref_e, G)
    got_e = _launch(K, d, G, relu, use_running=True, guarded=True)
    for k in ('out', 'xhat', 'rstd'):
        assert worst(got_e[k], ref_e[k], bound_e[k]) <= 1.0, 'use_running ' + k
    assert torch.equal(got_e['running_mean'], d['running_mean']) and torch.equal(got_e['running_var'], d['running_var'])


def test_linear_bn_single_row_in_eval_mode(K):
    inp = make_inputs(3, 1, 40, 20, True, True)
    ref = linear_bn_ref(inp, 3, True, use_running=True)
    bound = linear_bn_bounds(inp, ref, 3)
    got = _launch(K, _to_dev(inp), 3, True, use_running=True, guarded=True)
    for k in ('out', 'xhat', 'rstd'):
        assert worst(got[k], ref[k], bound[k]) <= 1.0, k


@pytest.mark.parametrize('use_running', [False, True])
@pytest.mark.parametrize('affine,relu,bias', FLAGS)
@pytest.mark.parametrize('G,R,K_,N', SHAPES)
def test_bn_bwd(K, G, R, K_, N, affine, relu, bias, use_running):
    """The backward kernel on the forward kernel's own f32 outputs against the float64 formula on the same
    values: only the rounding of its sums separates them."""
    inp = make_inputs(G, R, K_, N, affine, bias)
    d = _to_dev(inp)
    f = _launch(K, d, G, relu, use_running=use_running)
    g = torch.Generator().manual_seed(G * 1000 + N)
    dout = torch.randn(G * R, N, generator=g)
    got = K.ssl_bn_bwd(dout.to(dev), f['out'] if relu else None, f['xhat'], f['rstd'], d['gamma'], relu=relu,
                       use_running=use_running, want_affine=affine, want_bias=bias)
    again = K.ssl_bn_bwd(dout.to(dev), f['out'], f['xhat'], f['rstd'], d['gamma'], relu=relu,
                         use_running=use_running, want_affine=affine, want_bias=bias)
    c64 = lambda t: None if t is None else t.double().cpu()
    args = (dout.double(), c64(f['out']), c64(f['xhat']), c64(f['rstd']), c64(d['gamma']), relu, use_running)
    ref, bound = bn_bwd_ref(*args), bn_bwd_bounds(*args)
    want = dict(dy=True, dgamma=affine, dbeta=affine, dbias=bias)
    for (k, on), x, y in zip(want.items(), got, again):
        if not on:
            assert x is None
            continue
        assert torch.equal(x, y), k
        w = worst(x, ref[k], bound[k] + 1e-300)
        print(f'{k}: worst |d| / bound {w:.3f}')
        assert w <= 1.0, k


@pytest.mark.parametrize('affine,relu,bias', FLAGS)
@pytest.mark.parametrize('G,R,K_,N', SHAPES)
def test_linear_bn_function_gradients(G, R, K_, N, affine, relu, bias):
    """``LinearBNFn`` under autograd against float64 autograd of the restatement.  The bounds carry the
    forward's bounds (xhat, rstd, a ReLU mask that may flip where the pre-activation is within its bound of
    zero) through the backward expression, then through dX = dy W and dW = dy^T X with the chain bound
    4 n u |a| |b| of each product."""
    from ctclip_mi355x import functional as Fn
    inp = make_inputs(G, R, K_, N, affine, bias)
    d = _to_dev(inp)
    names = ('X', 'W', 'bias', 'gamma', 'beta')
    leaves = {k: (None if d[k] is None else d[k].detach().clone().requires_grad_(True)) for k in names}
    out = Fn.LinearBNFn.apply(leaves['X'], leaves['W'], leaves['bias'], leaves['gamma'], leaves['beta'],
                              d['running_mean'].clone(), d['running_var'].clone(), G, relu, EPS, MOM, False)
    gen = torch.Generator().manual_seed(N)
    Wt = torch.randn(G * R, N, generator=gen)
    (out * Wt.to(dev)).sum().backward()
    r = {k: (None if inp[k] is None else inp[k].double().clone().requires_grad_(True)) for k in names}
    ref = linear_bn_ref(dict(r, running_mean=inp['running_mean'], running_var=inp['running_var']), G, relu)
    (ref['out'] * Wt.double()).sum().backward()
    with torch.no_grad():
        ref = {k: v.detach() for k, v in ref.items()}
        fb = linear_bn_bounds(inp, ref, G)
        flip = (ref['pre'].abs() <= fb['out']).double() if relu else torch.zeros_like(ref['pre'])
        ga = inp['gamma'].double() if affine else None
        bargs = (Wt.double(), ref['out'], ref['xhat'], ref['rstd'], ga, relu, False)
        dy = bn_bwd_ref(*bargs)['dy']
        bb = bn_bwd_bounds(*bargs, d_d=flip * Wt.double().abs(), d_xhat=fb['xhat'], d_rstd=fb['rstd'])
        X64, W64, M = inp['X'].double(), inp['W'].double(), G * R
        bound = dict(X=bb['dy'] @ W64.abs() + 4 * N * U * (dy.abs() @ W64.abs()),
                     W=bb['dy'].t() @ X64.abs() + 4 * M * U * (dy.abs().t() @ X64.abs()),
                     bias=bb['dbias'], gamma=bb['dgamma'], beta=bb['dbeta'])
    for k in names:
        if r[k] is None:
            continue
        assert leaves[k].grad is not None and leaves[k].grad.shape == r[k].shape
        w = worst(leaves[k].grad, r[k].grad, bound[k] + 1e-300)
        print(f'd{k}: worst |d| / bound {w:.3f}')
        assert w <= 1.0, k


def _loss_inputs(B, P, seed=0):
    g = torch.Generator().manual_seed(100 * B + P + seed)
    return [torch.randn(B, P, generator=g) for _ in range(4)]


def _loss_bounds(p, z, B, P):
    """cos of a row: the three sums of P products are each within P u of their absolute sum, the norms and
    the quotient a few u more: |d cos| <= 4 (P + 8) u with margin 2.  loss = mean of two (2 - 2 cos) sums.
    d loss / d p = -2 / B (z^ - p^ cos) / |p|: the same relative error on a value of size (|z^| + |p^|) / |p|."""
    unit = lambda x: x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    p, z = p.double(), z.double()
    return (2.0 / B) / p.norm(dim=-1, keepdim=True).clamp_min(1e-12) * (unit(z).abs() + unit(p).abs()) * 4 * (P + 8) * U


@pytest.mark.parametrize('B,P', [(2, 4), (3, 72), (16, 256)])
def test_simsiam_loss(K, B, P):
    p1, p2, z1, z2 = _loss_inputs(B, P)
    loss, d1, d2 = K.simsiam_loss(*[t.to(dev) for t in (p1, p2, z1, z2)])
    rl, r1, r2 = simsiam_ref_grads(p1, p2, z1, z2)
    b_loss = (16 * (P + 8) + 4 * B) * U
    print(f'loss {loss.item():.8f} f64 {rl.item():.8f} |d| / bound {abs(loss.item() - rl.item()) / b_loss:.3f}')
    assert loss.shape == (1,) and abs(loss.item() - rl.item()) <= b_loss
    assert worst(d1, r1, _loss_bounds(p1, z2, B, P)) <= 1.0 and worst(d2, r2, _loss_bounds(p2, z1, B, P)) <= 1.0
    again = K.simsiam_loss(*[t.to(dev) for t in (p1, p2, z1, z2)])
    assert torch.equal(loss, again[0]) and torch.equal(d1, again[1]) and torch.equal(d2, again[2])
    # identical predictions and targets: cos = 1 up to the rounding of 1 / sqrt and two products per row
    same = K.simsiam_loss(p1.to(dev), p2.to(dev), p2.to(dev), p1.to(dev))[0]
    assert abs(same.item()) <= 32 * U
    # a zero row in p and in z: everything finite, the loss still the restatement's
    p1[1] = 0
    z1[0] = 0
    out = K.simsiam_loss(*[t.to(dev) for t in (p1, p2, z1, z2)])
    assert all(torch.isfinite(o).all() for o in out)
    assert abs(out[0].item() - simsiam_ref_grads(p1, p2, z1, z2)[0].item()) <= b_loss
    assert (out[2][0] == 0).all()                          # cos against a zero target is constant


def test_refusals(K):
    """Host-side checks of the C entry points: nothing is launched."""
    from ctclip_mi355x import _lib
    from ctclip_mi355x._lib import KernelError
    z = lambda *s: torch.zeros(*s, device=dev)
    o = lambda n: torch.ones(n, device=dev)
    with pytest.raises(KernelError, match='1003'):                  # G R > 128
        K.ssl_linear_bn(z(130, 8), z(4, 8), z(4), o(4), groups=2)
    with pytest.raises(KernelError, match='1003'):                  # R < 2 in training mode
        K.ssl_linear_bn(z(2, 8), z(4, 8), z(4), o(4), groups=2)
    K.ssl_linear_bn(z(2, 8), z(4, 8), z(4), o(4), groups=2, use_running=True)
    with pytest.raises(KernelError, match='1003'):                  # K % 4
        K.ssl_linear_bn(z(4, 6), z(4, 6), z(4), o(4), groups=2)
    with pytest.raises(KernelError, match='1003'):                  # an empty extent
        K.ssl_linear_bn(z(4, 8), z(0, 8), z(0), o(0), groups=2)
    with pytest.raises(ValueError, match='ssl_linear_bn'):
        K.ssl_linear_bn(z(5, 8), z(4, 8), z(4), o(4), groups=2)
    with pytest.raises(ValueError, match='f32|float32'):
        K.ssl_linear_bn(z(4, 8).double(), z(4, 8), z(4), o(4), groups=2)
    x, w, rm, rv = z(4, 8), z(4, 8), z(4), o(4)
    outs = [z(4, 4), z(4, 4), z(2, 4)]

    def args(**kw):
        a = _lib.SslLinearBnArgs(X=x.data_ptr(), ldx=8, W=w.data_ptr(), bias=None, gamma=None, beta=None,
                                 running_mean=rm.data_ptr(), running_var=rv.data_ptr(), G=2, R=2, K=8, N=4, relu=1,
                                 use_running=0, eps=1e-5, momentum=0.1, out=outs[0].data_ptr(),
                                 xhat=outs[1].data_ptr(), rstd=outs[2].data_ptr())
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    call = lambda a: _lib.lib().ctclip_ssl_linear_bn(_lib.ctypes.byref(a), _lib.stream_ptr())
    assert call(args()) == 0
    for name in ('X', 'W', 'running_mean', 'running_var', 'out', 'xhat', 'rstd'):
        assert call(args(**{name: None})) == 1001, name
    assert call(args(gamma=rv.data_ptr())) == 1001                   # half an affine pair
    assert call(args(G=0)) == 1003 and call(args(R=65)) == 1003 and call(args(K=0)) == 1003
    assert call(args(N=0)) == 1003 and call(args(R=1)) == 1003 and call(args(K=6)) == 1003
    assert call(args(X=x.data_ptr() + 4)) == 1002 and call(args(ldx=6)) == 1002 and call(args(ldx=4)) == 1002
    # backward
    with pytest.raises(KernelError, match='1003'):
        K.ssl_bn_bwd(z(130, 4), None, z(130, 4), o(8).view(2, 4))
    with pytest.raises(KernelError, match='1003'):
        K.ssl_bn_bwd(z(2, 4), None, z(2, 4), o(8).view(2, 4))
    with pytest.raises(KernelError, match='1001'):                  # relu without out
        K.ssl_bn_bwd(z(4, 4), None, z(4, 4), o(8).view(2, 4), relu=True)
    with pytest.raises(ValueError, match='ssl_bn_bwd'):
        K.ssl_bn_bwd(z(4, 4), None, z(4, 5), o(8).view(2, 4))
    # loss
    with pytest.raises(KernelError, match='1003'):
        K.simsiam_loss(*[z(8193, 4)] * 4)
    with pytest.raises(KernelError, match='1003'):
        K.simsiam_loss(*[z(2, 8193)] * 4)
    with pytest.raises(ValueError, match='simsiam_loss'):
        K.simsiam_loss(z(2, 4), z(2, 4), z(3, 4), z(2, 4))
    ss = _lib.lib().ctclip_simsiam_loss
    t = z(2, 4)
    assert ss(t.data_ptr(), t.data_ptr(), t.data_ptr(), None, 2, 4, t.data_ptr(), t.data_ptr(), t.data_ptr(),
              t.data_ptr(), _lib.stream_ptr()) == 1001
    assert _lib.lib().ctclip_version() == 2


def test_custom_ops(K):
    from ctclip_mi355x import functional as Fn
    from ctclip_mi355x import ops
    G, R, K_, N = 2, 3, 516, 72
    d = _to_dev(make_inputs(G, R, K_, N, True, True))
    X = d['X'].contiguous()
    names = ('W', 'bias', 'gamma', 'beta')
    a = [X.clone().requires_grad_(True)] + [d[k].clone().requires_grad_(True) for k in names]
    b = [X.clone().requires_grad_(True)] + [d[k].clone().requires_grad_(True) for k in names]
    out, rm, rv = ops.ssl_linear_bn(a[0], a[1], d['running_mean'], d['running_var'], G, a[2], a[3], a[4], True, EPS, MOM)
    rm2, rv2 = d['running_mean'].clone(), d['running_var'].clone()
    out2 = Fn.LinearBNFn.apply(b[0], b[1], b[2], b[3], b[4], rm2, rv2, G, True, EPS, MOM, False)
    assert torch.equal(out, out2) and torch.equal(rm, rm2) and torch.equal(rv, rv2)
    assert not torch.equal(rm, d['running_mean'])                    # functional: the inputs are left alone
    out.square().sum().backward()
    out2.square().sum().backward()
    for x, y in zip(a, b):
        assert x.grad is not None and torch.equal(x.grad, y.grad)
    utils = ('test_schema', 'test_faketensor', 'test_autograd_registration')
    torch.library.opcheck(torch.ops.ctclip.ssl_linear_bn,
                          (X, d['W'], d['running_mean'], d['running_var'], G, d['bias'], d['gamma'], d['beta'], True),
                          test_utils=utils)
    ps = [t.to(dev) for t in _loss_inputs(3, 72)]
    pa, pb = [t.clone().requires_grad_(True) for t in ps], [t.clone().requires_grad_(True) for t in ps]
    la, lb = ops.simsiam_loss(*pa), Fn.SimSiamLossFn.apply(*pb)
    assert la.shape == () and torch.equal(la, lb)
    (2.5 * la).backward()
    (2.5 * lb).backward()
    kl, k1, k2 = K.simsiam_loss(*ps)
    assert torch.equal(pa[0].grad, k1 * 2.5) and torch.equal(pa[1].grad, k2 * 2.5)
    assert torch.equal(pa[0].grad, pb[0].grad) and torch.equal(pa[1].grad, pb[1].grad)
    assert pa[2].grad is None and pb[3].grad is None                 # the targets are constants
    torch.library.opcheck(torch.ops.ctclip.simsiam_loss, tuple(ps), test_utils=utils)
    with pytest.raises(Exception):                                   # registered for the HIP device only
        torch.ops.ctclip.simsiam_loss(*[t.cpu() for t in ps])


# ------------------------------------------------------------------------------ model level
HIDDEN, PROJ, W_SSL = 64, 16, 0.05


def build_ssl(cfg, seed=0, **options):
    """sigmoid_loss_common.build with a VisualSSLHead (hidden 64, projection 16): the oracle's seeded weights
    for the towers, torch's seeded initialisation for the head; the heads train."""
    from oracle import weights as W
    from ctclip_mi355x.bert import BertConfig
    from ctclip_mi355x.models import build_ctclip, set_finetune_trainable
    v, b = cfg.vit, cfg.bert
    vit = dict(dim=v.dim, codebook_size=v.codebook_size, image_size=v.image_size, patch_size=v.patch_size,
               temporal_patch_size=v.temporal_patch_size, spatial_depth=v.spatial_depth,
               temporal_depth=v.temporal_depth, dim_head=v.dim_head, heads=v.heads)
    bert = BertConfig(vocab_size=b.vocab_size, hidden_size=b.hidden, num_hidden_layers=b.layers,
                      num_attention_heads=b.heads, intermediate_size=b.intermediate,
                      max_position_embeddings=b.max_position, hidden_dropout_prob=0.0,
                      attention_probs_dropout_prob=0.0)
    torch.manual_seed(100 + seed)
    m = build_ctclip(vit, bert, cfg.dim_latent, visual_ssl=dict(projection_size=PROJ, projection_hidden_size=HIDDEN),
                     image_ssl_loss_weight=W_SSL, **options)
    res = m.load_state_dict(W.make_state_dict(cfg, seed=seed), strict=False)
    assert not res.unexpected_keys and all(k.startswith('visual_ssl.') for k in res.missing_keys)
    m = set_finetune_trainable(m)
    for n, p in m.named_parameters():
        if n.startswith('visual_ssl.') or n in ('to_text_latent.weight', 'to_visual_latent.weight', 'temperature'):
            p.requires_grad = True
    return m.cuda()


def _trainer(K, seed=0):
    from ctclip_mi355x.trainer import CTClipTrainer
    K.reset_ln_status()
    torch.manual_seed(0)
    return CTClipTrainer(build_ssl(cfg_small(), seed=seed), lr=LR)


def _buffers(model):
    return {k: v.detach().clone() for k, v in model.visual_ssl.state_dict().items()}


@pytest.mark.parametrize('n_aug', [1, 2])
def test_forward_loss_is_the_weighted_sum(K, n_aug):
    """A forward hook on ``model.visual_ssl`` sees the last two views' raw latents and the loss: that loss is
    the float64 copy of the head on that input, and the total is (1 - w_ssl - w_mv) main + w_mv mean(views) +
    w_ssl ssl with the contrastive part restated in float64 on the same raw latents.  Tolerances: the project's
    1e-5 max(1, |ref|) for a contrastive loss; the head's loss (four normalised layers of at most 64 terms per
    chain, each within ~K u = 4e-6, amplified by the batch normalisation of 4 rows) 1e-4."""
    from ctclip_mi355x.augment import CTAugment
    from test_loss_options_cpu import general_loss
    cfg = cfg_small()
    K.reset_ln_status()
    model = build_ssl(cfg)
    hu, text = batch(cfg, 4)
    aug = CTAugment(seed=3).views(hu, step=0, n_views=n_aug)
    seen = {}
    handle = model.visual_ssl.register_forward_hook(lambda mod, args, out: seen.update(views=args[0].detach().clone(),
                                                                                       loss=out.detach().clone()))
    model.train()
    old = model.set_ema_mode('skip')
    try:
        with torch.no_grad():
            _, _, t_raw, i_raw = model.encode(text, torch.cat((hu, *aug), dim=0))
            t_raw, i_raw = t_raw.clone(), i_raw.clone()
            loss = model(text, hu, return_loss=True, aug_image=aug)
    finally:
        model.set_ema_mode(old)
        handle.remove()
    V, B, Dl = n_aug + 1, 4, cfg.dim_latent
    assert seen['views'].shape == (2, B, Dl)
    assert torch.allclose(seen['views'], i_raw.view(V, B, Dl)[-2:], rtol=1e-5, atol=1e-6)
    assert torch.equal(model.last_image_ssl_loss, seen['loss'].reshape(1))
    ssl_ref, _ = head_ref64(model.visual_ssl, seen['views'])
    w_mv = model.multiview_loss_weight
    cl, _ = general_loss(t_raw.double().cpu().view(1, B, Dl), i_raw.double().cpu().view(V, B, Dl),
                         model.temperature.detach().double().cpu(), w_main=1 - w_mv - W_SSL, w_multiview=w_mv)
    want = cl.item() + W_SSL * ssl_ref.item()
    print(f'ssl {seen["loss"].item():.7f} f64 {ssl_ref.item():.7f}; total {loss.item():.7f} f64 {want:.7f}')
    assert abs(seen['loss'].item() - ssl_ref.item()) <= 1e-4 * max(1.0, abs(ssl_ref.item()))
    assert abs(loss.item() - want) <= 1e-5 * max(1.0, abs(cl.item())) + W_SSL * 1e-4 * max(1.0, abs(ssl_ref.item()))
    assert ssl_ref.item() > 1e-3                                     # the term is really there


@pytest.fixture(scope='module')
def runs(K, tmp_path_factory):
    """n_views = 1: run A two ``train_step_augmented`` steps, run B one step, save, a stranger loads and takes
    the second.  n_views = 2: one step, twice."""
    from ctclip_mi355x.augment import CTAugment
    from ctclip_mi355x.trainer import CTClipTrainer
    from test_gpu_checkpoint import snapshot
    cfg = cfg_small()
    data = [batch(cfg, 2, seed=s) for s in range(2)]
    aug = CTAugment(seed=11)
    out = {}

    def state(tr):
        s = snapshot(tr)
        s['buffers'] = _buffers(tr.model)
        return s

    tr = _trainer(K)
    assert all(any(p is q for q in tr.flat.params) for p in tr.model.visual_ssl.parameters())
    out['head0'] = {n: p.detach().clone() for n, p in tr.model.visual_ssl.named_parameters()}
    out['buffers0'] = _buffers(tr.model)
    out['A_loss1'] = tr.train_step_augmented(data[0][1], data[0][0], aug, n_views=1).reshape(1).clone()
    out['A_ssl1'] = tr.model.last_image_ssl_loss.clone()
    out['A1'] = state(tr)
    out['A_loss2'] = tr.train_step_augmented(data[1][1], data[1][0], aug, n_views=1).reshape(1).clone()
    out['A2'] = state(tr)
    del tr
    tr = _trainer(K)
    out['B_loss1'] = tr.train_step_augmented(data[0][1], data[0][0], aug, n_views=1).reshape(1).clone()
    out['B1'] = state(tr)
    path = str(tmp_path_factory.mktemp('ck') / 'ssl.pt')
    tr.save(path)
    del tr
    K.reset_ln_status()
    torch.manual_seed(77)
    tr = CTClipTrainer(build_ssl(cfg, seed=7), lr=LR)
    out['stranger_differs'] = not torch.equal(tr.model.visual_ssl.projector[0].weight, out['A1']['param']
                                              ['visual_ssl.projector.0.weight'])
    out['load'] = tr.load(path)
    out['B_loss2'] = tr.train_step_augmented(data[1][1], data[1][0], aug, n_views=1).reshape(1).clone()
    out['B2'] = state(tr)
    del tr
    for tag in ('C', 'D'):
        tr = _trainer(K)
        out[tag + '_loss'] = tr.train_step_augmented(data[0][1], data[0][0], aug, n_views=2).reshape(1).clone()
        out[tag] = state(tr)
        del tr
    return out


def _assert_state_equal(a, b):
    from test_gpu_checkpoint import assert_same
    assert_same(a, b)
    assert a['buffers'].keys() == b['buffers'].keys()
    for k in a['buffers']:
        assert torch.equal(a['buffers'][k], b['buffers'][k]), k


@pytest.mark.parametrize('tag', ['A1', 'C'])
def test_train_step_moves_every_head_parameter(runs, tag):
    s = runs[tag]
    assert torch.isfinite(runs['A_loss1' if tag == 'A1' else 'C_loss']).all()
    for n, p0 in runs['head0'].items():
        p1 = s['param']['visual_ssl.' + n]
        assert torch.isfinite(p1).all() and not torch.equal(p1, p0), n
        assert torch.isfinite(s['m']['visual_ssl.' + n]).all() and s['m']['visual_ssl.' + n].abs().max() > 0, n
    for k, v in s['buffers'].items():
        assert torch.isfinite(v.float()).all(), k
        if 'running' in k:
            assert not torch.equal(v, runs['buffers0'][k]), k
        if 'num_batches_tracked' in k:
            assert v.item() == 2
    assert all(torch.isfinite(v).all() for v in s['param'].values())
    assert torch.isfinite(runs['A_ssl1']).all() and runs['A_ssl1'].shape == (1,)


def test_seeded_runs_give_the_same_bits(runs):
    assert torch.equal(runs['A_loss1'], runs['B_loss1']) and torch.equal(runs['C_loss'], runs['D_loss'])
    _assert_state_equal(runs['A1'], runs['B1'])
    _assert_state_equal(runs['C'], runs['D'])


def test_save_load_step_gives_the_bits_of_the_uninterrupted_run(runs):
    res = runs['load']
    assert runs['stranger_differs']
    assert res['step'] == 1 and not res['missing_keys'] and not res['unexpected_keys'] and res['hyper_mismatch'] == {}
    assert torch.equal(runs['A_loss2'], runs['B_loss2'])
    _assert_state_equal(runs['A2'], runs['B2'])
    assert any('running_var' in k for k in runs['A2']['buffers'])


def test_model_refusals(K):
    from ctclip_mi355x.trainer import CTClipTrainer
    cfg = cfg_small(layers=1)
    K.reset_ln_status()
    model = build_ssl(cfg)
    hu, text = batch(cfg, 2)
    with pytest.raises(ValueError, match='visual_ssl needs aug_image'):
        model(text, hu, return_loss=True)
    model.eval()
    with torch.no_grad():
        assert model(text, hu).shape == (2,)                         # without return_loss nothing changes
    tr = CTClipTrainer(model, lr=LR)
    with pytest.raises(NotImplementedError, match='visual_ssl is not chunked'):
        tr.train_step_chunked(text, hu, 1)
    with pytest.raises(NotImplementedError, match='visual_ssl with sigmoid_loss'):
        build_ssl(cfg, sigmoid_loss=True)
