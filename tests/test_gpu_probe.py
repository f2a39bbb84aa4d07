"""The linear-probe head on the GPU: ctclip_probe_step (csrc/probe.hip) against the float64 torch restatement
``probe.step_reference`` on the same f32 operands, its reproducibility and contract, ``LinearProbe.fit`` on the
device against the float64 host loop, and ``CTClipTrainer.linear_probe`` end to end.

Tolerances: both products are f32 fma chains (exact f32 operands on the matrix pipe), so Z, dW and db get the
project's bound for f32-accumulated products, 1e-5 relative Frobenius (tests/test_gpu_gemm.py,
tests/test_gpu_mlm.py); the loss 1e-5 * max(1, |loss|); the count is exact.  Measured maxima over the cases
below are recorded in DESIGN.md section 25."""
import functools
import types

import pytest
import torch

from oracle import ctclip_oracle as O
from oracle import weights as W

pytestmark = pytest.mark.gpu

F64 = torch.float64
TOL = 1e-5


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


# (M, D, P, pos_weight, 255s, idx): every M, D, P of the contract's corners at least once; M = 4096 has more
# tiles than workgroups, M <= 65 fewer tiles than a second workgroup would need
CASES = [
    (1, 16, 1, False, False, False),
    (31, 64, 17, True, True, False),
    (32, 512, 18, False, False, True),
    (33, 1024, 32, True, True, True),
    (65, 64, 18, True, False, True),
    (257, 512, 17, False, True, False),
    (4096, 16, 1, True, True, False),
    (4096, 512, 32, False, True, True),
]


@functools.lru_cache(maxsize=None)
def _case(M, D, P, with_pw, with_255, with_idx, w_scale=0.5):
    """Operands on the device (X a [N, D] view of rows D + 16 wide) and the float64 reference, made once."""
    from ctclip_mi355x import probe as PR
    g = torch.Generator().manual_seed(1000 * M + 10 * D + P)
    N = M + 9 if with_idx else M
    buf = torch.randn(N, D + 16, generator=g)
    buf[:, :D] /= buf[:, :D].norm(dim=1, keepdim=True)
    Wt = torch.randn(P, D, generator=g) * w_scale * D ** 0.5
    b = torch.randn(P, generator=g) * 0.3
    Y = (torch.rand(N, P, generator=g) < 0.35).to(torch.uint8)
    if with_255:
        Y[torch.rand(N, P, generator=g) < 0.2] = 255
        if P > 1:
            Y[:, P // 2] = 255                                        # one column never labelled
        Y[N // 2] = 255                                               # one row never labelled
    pw = torch.rand(P, generator=g) * 3 + 0.25 if with_pw else None
    idx = torch.randint(0, N, (M,), generator=g, dtype=torch.int32) if with_idx else None
    if idx is not None and M >= 4:
        idx[1] = idx[0]                                               # a repeat for certain
        idx[2] = N // 2                                               # ... and the unlabelled row
    X = buf[:, :D]
    ref = PR.step_reference(X.double(), Wt.double(), b.double(), Y, idx, None if pw is None else pw.double())
    dev = [None if t is None else t.cuda() for t in (buf, Wt, b, Y, pw, idx)]
    return (dev[0][:, :D],) + tuple(dev[1:]), ref


def _check(res, ref, tag):
    dl = abs(float(res['loss']) - float(ref['loss']))
    errs = {k: _rel(res[k], ref[k]) for k in ('Z', 'dW', 'db') if float(ref[k].norm()) > 0}
    print(f'{tag}: |dloss| {dl:.3e} (loss {float(ref["loss"]):.6f})', {k: f'{v:.3e}' for k, v in errs.items()})
    assert int(res['count']) == int(ref['count'])
    assert dl <= TOL * max(1.0, abs(float(ref['loss'])))
    for k, v in errs.items():
        assert v <= TOL, (k, v)
    for k in ('Z', 'dW', 'db'):
        assert bool(torch.isfinite(res[k]).all())
        if float(ref[k].norm()) == 0:
            assert not res[k].any(), k


ALL = ('loss', 'dW', 'db', 'Z', 'count')


@pytest.mark.parametrize('case', CASES, ids=lambda c: 'M{}-D{}-P{}-pw{:d}-u{:d}-idx{:d}'.format(*c))
def test_step_matches_float64(case):
    from ctclip_mi355x import kernels as K
    (X, Wt, b, Y, pw, idx), ref = _case(*case)
    assert X.stride(0) == case[1] + 16
    res = K.probe_step(X, Wt, b, Y, idx=idx, pos_weight=pw, want=ALL)
    _check(res, ref, str(case))
    if case[4] and case[2] > 1:                                       # the unlabelled column has no gradient
        assert not res['dW'][case[2] // 2].any() and float(res['db'][case[2] // 2]) == 0.0


def test_nothing_counted_gives_zeros():
    from ctclip_mi355x import kernels as K
    (X, Wt, b, Y, pw, idx), _ = _case(65, 64, 18, True, False, True)
    res = K.probe_step(X, Wt, b, torch.full_like(Y, 255), idx=idx, pos_weight=pw, want=ALL)
    assert int(res['count']) == 0 and float(res['loss']) == 0.0 and not res['dW'].any() and not res['db'].any()


@pytest.mark.parametrize('P', [3, 18])
def test_extreme_logits_are_finite(P):
    """W scaled so that logits of +-80 occur: the stable formula neither overflows nor loses the bound."""
    from ctclip_mi355x import kernels as K
    from ctclip_mi355x import probe as PR
    g = torch.Generator().manual_seed(7)
    X = torch.randn(96, 64, generator=g)
    X /= X.norm(dim=1, keepdim=True)
    sign = torch.where(torch.arange(P) % 2 == 0, 1.0, -1.0)[:, None]
    Wt = 80.0 * sign * X[:P] / (X[:P] * X[:P]).sum(1, keepdim=True)
    b = torch.zeros(P)
    Y = (torch.rand(96, P, generator=g) < 0.5).to(torch.uint8)
    pw = torch.rand(P, generator=g) * 3 + 0.25
    ref = PR.step_reference(X.double(), Wt.double(), b.double(), Y, None, pw.double())
    assert float(ref['Z'].max()) >= 79.99 and float(ref['Z'].min()) <= -79.99
    res = K.probe_step(X.cuda(), Wt.cuda(), b.cuda(), Y.cuda(), pos_weight=pw.cuda(), want=ALL)
    assert all(bool(torch.isfinite(res[k]).all()) for k in ALL if k != 'count')
    _check(res, ref, f'logits +-80, P {P}')


def test_bit_reproducible():
    from ctclip_mi355x import kernels as K
    (X, Wt, b, Y, pw, idx), _ = _case(4096, 512, 32, False, True, True)
    a = K.probe_step(X, Wt, b, Y, idx=idx, pos_weight=pw, want=ALL)
    c = K.probe_step(X, Wt, b, Y, idx=idx, pos_weight=pw, want=ALL)
    junk = torch.full((3_000_001,), 3.0, device='cuda')               # an unrelated allocation in between
    d = K.probe_step(X, Wt, b, Y, idx=idx, pos_weight=pw, want=ALL)
    for k in ALL:
        assert torch.equal(a[k], c[k]) and torch.equal(a[k], d[k]), k
    assert float(junk[0]) == 3.0


def test_logits_only_call_touches_nothing_else():
    from ctclip_mi355x import _lib
    from ctclip_mi355x import kernels as K
    (X, Wt, b, Y, pw, idx), _ = _case(257, 512, 17, False, True, False)
    full = K.probe_step(X, Wt, b, Y, pos_weight=pw, want=ALL)
    poison = {k: torch.full_like(full[k], 12345.0) for k in ('loss', 'dW', 'db')}
    z = K.probe_step(X, Wt, b, None, want=('Z',), out=dict(poison))   # the others are not wanted: not passed on
    assert list(z) == ['Z'] and torch.equal(z['Z'], full['Z'])
    for k, v in poison.items():
        assert bool((v == 12345.0).all()), k
    # the C entry itself: Z only, with a workspace on offer -- the workspace stays as it was
    M, D, P = 257, 512, 17
    Z = torch.empty(M, P, device='cuda')
    a = _lib.ProbeArgs(X=X.data_ptr(), ldx=X.stride(0), N=M, idx=None, M=M, D=D, P=P, W=Wt.data_ptr(),
                       b=b.data_ptr(), Y=Y.data_ptr(), Z=Z.data_ptr())
    n = _lib.lib().ctclip_probe_step_ws_bytes(_lib.ctypes.byref(a))
    assert n > 0 and n % 16 == 0
    ws = torch.full((n // 4,), 12345.0, device='cuda')
    a.ws, a.ws_bytes = ws.data_ptr(), n
    _lib.call('ctclip_probe_step', _lib.ctypes.byref(a), _lib.stream_ptr())
    assert torch.equal(Z, full['Z']) and bool((ws == 12345.0).all())
    # and the forward of the module is that path
    from ctclip_mi355x.probe import LinearProbe
    pr = LinearProbe(D, P, device='cuda')
    with torch.no_grad():
        pr.weight.copy_(Wt)
        pr.bias.copy_(b)
    Xc = X.contiguous()
    assert torch.equal(pr(Xc), K.probe_step(Xc, Wt, b, None, want=('Z',))['Z'])
    assert _rel(pr(Xc), full['Z']) <= TOL


def test_contract_violations_raise_before_any_launch():
    from ctclip_mi355x import _lib
    from ctclip_mi355x import kernels as K
    dev = 'cuda'
    X, Y = torch.randn(8, 32, device=dev), torch.zeros(8, 3, dtype=torch.uint8, device=dev)
    Wt, b = torch.zeros(3, 32, device=dev), torch.zeros(3, device=dev)
    K.probe_step(X, Wt, b, Y)                                                           # the valid call
    bad = [
        dict(W=torch.zeros(33, 32, device=dev), b=torch.zeros(33, device=dev),
             Y=torch.zeros(8, 33, dtype=torch.uint8, device=dev)),                      # P = 33
        dict(X=torch.randn(8, 24, device=dev), W=torch.zeros(3, 24, device=dev)),        # D = 24
        dict(X=torch.randn(8, 2048, device=dev), W=torch.zeros(3, 2048, device=dev)),    # D > 1024
        dict(idx=torch.zeros(0, dtype=torch.int32, device=dev)),                        # M = 0
        dict(idx=torch.zeros(4, dtype=torch.int64, device=dev)),                        # idx dtype
        dict(X=X.double()),                                                             # wrong dtype
        dict(Y=Y.float()),
        dict(W=torch.zeros(32, 3, device=dev).t()),                                     # non-contiguous W
        dict(X=torch.randn(8, 66, device=dev)[:, :32][:, ::1].t().contiguous().t()),    # column-major X
        dict(want=('loss', 'logits')),
    ]
    for kw in bad:
        args = dict(X=X, W=Wt, b=b, Y=Y)
        args.update(kw)
        with pytest.raises(ValueError):
            K.probe_step(args.pop('X'), args.pop('W'), args.pop('b'), args.pop('Y'), **args)
    # the C entry refuses the same shapes with a status, not a launch
    for M, D, P in ((0, 32, 3), (8, 24, 3), (8, 32, 33), (8, 2048, 3)):
        a = _lib.ProbeArgs(X=X.data_ptr(), ldx=32, N=max(M, 1), M=M, D=D, P=P, W=Wt.data_ptr(), b=b.data_ptr(),
                           Y=Y.data_ptr(), loss=b.data_ptr())
        assert _lib.lib().ctclip_probe_step_ws_bytes(_lib.ctypes.byref(a)) == 0
        assert _lib.lib().ctclip_probe_step(_lib.ctypes.byref(a), _lib.stream_ptr()) == 1003
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------ fit
@functools.lru_cache(maxsize=None)
def _fit_problem():
    g = torch.Generator().manual_seed(21)
    X = torch.randn(512, 64, generator=g)
    X /= X.norm(dim=1, keepdim=True)
    Y = ((X @ torch.randn(64, 18, generator=g) + 0.05 * torch.randn(512, 18, generator=g)) > 0.02).to(torch.uint8)
    return X, Y


def _host_fit(dtype, **kw):
    from ctclip_mi355x.probe import LinearProbe
    X, Y = _fit_problem()
    pr = LinearProbe(64, 18, dtype=dtype)
    loss = pr.fit(X.to(dtype), Y, steps=20, lr=1e-2, **kw)
    return pr, loss


@pytest.mark.parametrize('kw', [dict(), dict(wd=0.1), dict(pos_weight='balanced')], ids=['adam', 'adamw', 'balanced'])
def test_fit_follows_the_float64_trajectory(kw):
    """20 steps on the device against step_reference + torch.optim.Adam / AdamW in float64 on the host.  The
    bound is not a fixed number: torch's own float32 host run of the same loop is another f32 rounding of the
    same recurrence, and the device may be 4 x as far from the float64 trajectory as that run is (the
    factor covers the different summation order).  With 'balanced' the bias gradient of the zero-initialised
    probe vanishes identically (the weighted positives cancel the negatives) and Adam turns the rounding noise
    left there into +-lr steps, in every precision with its own signs: both distances are then of order 1e-4
    to 1e-3 instead of 1e-7, and the bound, being relative to the host's own, still holds."""
    from ctclip_mi355x.probe import LinearProbe
    X, Y = _fit_problem()
    p64, l64 = _host_fit(F64, **kw)
    p32, _ = _host_fit(torch.float32, **kw)
    pr = LinearProbe(64, 18, device='cuda')
    loss = pr.fit(X.cuda(), Y.cuda(), steps=20, lr=1e-2, **kw)
    assert loss.is_cuda and loss.shape == (20,) and bool((loss[1:] < loss[:-1]).all())
    d_host = _rel(p32.weight, p64.weight)
    d_dev = _rel(pr.weight, p64.weight)
    print(f'fit {kw}: device {d_dev:.3e}, host f32 {d_host:.3e} from float64; bias {_rel(pr.bias, p64.bias):.3e} '
          f'vs {_rel(p32.bias, p64.bias):.3e}; loss {_rel(loss, l64):.3e}')
    assert d_dev <= 4 * d_host
    assert _rel(loss, l64) <= TOL
    if 'wd' in kw:                                                    # the bias is not decayed: it follows the
        assert _rel(pr.bias, p64.bias) <= 1e-4                        # float64 bias of the SAME (decayed-weight) run
        plain, _ = _host_fit(F64)
        assert _rel(p64.weight, plain.weight) > 1e-3                  # ... and the decay did act on the weight


# ------------------------------------------------------------------------------------------ trainer
def test_trainer_linear_probe_end_to_end():
    from test_gpu_model import build, cfg_small
    from ctclip_mi355x import kernels as K
    from ctclip_mi355x.probe import LinearProbe, LinearProbeEvaluator
    from ctclip_mi355x.trainer import CTClipTrainer, EvalGuardError, StepGuardError
    torch.manual_seed(0)
    cfg = cfg_small()
    model = build(cfg)
    video = O.normalize_hu(W.make_hu(16, cfg.vit)).cuda()
    ids, mask = W.make_text(2, 32, cfg.bert.vocab_size, ragged=True)
    text = types.SimpleNamespace(input_ids=ids.cuda(), attention_mask=mask.cuda())
    K.reset_ln_status()
    tr = CTClipTrainer(model, lr=1e-3)
    tr.train_step(text, video[:2])
    tr.flush()
    # labels: the sign of a fixed projection of the volumes' own (centred) latents
    lat = LinearProbeEvaluator(model).encode(video, batch_size=4)
    assert lat.shape == (16, 512) and lat.dtype == torch.float32
    assert torch.allclose(lat.norm(dim=1), torch.ones(16, device='cuda'), atol=1e-5)
    proj = torch.randn(512, 3, generator=torch.Generator().manual_seed(5)).cuda()
    labels = (((lat - lat.mean(0)) @ proj) > 0).to(torch.uint8)
    assert bool(((labels.sum(0) > 0) & (labels.sum(0) < 16)).all())
    word = K.status_word(video.device)
    snap = word.clone()
    assert model.training
    res = tr.linear_probe(video, labels, video, labels, n_boot=4, curves=True, batch_size=4, steps=300, lr=5e-2)
    print('linear probe: auroc', res['auroc'].tolist(), 'fit loss', float(res['fit_loss'][0]), '->',
          float(res['fit_loss'][-1]))
    assert list(res) == ['probs', 'auroc', 'ci', 'f1_micro', 'flat_accuracy', 'curves', 'curves_ci', 'probe',
                         'fit_loss']
    assert bool((res['auroc'] == 1.0).all()), res['auroc']
    assert isinstance(res['probe'], LinearProbe) and res['fit_loss'].shape == (300,) and res['fit_loss'].is_cuda
    assert res['probs'].shape == (16, 3) and res['ci'].shape == (3, 3)
    assert torch.equal(res['probs'], res['probe'].predict_proba(lat))
    assert model.training and torch.equal(word, snap)
    # a flagged volume: EvalGuardError, the status word and the mode put back, training unaffected
    bad = video[:2].clone()
    bad[1, 0, 17, 33, 71] = float('nan')
    for args in ((video, labels, bad, labels[:2]), (bad, labels[:2], video, labels)):
        with pytest.raises(EvalGuardError) as ei:
            tr.linear_probe(*args, batch_size=4, steps=5)
        assert isinstance(ei.value, StepGuardError) and ei.value.bits != 0
        assert torch.equal(word, snap) and model.training
    before = tr.flat.data.clone()
    loss = tr.train_step(text, video[:2])
    tr.check()
    assert torch.isfinite(loss) and not torch.equal(before, tr.flat.data)
    model.eval()
    tr.linear_probe(video[:4], labels[:4], video[:4], labels[:4], batch_size=4, steps=5)
    assert not model.training
    model.train()
