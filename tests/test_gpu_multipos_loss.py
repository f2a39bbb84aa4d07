"""The multi-positive (duplicate-report-aware) InfoNCE loss on the GPU (csrc/loss_multipos.hip,
ctclip_multipos_loss and ctclip_report_ids) against the torch restatement of
multipos_loss_common.py evaluated in float64, and the option through the autograd Function, the custom op,
CTCLIP.forward, the trainer, the chunked step and the checkpoint.

Tolerances are the project's own for its losses (test_gpu_sigmoid_loss.py): loss 1e-5 max(1, |ref|), every
gradient and d loss / d log-temp 1e-4 relative (norm of the difference over the norm of the reference); the
positive count is exact.  Tile sizes of the kernels: 64 rows / columns (logits and gradient rows), 128 latent
columns per gradient tile, K steps of 16, workspace rows padded to 4 -- hence Bg 63 / 64 / 65 / 127 / 128 /
129 and Dl 2 / 100 / 127 / 129 below."""
import math

import pytest
import torch

from multipos_loss_common import (ID_PATTERNS, LOG_TEMPS, OBSERVED, check, duplicate_batch, id_pattern,
                                  multipos_loss, positive_count, ref64, rel, report_ids)
from sigmoid_loss_common import batch, build, cfg_small

pytestmark = pytest.mark.gpu
dev = 'cuda'
LR = 1e-3
LT10 = math.log(10.0)


@pytest.fixture(scope='module')
def K():
    from ctclip_mi355x import kernels
    return kernels


def _inputs(Bg, Dl, seed=0):
    g = torch.Generator(device=dev).manual_seed(1000 * Bg + Dl + seed)
    return torch.randn(Bg, Dl, device=dev, generator=g), torch.randn(Bg, Dl, device=dev, generator=g)


def _lt(lt):
    return torch.tensor([lt], device=dev)


# ------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize('Dl', [2, 64, 100, 127, 129, 512])
@pytest.mark.parametrize('Bg', [1, 2, 3, 8, 63, 64, 65, 127, 128, 129, 257, 300])
def test_kernel_matches_float64(K, Bg, Dl):
    """One tile, the tile edges +-1, several ragged tiles in both directions, the K / Dl tails; every id
    pattern at every temperature on the same latents."""
    t, i = _inputs(Bg, Dl)
    for kind in ID_PATTERNS:
        ids = id_pattern(kind, Bg)
        for lt in LOG_TEMPS:
            ltt = _lt(lt)
            check(K.multipos_loss(t, i, ids.to(dev), ltt), ref64(t, i, ids, ltt), f'Bg {Bg} Dl {Dl} {kind} {lt:.3f}')
    print('observed maxima so far', {k: f'{v:.2e}' for k, v in OBSERVED.items()})


@pytest.mark.parametrize('kind', ID_PATTERNS)
def test_kernel_matches_float64_1024(K, kind):
    t, i = _inputs(1024, 512)
    ids, ltt = id_pattern(kind, 1024), _lt(LT10)
    check(K.multipos_loss(t, i, ids.to(dev), ltt), ref64(t, i, ids, ltt), f'Bg 1024 {kind}')


@pytest.mark.parametrize('lt', LOG_TEMPS)
def test_all_ids_distinct_is_the_infonce_kernels(K, lt):
    """With all ids distinct the loss is InfoNCE: against the one-workgroup kernel (Bg = 100), the tiled
    kernel (Bg = 300) and ``ClipLossFn``, within the tolerances (not bit for bit: the formulas differ by the
    1e-20 terms and the subtracted maximum)."""
    from ctclip_mi355x import functional as Fn
    ltt = _lt(lt)
    for Bg in (100, 300):
        t, i = _inputs(Bg, 512, seed=2)
        out = K.multipos_loss(t, i, id_pattern('distinct', Bg).to(dev), ltt)
        assert out[4].item() == 0
        if Bg > 128:
            loss, dt, di, _, _, dlt, _ = K.clip_loss_tiled(t[None], i[None], ltt)
            dt, di = dt[0], di[0]
        else:
            loss, dt, di, dlt = K.clip_loss(t, i, ltt)[:4]
        print(f'Bg {Bg}: multipos {out[0].item():.7f} InfoNCE {loss.item():.7f}; rel dt {rel(out[1], dt):.2e} '
              f'di {rel(out[2], di):.2e} dlt {rel(out[3], dlt):.2e}')
        assert abs(out[0].item() - loss.item()) < 1e-5 * max(1.0, abs(loss.item()))
        assert rel(out[1], dt) < 1e-4 and rel(out[2], di) < 1e-4 and rel(out[3], dlt) < 1e-4
        fn = Fn.ClipLossFn.apply(t, i, ltt[0])
        assert abs(out[0].item() - fn.item()) < 1e-5 * max(1.0, abs(fn.item()))


def test_finite_at_temperature_100(K):
    """exp(tau) = 100 (a plain exp(x) overflows f32 at 89): random latents; a row whose every cosine is -1;
    a row whose positive cosine is -1 while its negative cosines are +1; a duplicate group.  Loss and all
    gradients are finite and within the tolerances against float64."""
    Bg, Dl = 70, 96
    ltt = _lt(math.log(100.0))
    t, i = _inputs(Bg, Dl, seed=3)
    ids = id_pattern('pair_tile', Bg)
    check(K.multipos_loss(t, i, ids.to(dev), ltt), ref64(t, i, ids, ltt), 'temp 100 random')
    # every image latent is a positive multiple of u and text 3 a negative one: every cosine of row 3 is -1
    u = torch.randn(Dl, device=dev)
    i2 = u.repeat(Bg, 1) * torch.linspace(0.5, 2.0, Bg, device=dev)[:, None]
    t2 = t.clone()
    t2[3] = -3.0 * u
    out = K.multipos_loss(t2, i2, ids.to(dev), ltt)
    check(out, ref64(t2, i2, ids, ltt), 'temp 100 row of -1')
    # row 7: its positive (column 7) at cosine -1, every negative at +1: x = -100 against +100
    t3, i3 = t.clone(), u.repeat(Bg, 1).clone()
    t3[7] = u
    i3[7] = -u
    x = 100.0 * torch.nn.functional.normalize(t3[7].double(), dim=0) @ torch.nn.functional.normalize(i3.double(), dim=-1).t()
    assert x[7].item() < -99.99 and x[torch.arange(Bg, device=dev) != 7].min().item() > 99.99
    out = K.multipos_loss(t3, i3, id_pattern('distinct', Bg).to(dev), ltt)
    check(out, ref64(t3, i3, id_pattern('distinct', Bg), ltt), 'temp 100 positive -1, negatives +1')
    assert out[0].item() > 1.0


def test_zero_norm_rows_give_finite_gradients(K):
    """A zero latent row (norm below 1e-12) takes the g / max(n, 1e-12) branch of the l2norm backward, as in
    the other loss kernels: everything stays finite and the loss is the restatement's."""
    t, i = _inputs(130, 64, seed=9)
    t[1] = 0
    i[129] = 0
    ids, ltt = id_pattern('random', 130), _lt(LT10)
    out = K.multipos_loss(t, i, ids.to(dev), ltt)
    assert all(torch.isfinite(x).all() for x in out[:4])
    ref = ref64(t, i, ids, ltt)
    assert abs(out[0].item() - ref[0].item()) < 1e-5 * max(1.0, abs(ref[0].item()))
    assert out[4].item() == ref[4].item()


def test_bit_reproducible(K):
    t, i = _inputs(300, 512, seed=5)
    ids, ltt = id_pattern('random', 300).to(dev), _lt(LT10)
    a = K.multipos_loss(t, i, ids, ltt)
    b = K.multipos_loss(t, i, ids, ltt)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_row_ranges_give_the_bits_of_the_full_call(K):
    """A row's gradient does not depend on the range it was asked in; the scalars are always global."""
    Bg = 300
    t, i = _inputs(Bg, 512, seed=6)
    ids, ltt = id_pattern('random', Bg), _lt(math.log(1 / 0.07))
    full = K.multipos_loss(t, i, ids.to(dev), ltt)
    check(full, ref64(t, i, ids, ltt))
    for row0, n in [(0, Bg), (37, 16), (Bg - 1, 1), (128, 128)]:
        out = K.multipos_loss(t, i, ids.to(dev), ltt, rows=(row0, n))
        assert torch.equal(out[0], full[0]) and torch.equal(out[3], full[3]) and torch.equal(out[4], full[4])
        for g, f in zip(out[1:3], full[1:3]):
            assert g.shape == (n, f.shape[1])
            assert torch.equal(g, f[row0:row0 + n]), (row0, n)


def test_refusals(K):
    """Host-side checks of the wrapper and the C entry point: nothing is launched."""
    from ctclip_mi355x import _lib
    from ctclip_mi355x._lib import KernelError
    t, i = _inputs(8, 64)
    ltt = _lt(1.0)
    ids = torch.arange(8, device=dev)
    for rows in [(0, 9), (8, 1), (-1, 2), (3, 0)]:
        with pytest.raises(ValueError, match='rows'):
            K.multipos_loss(t, i, ids, ltt, rows=rows)
    with pytest.raises(ValueError, match='f32'):
        K.multipos_loss(t.double(), i.double(), ids, ltt)
    with pytest.raises(ValueError, match='contiguous'):
        K.multipos_loss(t.t().contiguous().t(), i, ids, ltt)
    with pytest.raises(ValueError, match='latent sets'):
        K.multipos_loss(t, i[:7], ids, ltt)
    with pytest.raises(ValueError, match='latent sets'):
        K.multipos_loss(t[None], i[None], ids, ltt)
    with pytest.raises(ValueError, match='int64'):
        K.multipos_loss(t, i, ids.int(), ltt)
    with pytest.raises(ValueError, match='int64'):
        K.multipos_loss(t, i, ids[:7], ltt)
    z = lambda *s: torch.zeros(*s, device=dev)
    with pytest.raises(KernelError, match='1003'):        # CT_ESHAPE
        K.multipos_loss(z(8193, 4), z(8193, 4), torch.arange(8193, device=dev), ltt)
    with pytest.raises(KernelError, match='1003'):
        K.multipos_loss(z(2, 8193), z(2, 8193), ids[:2].contiguous(), ltt)
    o = [torch.empty_like(t) for _ in range(2)]
    s = [torch.empty(1, device=dev) for _ in range(2)]
    npos = torch.empty(1, device=dev, dtype=torch.int32)
    ws = torch.empty(1 << 16, device=dev)

    def args(**kw):
        a = _lib.MultiposLossArgs(t_raw=t.data_ptr(), i_raw=i.data_ptr(), ids=ids.data_ptr(), log_temp=ltt.data_ptr(),
                                  Bg=8, Dl=64, grad_row0=0, grad_rows=8, loss=s[0].data_ptr(), dt_raw=o[0].data_ptr(),
                                  di_raw=o[1].data_ptr(), dlogtemp=s[1].data_ptr(), npos=npos.data_ptr(),
                                  ws=ws.data_ptr(), ws_bytes=4 * ws.numel())
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    call = lambda a: _lib.lib().ctclip_multipos_loss(_lib.ctypes.byref(a), _lib.stream_ptr())
    nbytes = lambda a: _lib.lib().ctclip_multipos_loss_ws_bytes(_lib.ctypes.byref(a))
    assert call(args(grad_row0=1)) == 1001
    assert call(args(grad_rows=0)) == 1001
    assert call(args(ws_bytes=64)) == 1001
    assert call(args(ids=None)) == 1001 and call(args(npos=None)) == 1001
    assert call(args(Bg=8193)) == 1003 and call(args(Dl=0)) == 1003
    assert call(args(ws=ws.data_ptr() + 4)) == 1002
    assert nbytes(args(Bg=8193)) == 0
    assert 0 < nbytes(args()) <= 4 * ws.numel() and call(args()) == 0
    # the stored matrix of the largest batch does not fit 32 bits
    assert nbytes(args(Bg=8192, Dl=512)) > 2 ** 28
    assert _lib.lib().ctclip_version() == 2
    rid = lambda *a: _lib.lib().ctclip_report_ids(*a, _lib.stream_ptr())
    tok = torch.ones(2, 4, device=dev, dtype=torch.int64)
    out = torch.empty(2, device=dev, dtype=torch.int64)
    assert rid(tok.data_ptr(), tok.data_ptr(), 0, 4, out.data_ptr()) == 1003
    assert rid(tok.data_ptr(), tok.data_ptr(), 2, 0, out.data_ptr()) == 1003
    assert rid(None, tok.data_ptr(), 2, 4, out.data_ptr()) == 1001
    assert rid(tok.data_ptr(), tok.data_ptr(), 2, 4, out.data_ptr()) == 0


# ------------------------------------------------------------------------------ report ids
@pytest.mark.parametrize('L', [1, 4, 512])
@pytest.mark.parametrize('B', [1, 8])
def test_report_ids_equal_the_python_restatement(K, B, L):
    g = torch.Generator().manual_seed(31 * B + L)
    tok = torch.randint(0, 30000, (B, L), generator=g, dtype=torch.int64)
    mask = (torch.rand(B, L, generator=g) < 0.7).to(torch.int64)
    mask[0] = 1
    if B > 1:
        tok[1, 0] = -5                       # any int64 is hashed as its 64-bit pattern
        mask[B - 1] = 0                      # an all-masked row has a defined id
    out = K.report_ids(tok.to(dev), mask.to(dev))
    assert out.dtype == torch.int64 and out.shape == (B,)
    assert torch.equal(out.cpu(), report_ids(tok, mask))
    assert torch.equal(K.report_ids(tok.to(dev).int(), mask.to(dev).bool().to(torch.uint8)).cpu(), out.cpu())
    if B > 1:
        assert out[B - 1].item() == 0


def test_report_ids_see_the_kept_sequence_only(K):
    L = 130
    g = torch.Generator().manual_seed(5)
    row = torch.randint(1, 30000, (L,), generator=g, dtype=torch.int64)
    mask = torch.ones(L, dtype=torch.int64)
    mask[100:] = 0
    tok = row.repeat(6, 1)
    m = mask.repeat(6, 1)
    tok[1, 100:] = 7                          # differs only behind the mask
    tok[2, 70] += 1                           # one kept token differs
    tok[3, 63], tok[3, 64] = row[64], row[63]  # two kept tokens swapped (across the wave's 64-token step)
    m[4, 99] = 0                              # kept length differs
    m[5, 100] = 1
    out = K.report_ids(tok.to(dev), m.to(dev)).cpu()
    assert torch.equal(out, report_ids(tok, m))
    assert out[1] == out[0]
    assert len({int(v) for v in out[[0, 2, 3, 4, 5]]}) == 5


# ------------------------------------------------------------------------------ autograd Function, custom op
def _leaves(*xs):
    return [x.detach().clone().requires_grad_(True) for x in xs]


@pytest.mark.parametrize('Bg', [8, 130])
def test_function_backward_is_the_kernel_outputs_times_the_upstream_gradient(K, Bg):
    """``MultiPosLossFn.backward`` under an upstream gradient of 2.5: the kernel's outputs scaled (bit for
    bit: one f32 product each), and the float64 gradient of 2.5 L within the tolerances."""
    from ctclip_mi355x import functional as Fn
    t, i = _inputs(Bg, 512, seed=12)
    ids = id_pattern('random', Bg)
    lt0 = torch.tensor(LT10, device=dev)
    a = _leaves(t, i, lt0)
    loss, npos = Fn.MultiPosLossFn.apply(a[0], a[1], ids.to(dev), a[2])
    (2.5 * loss).backward()
    out = K.multipos_loss(t, i, ids.to(dev), lt0.reshape(1))
    assert torch.equal(loss.detach().reshape(1), out[0]) and torch.equal(npos, out[4])
    assert not npos.requires_grad and npos.item() == positive_count(ids)
    for x, g in zip(a, out[1:4]):
        assert x.grad.shape == x.shape and torch.equal(x.grad, (g * 2.5).reshape(x.shape))
    r = _leaves(*[x.double().cpu() for x in (t, i, lt0)])
    (2.5 * multipos_loss(r[0], r[1], ids, r[2])).backward()
    for x, y in zip(a, r):
        assert rel(x.grad, y.grad) < 1e-4
    # all rows from the one call, for the chunked step
    allrows = Fn.multipos_loss_all_rows(t, i, ids.to(dev), lt0)
    for x, y in zip(allrows, out):
        assert torch.equal(x, y)


def test_custom_op(K):
    from torch._subclasses.fake_tensor import FakeTensorMode
    from ctclip_mi355x import ops
    t, i = _inputs(130, 512, seed=14)
    ids = id_pattern('random', 130)
    ltt = _lt(math.log(1 / 0.07))
    a = _leaves(t, i, ltt)
    loss = ops.multipos_loss(a[0], a[1], ids.to(dev), a[2])
    r = _leaves(*[x.double().cpu() for x in (t, i, ltt)])
    rl = multipos_loss(r[0], r[1], ids, r[2])
    assert abs(loss.item() - rl.item()) < 1e-5 * max(1.0, abs(rl.item()))
    (2.0 * loss).backward()
    (2.0 * rl).backward()
    for x, y in zip(a, r):
        assert x.grad.shape == x.shape and rel(x.grad, y.grad) < 1e-4
    utils = ('test_schema', 'test_faketensor', 'test_autograd_registration')
    torch.library.opcheck(torch.ops.ctclip.multipos_loss, (t, i, ids.to(dev), ltt), test_utils=utils)
    with FakeTensorMode():
        ft, fs = torch.empty(8, 512, device=dev), torch.empty(1, device=dev)
        fi = torch.empty(8, device=dev, dtype=torch.int64)
        out = torch.ops.ctclip.multipos_loss(ft, ft, fi, fs)
        assert out[0].shape == () and out[1].shape == out[2].shape == ft.shape and out[3].shape == (1,)
        assert out[4].shape == (1,) and out[4].dtype == torch.int32
    with pytest.raises(Exception):      # registered for the HIP device only
        torch.ops.ctclip.multipos_loss(t.cpu(), i.cpu(), ids, ltt.cpu())


# ------------------------------------------------------------------------------ model level
def _trainer(K, seed=0, **options):
    from ctclip_mi355x.trainer import CTClipTrainer
    K.reset_ln_status()
    torch.manual_seed(0)
    return CTClipTrainer(build(cfg_small(), seed=seed, multi_positive=True, **options), lr=LR)


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


def _dropout_forward(model, text, hu, **kw):
    """A train-mode forward with BERT's hidden dropout at 0.1, from dropout call state 0, the codebook EMA
    withheld, no graph: two such calls see the same dropout masks."""
    tt = model.text_transformer
    model.train()
    old_p, tt.config.hidden_dropout_prob = tt.config.hidden_dropout_prob, 0.1
    old = model.set_ema_mode('skip')
    try:
        tt.set_dropout_state(0)
        with torch.no_grad():
            return model(text, hu, **kw)
    finally:
        model.set_ema_mode(old)
        tt.config.hidden_dropout_prob = old_p


def test_two_identical_reports_are_positives_of_each_other(K):
    """Fails without the feature (the keyword is swallowed, plain InfoNCE is trained and
    ``last_positive_count`` does not exist).  A batch of 4 whose reports 1 and 3 are the same kept tokens
    (their pad content differs).

    Training mode, BERT's dropout on (each copy of the report gets its own masks, so the two text latents
    differ -- the case the option is for): ``forward(return_loss=True)`` is the restatement (float64) on the
    latents ``return_latents`` gives under the same masks with ids (a, b, c, b); it differs from the plain
    model's loss on the same masks by more than the bound; ``last_positive_count`` is 2.

    Eval mode: the same against the restatement, and explicit ``pair_ids`` with the same groups give the same
    bits.  There the two text latents are the same bits, and then the multi-positive loss EQUALS InfoNCE as a
    function: with t_1 = t_3, x_1j = x_3j for every j, so the group means (x_11 + x_13) / 2 + (x_31 + x_33) / 2
    sum to x_11 + x_33 in both directions -- asserted here as an identity within the loss
    bound; grouping two DIFFERENT reports through ``pair_ids`` moves the loss.  Scores, latents and encodings
    are the plain model's."""
    cfg = cfg_small()
    model = build(cfg, multi_positive=True)
    plain_model = build(cfg)
    with torch.no_grad():
        model.temperature.fill_(LT10)
        plain_model.temperature.fill_(LT10)
    hu, text = duplicate_batch(cfg, 4, dup=(1, 3))
    assert not torch.equal(text.input_ids[1], text.input_ids[3])        # behind the mask they differ
    ids = torch.tensor([0, 1, 2, 1])
    lt = model.temperature.detach()
    bound = lambda v: 1e-5 * max(1.0, abs(v))
    # ---- training mode, dropout on
    loss = _dropout_forward(model, text, hu, return_loss=True)
    npos = model.last_positive_count
    tn, inn, _ = _dropout_forward(model, text, hu, return_latents=True)
    plain = _dropout_forward(plain_model, text, hu, return_loss=True)
    ref = multipos_loss(tn.double().cpu(), inn.double().cpu(), ids, lt.double().cpu()).item()
    cos13 = (tn[1] * tn[3]).sum().item()
    print(f'train mode: loss {loss.item():.7f} restatement {ref:.7f} (plain model {plain.item():.7f}); '
          f'npos {npos.item()}; cosine of the two copies\' text latents {cos13:.6f}')
    assert not torch.equal(tn[1], tn[3])
    assert abs(loss.item() - ref) < bound(ref)
    assert abs(loss.item() - plain.item()) > bound(plain.item())
    assert npos.is_cuda and npos.dtype == torch.int32 and npos.item() == 2 and not npos.requires_grad
    # ---- eval mode
    model.eval()
    plain_model.eval()
    with torch.no_grad():
        loss = model(text, hu, return_loss=True)
        npos = model.last_positive_count
        tn, inn, tokens = model(text, hu, return_latents=True)
        scores = model(text, hu)
        enc = model(text, hu, return_encodings=True)
        plain = plain_model(text, hu, return_loss=True)
        assert torch.equal(scores, plain_model(text, hu))
        assert all(torch.equal(a, b) for a, b in zip(enc, plain_model(text, hu, return_encodings=True)))
        assert all(torch.equal(a, b) for a, b in zip((tn, inn), plain_model(text, hu, return_latents=True)[:2]))
        by_ids = model(text, hu, return_loss=True, pair_ids=torch.tensor([5, -9, 6, -9]))
        by_dev_ids = model(text, hu, return_loss=True, pair_ids=torch.tensor([1, 2, 3, 2], device=dev))
        other_pair = model(text, hu, return_loss=True, pair_ids=torch.tensor([3, 1, 3, 2]))
        all_distinct = model(text, hu, return_loss=True, pair_ids=torch.arange(4))
        npos_distinct = model.last_positive_count
    ref = multipos_loss(tn.double().cpu(), inn.double().cpu(), ids, lt.double().cpu()).item()
    ref_other = multipos_loss(tn.double().cpu(), inn.double().cpu(), torch.tensor([3, 1, 3, 2]), lt.double().cpu()).item()
    print(f'eval mode: loss {loss.item():.7f} restatement {ref:.7f} (plain model {plain.item():.7f}); npos '
          f'{npos.item()}; reports 0 and 2 grouped {other_pair.item():.7f} restatement {ref_other:.7f}')
    assert torch.equal(tn[1], tn[3])
    assert abs(loss.item() - ref) < bound(ref) and npos.item() == 2
    assert abs(loss.item() - plain.item()) < bound(plain.item())         # the identity for equal text latents
    assert torch.equal(by_ids, loss) and torch.equal(by_dev_ids, loss)
    assert abs(other_pair.item() - ref_other) < bound(ref_other)
    assert abs(other_pair.item() - plain.item()) > bound(plain.item())
    assert npos_distinct.item() == 0
    assert abs(all_distinct.item() - plain.item()) < bound(plain.item())
    with pytest.raises(ValueError, match='pair_ids'):
        model(text, hu, return_loss=True, pair_ids=torch.arange(4, dtype=torch.int32))
    with pytest.raises(ValueError, match='pair_ids'):
        model(text, hu, return_loss=True, pair_ids=torch.arange(3))
    with pytest.raises(ValueError, match='pair_ids without multi_positive'):
        plain_model(text, hu, return_loss=True, pair_ids=torch.arange(4))


@pytest.fixture(scope='module')
def steps(K, tmp_path_factory):
    """Two ``train_step``s of a multi-positive model on two batches with a duplicate report each (run A), and
    the same stopped after the first: saved, loaded into a stranger (other weights, another seed) and
    continued (run B)."""
    from test_gpu_checkpoint import snapshot
    cfg = cfg_small()
    data = [duplicate_batch(cfg, 2, seed=s) for s in range(2)]
    out = {}
    tr = _trainer(K)
    model = tr.model
    assert dict(model.named_parameters())['temperature'].requires_grad
    hu, text = data[0]
    out['latents'] = _raw_latents(model, text, hu)
    out['p0'] = model.temperature.detach().clone()
    out['hyper'] = (tr.lr, tr.betas, tr.eps)
    out['loss1'] = tr.train_step(text, hu).reshape(1).clone()
    out['npos1'] = model.last_positive_count.clone()
    tr.flush()
    torch.cuda.synchronize()
    out['p1'] = model.temperature.detach().clone()
    out['norm'] = tr.norm.clone()
    out['loss2'] = tr.train_step(data[1][1], data[1][0]).reshape(1).clone()
    out['A'] = snapshot(tr)
    del tr, model
    # run B
    path = str(tmp_path_factory.mktemp('ck') / 'multipos.pt')
    tr = _trainer(K)
    tr.train_step(data[0][1], data[0][0])
    tr.save(path)
    del tr
    from ctclip_mi355x.trainer import CTClipTrainer
    torch.manual_seed(77)
    tr = CTClipTrainer(build(cfg, seed=7, multi_positive=True), lr=LR)
    out['load'] = tr.load(path)
    out['loss2_resumed'] = tr.train_step(data[1][1], data[1][0]).reshape(1).clone()
    out['B'] = snapshot(tr)
    out['path'] = path
    del tr
    return out


def test_train_step_moves_temperature_by_the_predicted_adam_update(steps):
    """Step 1 of Adam moves a parameter by -lr g c / (|g c| + eps) (c the clip coefficient): with g the
    FLOAT64 gradient of the restatement on the step's own raw latents and ids (both reports one group),
    ``temperature`` lands there within 1e-5 lr plus one f32 ulp of the parameter (the allowance of
    test_gpu_chunked_step.py).  The loss of the step is the restatement's."""
    t_raw, i_raw = steps['latents']
    lt0 = steps['p0']
    rl, _, _, rdlt, _ = ref64(t_raw, i_raw, torch.tensor([4, 4]), lt0.reshape(1))
    loss = steps['loss1'].item()
    print(f'step loss {loss:.7f} restatement {rl.item():.7f}; f64 dlt {rdlt.item():.6e}; '
          f'grad norm {steps["norm"][0].item():.4e} clip {steps["norm"][1].item():.4e}')
    assert abs(loss - rl.item()) < 1e-5 * max(1.0, abs(rl.item()))
    assert steps['npos1'].item() == 2
    lr, _, eps = steps['hyper']
    gc = rdlt.item() * steps['norm'][1].double().item()
    want = lt0.double().item() - lr * gc / (abs(gc) + eps)
    p1 = steps['p1']
    err = abs(p1.double().item() - want)
    print(f'temperature: {lt0.item():.7f} -> {p1.item():.7f}, predicted {want:.7f}, |d| {err:.2e}')
    assert p1.item() != lt0.item() and abs(gc) > 1e3 * eps
    assert err <= 1e-5 * lr + abs(want) * 2.0 ** -23


def test_save_load_step_gives_the_bits_of_the_uninterrupted_run(steps):
    from test_gpu_checkpoint import assert_same
    res = steps['load']
    assert res['step'] == 1 and not res['missing_keys'] and not res['unexpected_keys'] and res['hyper_mismatch'] == {}
    ck = torch.load(steps['path'], map_location='cpu', weights_only=True)
    assert not any('positive' in k or 'multi' in k for k in ck['model'])        # checkpoints need nothing new
    assert torch.equal(steps['loss2_resumed'], steps['loss2'])
    assert_same(steps['A'], steps['B'])


def test_chunked_step_matches_train_step(K):
    """Bg = 4, reports 1 and 2 identical so the duplicate spans the two chunks: ``train_step_chunked(chunk=2)``
    against ``train_step`` from the same state -- the loss within 1e-5 max(1, |loss|) (the project's loss
    tolerance) -- and the same bits on repeat (loss, parameters, moments).  The temperature gets its gradient
    once; explicit ``pair_ids`` take the same path."""
    cfg = cfg_small()
    hu, text = duplicate_batch(cfg, 4, dup=(1, 2))
    runs = []
    for mode in ('chunked', 'chunked', 'ids', None):
        tr = _trainer(K)
        if mode == 'ids':
            loss = tr.train_step_chunked(text, hu, 2, pair_ids=torch.tensor([8, 3, 3, -1]))
        else:
            loss = tr.train_step_chunked(text, hu, 2) if mode else tr.train_step(text, hu)
        tr.flush()
        torch.cuda.synchronize()
        assert torch.isfinite(loss) and tr.steps == 1 and tr.model.last_positive_count.item() == 2
        runs.append((loss.reshape(1).clone(), tr.flat.data.clone(), tr.m.clone(), tr.v.clone(),
                     tr.model.temperature.detach().clone()))
        del tr
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)
    for a, b in zip(runs[0], runs[2]):
        assert torch.equal(a, b)
    chunked, one = runs[0][0].item(), runs[3][0].item()
    print(f'loss: chunked {chunked:.7f} one-shot {one:.7f} |d| {abs(chunked - one):.2e}; temperature '
          f'{runs[0][4].item():.7f} / {runs[3][4].item():.7f}')
    assert abs(chunked - one) < 1e-5 * max(1.0, abs(one))
    # step 1 of Adam moves a scalar by lr (its sign): added once, not once per chunk
    assert abs(runs[0][4].item() - runs[3][4].item()) <= 1e-5 * LR + abs(runs[3][4].item()) * 2.0 ** -23
    with pytest.raises(ValueError, match='pair_ids'):
        _trainer(K).train_step_chunked(text, hu, 2, pair_ids=torch.arange(3))
