"""The volume-augmentation kernel on the GPU (csrc/augment.hip ctclip_augment_volume):
exact cases against torch slicing / flip / rot90, drawn parameters against the float64 restatement
of tests/augment_common.py (pinned on the host by test_augment_cpu.py), the noise path against the
integer restatement of the hash, launch and chunk invariance, and the views through the trainer.

Shapes (B, D, H, W): (2, 5, 7, 19) odd extents, the voxel-by-voxel stores and unaligned rows;
(1, 4, 8, 8) every store a 16-byte vector; (2, 3, 9, 72) rows wider than 64 voxels, so a wave's
64 lanes wrap from one output row into the next.  Each for int16 and f32 with V = 2."""
import pytest
import torch

import augment_common as AC
from ctclip_mi355x.augment import AugmentParams, CTAugment, apply, augment_volume

pytestmark = pytest.mark.gpu
dev = 'cuda'
SHAPES = [(2, 5, 7, 19), (1, 4, 8, 8), (2, 3, 9, 72)]
DTYPES = [torch.int16, torch.float32]
FILLS = {torch.int16: -1000, torch.float32: -1.0}
WIDE = dict(rotate_deg=45.0, scale=(0.7, 1.4), gain=(0.9, 1.1), shift=0.05, noise_sigma=(0.05, 0.05))


def _wide(shape, seed=0):
    _, D, H, W = shape
    return CTAugment(seed=seed, translate=(D / 3, H / 3, W / 3), **WIDE)


@pytest.mark.parametrize('dtype', DTYPES, ids=['i16', 'f32'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_exact_cases(shape, dtype):
    B, D, H, W = shape
    x = AC.make_volume(B, D, H, W, dtype)
    xd = x.to(dev)
    # view 0 the identity, view 1 a flip along w
    p = AugmentParams.identity(2, B)
    p.matrix[1, :, 2, 2] = -1.0
    out = apply(xd, p)
    assert out.shape == (2, B, 1, D, H, W) and out.dtype == dtype and out.is_contiguous()
    assert torch.equal(out[0].cpu(), x) and torch.equal(out[1].cpu(), torch.flip(x, dims=(-1,)))
    # integer translations, one per view; the last pair shifts the whole volume out
    for ta, tb in [((1, -2, 3), (0, 0, -(W - 1))), ((-(D - 1), H - 1, 0), (0, 1, 0)), ((0, 0, W), (-D, 0, 0))]:
        p = AugmentParams.identity(2, B)
        p.matrix[0, :, :, 3] = torch.tensor(ta, dtype=torch.float64)
        p.matrix[1, :, :, 3] = torch.tensor(tb, dtype=torch.float64)
        out = apply(xd, p).cpu()
        assert torch.equal(out[0], AC.shifted(x, ta, FILLS[dtype])), ta
        assert torch.equal(out[1], AC.shifted(x, tb, FILLS[dtype])), tb
    assert (out == FILLS[dtype]).all()
    if H == W:
        p = AC.set_matrix(AugmentParams.identity(2, B), AC.QUARTER_TURN_HW)
        out = apply(xd, p).cpu()
        assert torch.equal(out[0], torch.rot90(x, 1, dims=(-2, -1))) and torch.equal(out[1], out[0])


@pytest.mark.parametrize('dtype', DTYPES, ids=['i16', 'f32'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_drawn_parameters_match_restatement(shape, dtype):
    """Every range widened (45 degrees, scale 0.7-1.4, translations of a third of each extent, sigma
    0.05).  Equality is expected; the allowance is test_preprocess.py's for the resample kernel: at
    most 1e-4 of the voxels may differ, each by at most 1 f32 ulp / 1 HU."""
    B, D, H, W = shape
    x = AC.make_volume(B, D, H, W, dtype, seed=1)
    p = _wide(shape, seed=5).draw(step=3, B=B, n_views=2)
    got = apply(x.to(dev), p).cpu()
    ref = AC.restate(x, p)
    n, worst = AC.compare(got, ref)
    inside = (ref != FILLS[dtype]).float().mean().item()
    print(f'{shape} {dtype}: {n} of {ref.numel()} voxels differ (worst {worst}); {inside:.2f} not fill')
    assert inside > 0.3                      # the views are not mostly padding
    assert n <= 1e-4 * ref.numel() and worst <= 1


@pytest.mark.parametrize('dtype', DTYPES, ids=['i16', 'f32'])
def test_noise_path_against_integer_hash(dtype):
    """Identity geometry, sigma > 0: y = x + sigma * n with n from the plain-Python-int hash."""
    B, D, H, W = 2, 5, 7, 19
    x = AC.make_volume(B, D, H, W, dtype, seed=2)
    p = AugmentParams.identity(2, B)
    p.sigma[:] = torch.tensor([[0.05, 0.3], [1e-3, 0.05]], dtype=torch.float64)
    p.seed[:] = torch.tensor([[1, -1], [0x7fffffffffffffff, -0x8000000000000000]])
    got = apply(x.to(dev), p).cpu()
    xn = x.double() / 1000.0 if dtype == torch.int16 else x.double()
    for v in range(2):
        for b in range(B):
            n = torch.tensor([AC.noise_int(int(p.seed[v, b]), i) for i in range(D * H * W)], dtype=torch.float64)
            y = (xn[b].reshape(-1) * 1.0 + 0.0 + float(p.sigma[v, b]) * n).clamp(-1.0, 1.0)
            want = torch.round(1000.0 * y).to(torch.int16) if dtype == torch.int16 else y.float()
            assert torch.equal(got[v, b].reshape(-1), want), (v, b)
    assert not torch.equal(got[0, 0], got[1, 0])


@pytest.mark.parametrize('dtype', DTYPES, ids=['i16', 'f32'])
def test_launch_and_chunk_invariance(dtype):
    """Two calls with the same parameters are bit-equal, and the output of sample b does not change
    when the batch is split into two calls (each with its own slice of the records)."""
    shape = (3, 3, 9, 72)
    B, D, H, W = shape
    xd = AC.make_volume(B, D, H, W, dtype, seed=3).to(dev)
    aug = _wide(shape, seed=9)
    whole = apply(xd, aug.draw(step=1, B=B, n_views=2))
    assert torch.equal(whole, apply(xd, aug.draw(step=1, B=B, n_views=2)))
    first = apply(xd[:1], aug.draw(step=1, B=1, n_views=2))
    rest = apply(xd[1:], aug.draw(step=1, B=2, n_views=2, sample_offset=1))
    assert torch.equal(whole, torch.cat([first, rest], dim=1))
    views = aug.views(xd, step=1, n_views=2)
    assert len(views) == 2 and all(v.shape == xd.shape and v.is_contiguous() for v in views)
    assert torch.equal(torch.stack(views), whole)


def test_refusals_and_op():
    from ctclip_mi355x._lib import AugmentArgs, KernelError, call, ptr
    import ctypes
    x = AC.make_volume(2, 3, 4, 8, torch.float32).to(dev)
    rec = AugmentParams.identity(2, 2).pack().to(dev)
    out = torch.ops.ctclip.augment_volume(x, rec)
    assert torch.equal(out, torch.stack([x, x]))
    for bad in (x[:, :, :, :, ::2], x[:, 0], x.expand(2, 2, 3, 4, 8), x.double()):
        with pytest.raises(ValueError, match='augment:'):
            augment_volume(bad, rec)
    with pytest.raises(ValueError, match='augment: records'):
        augment_volume(x, rec[:, :1].contiguous())
    a = AugmentArgs()
    a.src, a.dtype, a.recs = ptr(x), 0, ptr(rec)
    a.B, a.D, a.H, a.W, a.V = 2, 3, 4, 8, 0
    with pytest.raises(KernelError, match='1003'):                    # CT_ESHAPE: V < 1
        call('ctclip_augment_volume', ctypes.byref(a), ptr(out), None)
    a.V, a.B = 2, 40000
    with pytest.raises(KernelError, match='1003'):                    # V * B > 65535
        call('ctclip_augment_volume', ctypes.byref(a), ptr(out), None)
    a.B, a.recs = 2, None
    with pytest.raises(KernelError, match='1001'):                    # CT_EINVAL: null records
        call('ctclip_augment_volume', ctypes.byref(a), ptr(out), None)


# ------------------------------------------------------------------------------ trainer
def test_train_step_augmented():
    """One train_step_augmented with n_views = 1: a finite loss that differs from the plain step's,
    bit-equal between two identically seeded runs and to train_step(aug_image=augment.views(...))."""
    from ctclip_mi355x.trainer import CTClipTrainer
    from test_gpu_loss_options import cfg_small, build, _batch
    cfg = cfg_small(layers=1)
    hu, _, _, _, text = _batch(cfg)
    hu = hu.to(dev)
    aug = CTAugment(seed=4, translate=(2, 8, 8))

    def run(step):
        torch.manual_seed(0)
        model = build(cfg)
        tr = CTClipTrainer(model, lr=1e-4)
        loss = step(tr)
        tr.flush()
        torch.cuda.synchronize()
        return loss.detach().clone(), tr.flat.data.clone()

    plain = run(lambda tr: tr.train_step(text, hu))
    a = run(lambda tr: tr.train_step_augmented(text, hu, aug, n_views=1))
    b = run(lambda tr: tr.train_step_augmented(text, hu, aug, n_views=1))
    c = run(lambda tr: tr.train_step(text, hu, aug_image=aug.views(hu, step=tr.steps, n_views=1, sample_offset=0)))
    print(f'plain loss {plain[0].item():.6f}, augmented {a[0].item():.6f}')
    assert torch.isfinite(a[0]).all() and not torch.equal(a[0], plain[0])
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1])
