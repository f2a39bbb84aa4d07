"""Host-side checks of the volume augmentation (ctclip_mi355x/augment.py): the float64
restatement of the kernel (tests/augment_common.py) against torch slicing / flip / rot90, which pins
the restatement itself, and the parameter draw: deterministic, a function of (seed, step, global
sample index, view), inside its configured ranges, and a unit-variance noise variate."""
import math

import numpy as np
import pytest
import torch

import augment_common as AC
from ctclip_mi355x.augment import AugmentParams, CTAugment, apply, mix64

DTYPES = [torch.int16, torch.float32]
FILLS = {torch.int16: -1000, torch.float32: -1.0}


# ------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('dtype', DTYPES)
def test_restatement_identity_flip_shift(dtype):
    x = AC.make_volume(2, 5, 7, 19, dtype)
    ident = AugmentParams.identity(2, 2)
    assert torch.equal(AC.restate(x, ident), torch.stack([x, x]))
    flip = AC.set_matrix(AugmentParams.identity(1, 2), AC.FLIP_W)
    assert torch.equal(AC.restate(x, flip)[0], torch.flip(x, dims=(-1,)))
    for t in [(1, -2, 3), (0, 0, -18), (-4, 6, 0), (0, 0, 19), (5, 0, 0)]:     # the last two: all fill
        p = AC.set_matrix(AugmentParams.identity(1, 2), t=[float(k) for k in t])
        assert torch.equal(AC.restate(x, p)[0], AC.shifted(x, t, FILLS[dtype])), t
    assert (AC.shifted(x, (0, 0, 19), FILLS[dtype]) == FILLS[dtype]).all()


@pytest.mark.parametrize('dtype', DTYPES)
def test_restatement_quarter_turn(dtype):
    x = AC.make_volume(1, 4, 8, 8, dtype)
    p = AC.set_matrix(AugmentParams.identity(1, 1), AC.QUARTER_TURN_HW)
    assert torch.equal(AC.restate(x, p)[0], torch.rot90(x, 1, dims=(-2, -1)))


def test_restatement_noise_and_hash():
    """The vectorised uint64 hash equals the plain-int one (and the module's), and sigma > 0 with
    identity geometry adds exactly sigma * n."""
    seed = 0x123456789abcdef0fedcba
    field = AC.noise_field(seed, 300)
    assert [AC.noise_int(seed, i) for i in range(300)] == field.tolist()
    assert AC.mix64(seed & AC.M64, 77) == mix64(seed & AC.M64, 77)
    x = AC.make_volume(1, 3, 4, 5, torch.float32)
    p = AugmentParams.identity(1, 1)
    p.sigma[:] = 0.05
    p.seed[:] = -12345
    want = np.clip(x.numpy().astype(np.float64).ravel() + 0.05 * AC.noise_field(-12345, 60), -1, 1).astype(np.float32)
    assert np.array_equal(AC.restate(x, p).numpy().ravel(), want)


# ------------------------------------------------------------------------------ the draw
def _eq(a, b):
    return all(torch.equal(getattr(a, n), getattr(b, n)) for n in ('matrix', 'gain', 'shift', 'sigma', 'seed'))


def test_draw_is_a_function_of_seed_step_sample_view():
    aug = CTAugment(seed=3)
    a = aug.draw(step=5, B=4, n_views=2)
    assert a.matrix.shape == (2, 4, 3, 4) and a.matrix.dtype == torch.float64
    assert a.gain.shape == a.shift.shape == a.sigma.shape == a.seed.shape == (2, 4) and a.seed.dtype == torch.int64
    assert _eq(a, CTAugment(seed=3).draw(step=5, B=4, n_views=2))
    torch.manual_seed(99)
    np.random.seed(99)                       # no global generator state enters
    assert _eq(a, aug.draw(step=5, B=4, n_views=2))
    assert not _eq(a, aug.draw(step=6, B=4, n_views=2))
    assert not _eq(a, CTAugment(seed=4).draw(step=5, B=4, n_views=2))
    assert not _eq(a, aug.draw(step=5, B=4, n_views=2, sample_offset=4))
    assert not torch.equal(a.matrix[0], a.matrix[1]) and not torch.equal(a.seed[0], a.seed[1])    # views
    assert len(set(a.seed.flatten().tolist())) == 8 and len(set(a.gain.flatten().tolist())) == 8


def test_draw_is_invariant_to_chunking():
    aug = CTAugment(seed=1)
    whole = aug.draw(step=2, B=6, n_views=2, sample_offset=12)
    parts = [aug.draw(step=2, B=n, n_views=2, sample_offset=12 + o) for o, n in ((0, 2), (2, 1), (3, 3))]
    for name in ('matrix', 'gain', 'shift', 'sigma', 'seed'):
        assert torch.equal(getattr(whole, name), torch.cat([getattr(p, name) for p in parts], dim=1)), name
    assert torch.equal(whole.matrix[1, 3], aug.draw(step=2, B=1, n_views=2, sample_offset=15).matrix[1, 0])


def test_drawn_parameters_stay_inside_their_ranges():
    """10,000 records (100 steps x 50 samples x 2 views).  From M = S^-1 R(th)^T: the d scale is
    1 / M[0, 0], the in-plane scale 1 / |row h|, the angle atan2(M[1, 2], M[1, 1]).  The tolerances
    only absorb the float64 rounding of that inversion."""
    aug = CTAugment(seed=7)
    recs = [aug.draw(step=s, B=50, n_views=2) for s in range(100)]
    m = torch.cat([r.matrix.reshape(-1, 3, 4) for r in recs])
    cat = lambda n: torch.cat([getattr(r, n).reshape(-1) for r in recs])
    gain, shift, sigma = cat('gain'), cat('shift'), cat('sigma')
    assert m.shape[0] == 10000 and bool(torch.isfinite(m).all())
    e = 1e-12
    s_d = 1.0 / m[:, 0, 0]
    s_hw = 1.0 / torch.sqrt(m[:, 1, 1] ** 2 + m[:, 1, 2] ** 2)
    ang = torch.rad2deg(torch.atan2(m[:, 1, 2], m[:, 1, 1]))
    for v, lo, hi in ((s_d, 0.9, 1.1), (s_hw, 0.9, 1.1), (ang, -10.0, 10.0), (m[:, 0, 3], -8, 8), (m[:, 1, 3], -24, 24),
                      (m[:, 2, 3], -24, 24)):
        assert lo - e <= v.min().item() and v.max().item() <= hi + e
        assert v.max().item() - v.min().item() > 0.9 * (hi - lo)           # and the range is used
    assert (m[:, 0, 1:3] == 0).all() and (m[:, 1:, 0] == 0).all()              # rotation about d only
    assert 0.9 <= gain.min().item() and gain.max().item() <= 1.1
    assert -0.05 <= shift.min().item() and shift.max().item() <= 0.05
    assert 0.0 <= sigma.min().item() and sigma.max().item() <= 0.02
    det = torch.linalg.det(m[:, :, :3])
    assert bool(torch.isfinite(det).all()) and det.min().item() > 0            # flip_w = 0: no reflection
    # flip_w = 1 reflects every record, 0.5 about half of them
    assert (torch.linalg.det(CTAugment(flip_w=1.0).draw(0, 64).matrix[0, :, :, :3]) < 0).all()
    half = (torch.linalg.det(CTAugment(flip_w=0.5).draw(0, 1000).matrix[0, :, :, :3]) < 0).float().mean().item()
    assert 0.4 < half < 0.6


def test_noise_variate_has_zero_mean_and_unit_variance():
    """10,000 variates of one seed: the mean within 3 standard errors of 0 (se = 1 / sqrt N) and the
    variance within 3 of 1 (se = sqrt((kurtosis - 1) / N), Irwin-Hall(4): kurtosis 3 - 1.2 / 4 = 2.7)."""
    n = AC.noise_field(mix64(11, 0), 10000)
    N = n.size
    assert abs(n.mean()) < 3.0 / math.sqrt(N)
    assert abs(n.var() - 1.0) < 3.0 * math.sqrt(1.7 / N)
    assert n.min() >= -2 * 65535 / AC.NOISE_DIV and n.max() <= 2 * 65535 / AC.NOISE_DIV
    assert AC.NOISE_DIV == math.sqrt(4 * (65536 ** 2 - 1) / 12)


# ------------------------------------------------------------------------------ refusals
def test_host_tensor_is_refused():
    x = AC.make_volume(1, 2, 3, 4, torch.int16)
    with pytest.raises(ValueError, match='augment: the volume must be a device tensor'):
        apply(x, AugmentParams.identity(1, 1))
    with pytest.raises(ValueError, match='augment: the volume must be a device tensor'):
        CTAugment().views(x, step=0)


def test_non_finite_parameters_are_refused():
    for name in ('matrix', 'gain', 'shift', 'sigma'):
        p = AugmentParams.identity(1, 2)
        getattr(p, name).view(-1)[1] = float('nan')
        with pytest.raises(ValueError, match=f'non-finite {name}'):
            p.pack()
    p = AugmentParams.identity(2, 3)
    p.seed[1, 2] = -2
    rec = p.pack()
    assert rec.shape == (2, 3, 16) and rec.view(torch.int64)[1, 2, 15].item() == -2
    assert rec[0, 0, :12].tolist() == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0] and rec[0, 0, 12:15].tolist() == [1, 0, 0]


def test_use_visual_ssl_still_raises():
    from ctclip_mi355x.ct_clip import CTCLIP
    with pytest.raises(Exception):
        CTCLIP(use_visual_ssl=True)
