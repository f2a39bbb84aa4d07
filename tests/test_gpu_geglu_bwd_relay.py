"""The GEGLU-backward GEMM's row-contiguous epilogue (gemm256.hip, epilogue_geglu_bwd_rows: h loads
and dh stores relayed through a wave-private LDS strip) at the smallest shapes that reach every guard:
M ragged against the 16-row block and the 256-row tile, G = one wave's 64 columns / ragged against
the 256-column tile / ragged on the second column tile, one and eight K-steps, both forms of h."""
import pytest
import torch

pytestmark = pytest.mark.gpu
F16, BF16 = torch.float16, torch.bfloat16
SENT = 7.0
CASES = [(M, G, D, hdt) for M in (16, 272) for G in (64, 192, 320) for D in (64, 512) for hdt in (F16, BF16)]

# cases at which the lane-per-row epilogue (the parent of the relay) differs from the unfused composition
NOT_EXACT = {(272, 64, 512, F16), (272, 192, 512, F16), (272, 192, 512, BF16), (272, 320, 512, F16),
             (272, 320, 512, BF16)}


@pytest.fixture(scope='module')
def K():
    from ctclip_mi355x import kernels
    return kernels


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def make_inputs(M, G, D, hdt):
    """dy, w2p, h (a view into a NaN-padded buffer: a read past column 2G shows in dh)"""
    g_ = torch.Generator(device='cuda').manual_seed(1000 * M + 10 * G + D + (hdt == F16))
    hbuf = torch.full((M, 2 * G + 64), float('nan'), device='cuda', dtype=hdt)
    h = hbuf[:, :2 * G]
    h.copy_(torch.randn(M, 2 * G, device='cuda', generator=g_).to(hdt))
    dy = (torch.randn(M, D, device='cuda', generator=g_) * 0.1).bfloat16()
    w2p = (torch.randn(D, G, device='cuda', generator=g_) * 0.05).bfloat16()
    return dy, w2p, h


def run_fused(K, dy, w2p, h):
    """(dh, whole sentinel-filled buffer): 16 spare rows below and 64 spare columns right of dh"""
    M, G = dy.shape[0], w2p.shape[1]
    dbuf = torch.full((M + 16, 2 * G + 64), SENT, device='cuda', dtype=BF16)
    dh = dbuf[:M, :2 * G]
    K.matmul_nn_geglu_bwd(dy, w2p, h, out=dh)
    torch.cuda.synchronize()
    return dh, dbuf


def reference64(dy, w2p, h):
    """float64 from the same inputs; dg rounded to bf16 as the kernel documents, then float64 products"""
    M, G = dy.shape[0], w2p.shape[1]
    d = (dy.double() @ w2p.double()).float().bfloat16().double().view(M, G // 32, 32)
    hv = h.double().view(M, G // 32, 2, 32)
    xg, gt = hv[:, :, 0], hv[:, :, 1]
    if h.dtype == F16:     # derivative form [gelu(gate) | x gelu'(gate)]
        ref = torch.stack([d * xg, d * gt], 2)
    else:                  # pre-activation [x | gate]
        cdf = 0.5 * (1 + torch.erf(gt / 2 ** 0.5))
        pdf = torch.exp(-0.5 * gt * gt) / (2 * torch.pi) ** 0.5
        ref = torch.stack([d * gt * cdf, d * xg * (cdf + gt * pdf)], 2)
    return ref.reshape(M, 2 * G)


def unfused(K, dy, w2p, h):
    """The composition the fused kernel replaces: dg = dy @ w2p stored as bf16, then the GEGLU backward
    (the stand-alone kernel for the bf16 form; two f32 products rounded to bf16 for the fp16 form)."""
    M, G = dy.shape[0], w2p.shape[1]
    dg = K.matmul_nn(dy, w2p)
    if h.dtype == BF16:
        return K.geglu_bwd(dg, h.contiguous())
    hv = h.float().view(M, G // 32, 2, 32)
    d = dg.float().view(M, G // 32, 1, 32)
    return (d * hv).bfloat16().reshape(M, 2 * G)


@pytest.mark.parametrize('M,G,D,hdt', CASES)
def test_geglu_bwd_rows(K, M, G, D, hdt):
    """Against float64 at the tolerance test_geglu_bwd_epilogue_bounds uses for this kernel (relative
    Frobenius error < 1e-2); rows >= M and columns >= 2G of the over-allocated output untouched.
    The relay moves bytes only, so dh was checked bit-identical to the lane-per-row epilogue's at
    every case here (and at M = 4,100, G = 1,408); where that epilogue equals the unfused composition
    (everywhere but NOT_EXACT, where the small-shape matmul_nn sums K = 512 in another order and a few
    dg land on the other side of a bf16 rounding), so must this one."""
    dy, w2p, h = make_inputs(M, G, D, hdt)
    dh, dbuf = run_fused(K, dy, w2p, h)
    assert (dbuf[:, 2 * G:] == SENT).all() and (dbuf[M:] == SENT).all()
    assert torch.isfinite(dh.float()).all()
    err = _rel(dh, reference64(dy, w2p, h))
    print(f'M {M} G {G} D {D} {hdt}: rel err vs float64 {err:.3e}')
    assert err < 1e-2
    if (M, G, D, hdt) not in NOT_EXACT:
        assert torch.equal(dh, unfused(K, dy, w2p, h))
