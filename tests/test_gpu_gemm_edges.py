"""Every GEMM epilogue of both MFMA families at ragged edges: operands are views into NaN-padded
buffers, outputs views into sentinel-filled ones (tests/gemm_edge_common.py), and every output element is held
to a float64 reference within a derived per-element bound, for every launch variant of the 8-phase kernel
(tests/test_gpu_gemm_tiles.py _variants) and every operand layout of the 128-tile kernel.  Each case prints
max(err / bound) per output."""
import pytest
import torch

import gemm_edge_common as G
from test_gpu_gemm_tiles import _PLAN_CASES, _variants

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def K():
    from ctclip_mi355x import kernels
    return kernels


# ---------------------------------------------------------------- 8-phase family (gemm.hip routes_to_256)
# ragged N per kind: 9 tiles + 8 columns where the epilogue takes N % 8, + 64 for act 2 / 3 / 5, + 32 for act 4
def _n_ragged(kind):
    return 2368 if kind in G.KINDS_NEED_N64 else 2336 if kind.startswith('geglu_bwd') else 2312


_EXTRA = [(True, True, k) for k in ('rows', 'res', 'bf16', 'geglu', 'argmax', 'l2n', 'acc', 'res_shadow', 'gelu',
                                    'geglu_bwd_h16')] + [(True, False, 'acc'), (False, True, 'res_shadow')]
_KC_KINDS = sorted({k for a, b, k in _PLAN_CASES + _EXTRA if a and b})
# every (layout, kind) at ragged M x ragged N x K = 192 (the ring wraps; slabs: K = 1024, split 2); the
# K-contiguous layout also at the 160-row tail with one K-step, and at the aligned control N = 2560
CASES_256 = ([(ak, bk, kind, 3848, _n_ragged(kind), 1024 if kind == 'slabs' else 192) for ak, bk, kind in _PLAN_CASES + _EXTRA]
             + [(True, True, kind, 4000, _n_ragged(kind), 1024 if kind == 'slabs' else 64) for kind in _KC_KINDS]
             + [(True, True, kind, 4000, 2560, 1024 if kind == 'slabs' else 192) for kind in _KC_KINDS])


def _check_l2n_bits(K, c, outs):
    """qn is the stand-alone l2norm kernel's output on the stored q, bit for bit (tests/test_gpu_gemm_tiles.py)"""
    want = K.l2norm_scale_fwd(outs['C'].view[:, :c.n2], c.n2 // 32, 32, c.scale)
    assert torch.equal(outs['C2'].view, want), 'qn differs from l2norm_scale_fwd(q)'


@pytest.mark.parametrize('ak,bk,kind,M,N,Kd', CASES_256)
def test_8phase_edges(K, ak, bk, kind, M, N, Kd):
    dev = torch.device('cuda')
    c = G.make_case(kind, M, N, Kd, ak, bk, dev, family=256)
    spec = G.new_outs(c)
    before = {k: o.buf.clone() for k, o in spec.items()}

    def run():
        outs = G.new_outs(c)
        G.launch(K, c, outs)
        return G.pack(outs)
    res = _variants(K, run)
    checked = []
    for name, packed in res.items():
        if any(torch.equal(packed, p) for p in checked):     # the same bytes, margins included: the same verdict
            continue
        outs = G.unpack(packed, spec)
        rep = G.verify(c, outs, before, label=f'8-phase {kind} ak={int(ak)} bk={int(bk)} {M}x{N}x{Kd} variant {name}')
        assert rep.ok(), (name, rep.failed)
        if kind == 'l2n':
            _check_l2n_bits(K, c, outs)
        checked.append(packed)


def test_8phase_batched_argmax(K):
    """batch = 2 through sA / sC / sC2: PAD_R sentinel rows lie between the two batches' outputs"""
    dev = torch.device('cuda')
    nb, M, N, Kd = 2, 1800, 2368, 192          # 8 x 10 tiles x 2 batches = 160
    cs = [G.make_case('argmax', M + 8 * b, N, Kd, True, True, dev, family=256) for b in range(nb)]
    lda, ng = Kd + G.PAD_C, N // 64
    A = torch.full((nb, M + G.PAD_R, lda), float('nan'), device=dev, dtype=G.BF16)
    for b in range(nb):
        A[b, :M, :Kd] = cs[b].op.A[:M]
    Bm = cs[0].Bm
    ldc, ldc2 = ng + G.PAD_C, ng + G.PAD_C

    def run():
        C = torch.full((nb, M + G.PAD_R, 2 * ldc), G.SENT32, device=dev, dtype=torch.int32).view(G.F32)
        C2 = torch.full((nb, M + G.PAD_R, ldc2), G.SENT32, device=dev, dtype=torch.int32).view(G.F32)
        K._gemm_raw(M, N, Kd, A, lda, True, Bm, Bm.stride(0), True, C, ldc, act=K.ACT_ARGMAX, batch=nb,
                    sA=(M + G.PAD_R) * lda, sB=0, sC=(M + G.PAD_R) * ldc, C2=C2, ldc2=ldc2, sC2=(M + G.PAD_R) * ldc2)
        return torch.cat([C.reshape(-1), C2.reshape(-1)]).view(torch.int32)     # integers: NaN sentinels compare equal
    res = _variants(K, run)
    for name, flat in res.items():
        C = flat[:nb * (M + G.PAD_R) * 2 * ldc].view(G.F32).view(nb, M + G.PAD_R, 2 * ldc)
        C2 = flat[nb * (M + G.PAD_R) * 2 * ldc:].view(G.F32).view(nb, M + G.PAD_R, ldc2)
        for T, live in ((C, 2 * ng), (C2, ng)):
            m = T.view(torch.int32).clone()
            m[:, :M, :live] = G.SENT32
            assert (m == G.SENT32).all(), f'variant {name}: a store outside the live outputs'
        for b in range(nb):
            cb = G.types.SimpleNamespace(M=M, N=N)
            P = A[b, :M, :Kd].double() @ cs[0].op.B.double().t()
            E = Kd * G.U23 * (A[b, :M, :Kd].double().abs() @ cs[0].op.B.double().abs().t())
            ratios, bad = G.check_argmax(cb, C[b, :M, :2 * ng], C2[b, :M, :ng], P=P, E=E)
            print(f'8-phase batched argmax variant {name} batch {b}: ' + ', '.join(f'{k} {r:.3f}' for k, r in ratios.items()))
            assert not bad and all(r <= 1.0 for r in ratios.values()), (name, b, ratios, bad)


# ---------------------------------------------------------------- 128-tile family (gemm.hip)
KINDS_128 = ['res', 'bf16', 'gelu', 'geglu', 'l2n', 'gelu_bwd', 'hilo', 'split3', 'argmax', 'geglu_bwd', 'rows', 'acc',
             'res_shadow', 'slabs']
SHAPES_128 = [(136, 72, 200), (300, 136, 200), (8, 512, 1024)]


def _n_128(kind, N):
    if kind in ('geglu', 'l2n'):
        return (N + 63) // 64 * 64
    return (N + 31) // 32 * 32 if kind.startswith('geglu_bwd') else N     # (the argmax keeps its ragged last group)


@pytest.mark.parametrize('M,N,Kd', SHAPES_128)
@pytest.mark.parametrize('kind', KINDS_128)
def test_128tile_edges(K, kind, M, N, Kd):
    """every operand layout the entry point offers (an M-contiguous A needs M % 8 == 0, so M = 300 runs
    with K-contiguous A only); M = 8, K = 1024 also takes the wrapper's automatic split-K where it has one"""
    dev = torch.device('cuda')
    N = _n_128(kind, N)
    for ak in ((True, False) if M % 8 == 0 else (True,)):
        for bk in (True, False):
            c = G.make_case(kind, M, N, Kd, ak, bk, dev, family=128)
            outs = G.new_outs(c)
            before = {k: o.buf.clone() for k, o in outs.items()}
            c.extra_adds = K._auto_split(M, N, Kd, c.kw.get('act', 0), c.kw.get('split_k', 1), 1,
                                         c.kw.get('accumulate', False), outs['C'].view) - 1
            G.launch(K, c, outs)
            torch.cuda.synchronize()
            rep = G.verify(c, outs, before, label=f'128-tile {kind} ak={int(ak)} bk={int(bk)} {M}x{N}x{Kd}')
            assert rep.ok(), rep.failed
            if kind == 'l2n':
                _check_l2n_bits(K, c, outs)


def test_routes():
    """the shapes above reach the family they are meant for: gemm.hip routes_to_256 restated (K % 64 == 0,
    M, N >= 256, at least 160 tiles of 256 x 256, slabs of at least 512)"""
    def to256(M, N, Kd, split=1, batch=1):
        tiles = -(-M // 256) * -(-N // 256) * split * batch
        return Kd % 64 == 0 and M >= 256 and N >= 256 and tiles >= 160 and (split == 1 or Kd // split >= 512)
    for ak, bk, kind, M, N, Kd in CASES_256:
        assert to256(M, N, Kd, 2 if kind == 'slabs' else 1), (kind, M, N, Kd)
    assert to256(1800, 2368, 192, batch=2)
    for M, N, Kd in SHAPES_128:
        assert not to256(M, N, Kd) and not to256(M, N, Kd, 3)
