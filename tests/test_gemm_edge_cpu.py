"""Checks the checks of tests/gemm_edge_common.py without a GPU: an f32 restatement of the GEMM with
each epilogue stays inside every per-element bound and leaves every guard band intact, and each of seven seeded
edge faults breaks a bound or a guard -- while the older tests' whole-matrix norm, printed next to it, lets
several of them through."""
import pytest
import torch

import gemm_edge_common as G

CPU = torch.device('cpu')
KINDS = ['rows', 'res', 'res_shadow', 'acc', 'slabs', 'bf16', 'gelu', 'geglu', 'argmax', 'argmax_f16', 'l2n',
         'geglu_bwd', 'geglu_bwd_h16', 'gelu_bwd', 'hilo', 'split3']
# the GPU file's shape classes scaled down: a row tail shorter than a 16-row block / a longer one, N ragged by
# 8 / by 64 / aligned, K of one step / ragged against the 64-deep step
SHAPES = [(72, 72, 200), (136, 128, 64)]


def _n_for(kind, N):
    if kind in G.KINDS_NEED_N64:
        return (N + 63) // 64 * 64
    if kind.startswith('geglu_bwd'):
        return (N + 31) // 32 * 32
    return N


def _run(c, **kw):
    outs = G.new_outs(c)
    before = {k: o.buf.clone() for k, o in outs.items()}
    G.restate(c, outs, **kw)
    return outs, before


@pytest.mark.parametrize('M,N,K', SHAPES)
@pytest.mark.parametrize('kind', KINDS)
def test_clean_restatement_holds(kind, M, N, K):
    for ak, bk in ((True, True), (False, False)):
        c = G.make_case(kind, M, _n_for(kind, N), K, ak, bk, CPU, family=128)
        outs, before = _run(c)
        rep = G.verify(c, outs, before, label=f'{kind} {M}x{c.N}x{K}')
        assert rep.ok(), rep.failed


def test_padded_views():
    """operands and outputs really are views with the margins the design states"""
    c = G.make_case('res_shadow', 72, 72, 200, True, False, CPU, family=128)
    assert c.Am.stride(0) == 200 + G.PAD_C and c.Bm.shape == (200, 72) and c.Bm.stride(0) == 72 + G.PAD_C
    assert torch.isnan(c.Am.as_strided((72 + G.PAD_R, 200 + G.PAD_C), (200 + G.PAD_C, 1))[72:]).all()
    assert torch.isnan(c.bias.as_strided((72 + G.PAD_C,), (1,))[72:]).all()
    outs = G.new_outs(c)
    assert outs['C'].buf.shape == (72 + G.PAD_R, 72 + G.PAD_C) and outs['C2'].view.stride(0) == 72 + G.PAD_C
    s = G.new_outs(G.make_case('slabs', 72, 72, 200, True, True, CPU, family=128))['C']
    assert s.buf.shape == (3, 72, 72 + G.PAD_C) and s.view.shape == (2, 72, 72)
    packed = G.pack(outs)
    back = G.unpack(packed, outs)
    assert all(torch.equal(G._ints(back[k].buf), G._ints(outs[k].buf)) for k in outs)


def test_slab_ranges():
    assert G.slab_ranges(1024, 2, 64, 256) == [(0, 512), (512, 1024)]
    assert G.slab_ranges(200, 3, 64, 128) == [(0, 128), (128, 200), (200, 200)]     # the third slab is empty
    assert G.slab_ranges(1024, 3, 64, 128) == [(0, 384), (384, 768), (768, 1024)]


def test_gelu_allowance():
    """the GELU allowance's provenance: the measurement recomputed, the recorded constants cover it tightly"""
    g, dg = G.measure_gelu_error()
    print(f'gelu_dev_f32 vs float64 over bf16 [-16, 16]: gelu {g:.4e}, derivative {dg:.4e}; '
          f'allowances {G.GELU_ALLOW:.3e}, {G.DGELU_ALLOW:.3e}')
    assert g <= G.GELU_ERR_MEASURED <= 1.01 * g
    assert dg <= G.DGELU_ERR_MEASURED <= 1.01 * dg
    assert G.GELU_ALLOW == 2 * G.GELU_ERR_MEASURED and G.DGELU_ALLOW == 2 * G.DGELU_ERR_MEASURED


def test_half_ulp_is_of_the_binade():
    """The 16-bit rounding term: a correctly rounded store of an exactly known value errs by up to half an ulp
    = 2^-9 (bf16) / 2^-12 (fp16) of the power of two closing the value's binade -- up to twice 2^-9 |value|,
    which therefore no kernel can meet; _r16 is that half ulp, attained and never exceeded."""
    x = torch.linspace(0.5, 4.0, 200001, dtype=torch.float64)
    zero = torch.zeros_like(x)
    for dt, rel in ((G.BF16, 2.0 ** -9), (G.F16, 2.0 ** -12)):
        err = (x.to(dt).double() - x).abs()
        assert (err / (rel * x)).max() > 1.9
        r = err / G._r16(x, zero, dt)
        assert 0.99 < r.max() <= 1.0


# ---------------------------------------------------------------- seeded faults
# One shape for all seven: M = 1032 (four 256-row tiles + 8 rows), N = 520 (two 256-column tiles + 8), K = 96
# (three 32-deep steps); large enough that a single wrong 8-column chunk moves the whole-matrix norm of a
# 16-bit output by ~ sqrt(16 / (M N)) = 5e-3, under the older tests' 1e-2.
FM, FN, FK, TILE = 1032, 520, 96, 256
FAULTS = ['1 chunk from the row above', '2 last ragged row not stored', '3 a row written at index M',
          '4 8 columns written at column N', '5 bias of the last column tile shifted by 16',
          '6 one K-step dropped for a 16-row strip', '7 a NaN pad column of A summed']
# where the older whole-matrix norm is SHOWN here to pass (asserted); elsewhere its verdict is only printed
OLD_PASSES = {('bf16', 1), ('bf16', 3), ('bf16', 4), ('bf16', 5), ('res', 3), ('res', 4)}


def _seed(c, fault):
    """the restated output with fault number `fault` seeded: (outs, before)"""
    op = c.op
    acc = bias = None
    r0 = FM // TILE * TILE                       # first row of the ragged row tile
    n0 = FN // TILE * TILE                       # first column of the last column tile
    if fault == 5:
        full = c.bias.as_strided((FN + G.PAD_C,), (1,))
        bias = c.bias.clone()
        bias[n0:] = full[n0 - 16:FN - 16]
    if fault == 6:
        acc = op.A.float() @ op.B.float().t()
        acc[r0:r0 + 16] -= op.A.float()[r0:r0 + 16, 32:64] @ op.B.float()[:, 32:64].t()
    if fault == 7:
        Af = c.Am.as_strided((FM, FK + 8), (c.Am.stride(0), 1)).float()
        Bf = c.Bm.as_strided((FN, FK + 8), (c.Bm.stride(0), 1)).float()
        acc = Af @ Bf.t()
    outs, before = _run(c, acc=acc, bias=bias)
    C = outs['C']
    if fault == 1:
        C.view[700, FN - 8:] = C.view[699, FN - 8:]
    if fault == 2:
        C.view[FM - 1] = before['C'][FM - 1, :FN]
    if fault == 3:
        C.buf[FM, :FN] = C.view[FM - 1]
    if fault == 4:
        C.buf[300, FN:FN + 8] = C.view[300, FN - 8:]
    return outs, before


@pytest.mark.parametrize('fault', range(1, 8), ids=FAULTS)
@pytest.mark.parametrize('kind', ['bf16', 'res'])
def test_seeded_fault_is_caught(kind, fault):
    c = G.make_case(kind, FM, FN, FK, True, True, CPU, family=128)
    if fault == 1:
        clean, before = _run(c)
        assert G.verify(c, clean, before).ok()
    outs, before = _seed(c, fault)
    rep = G.verify(c, outs, before)
    ref = c.op.P + c.bias.double() + (c.R.double() if kind == 'res' else 0)
    old = G.old_norm(outs['C'].view, ref)
    thr = G.OLD_NORM_16 if kind == 'bf16' else G.OLD_NORM_F32
    old_passes = old < thr
    print(f'fault {FAULTS[fault - 1]} ({kind} output): new checks fail: {"; ".join(rep.failed) or "NONE"}; '
          f'old whole-matrix norm {old:.3e} vs {thr:g}: {"would have PASSED" if old_passes else "fails"}')
    assert not rep.ok()
    want = 'guard' if fault in (3, 4) else 'bound'
    assert any(f.startswith(want) for f in rep.failed), rep.failed
    if (kind, fault) in OLD_PASSES:
        assert old_passes, old


@pytest.mark.parametrize('kind', ['argmax', 'geglu', 'slabs'])
def test_structural_faults(kind):
    """the kind-specific rules: an argmax tie resolved to the later column / an index at or beyond N, a
    GEGLU g chunk computed from the neighbouring 32-column pair, a store into the spare slab"""
    c = G.make_case(kind, 72, 128 if kind != 'argmax' else 72, 200, True, True, CPU, family=128)
    outs, before = _run(c)
    assert G.verify(c, outs, before).ok()
    if kind == 'argmax':
        idx = outs['C'].view[:, 1::2].contiguous().view(torch.int32)
        rows = (idx[:, 1] == 69).nonzero().flatten()      # the last group: columns 64 .. 71, 71 repeats 69
        assert len(rows)                         # the duplicated column does win somewhere
        idx[rows[0], 1] = 71
        outs['C'].view[:, 1::2] = idx.view(torch.float32)
        assert any('tie' in r for r in G.verify(c, outs, before).rules)
        idx[rows[0], 1], idx[3, 1] = 69, 72      # = N: outside
        outs['C'].view[:, 1::2] = idx.view(torch.float32)
        assert any('outside' in r for r in G.verify(c, outs, before).rules)
    elif kind == 'geglu':
        outs['C2'].view[9, 32:40] = outs['C2'].view[9, 0:8]
        assert not G.verify(c, outs, before).ok()
    else:
        outs['C'].buf[2, 0, :8] = 0.0
        assert G.verify(c, outs, before).guard == ['C']
