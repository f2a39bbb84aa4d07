"""tests/peg_common.py checked without a GPU: the float64 reference agrees with the oracle and with
autograd through it; a plain f32 evaluation of the same operation stays inside the per-element bounds on every
case of the list (the bounds are not too tight); planted single-voxel / single-tap faults are caught by verify
while the older whole-tensor norm figure lets the input-localised ones through; the guard helpers see a
one-element stray write and an unwritten element."""
import os
import re

import pytest
import torch

import peg_common as P
from oracle import ctclip_oracle as O

ALL_CASES = P.CASES + P.CUBE_CASES
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _oracle(x, w, b, geom, mode):
    """x + PEG(x) through the oracle, canonical rows (tests/test_gpu_ops.py _peg_ref)"""
    B, T, H, W = geom
    D = x.shape[1]
    sd = {'p.dsconv.weight': w.reshape(D, 1, 3, 3, 3), 'p.dsconv.bias': b}
    if mode == 0:
        xs = x.reshape(B * T, H * W, D)
        return (O.peg_forward(sd, 'p.', xs, geom) + xs).reshape(-1, D)
    xt = x.reshape(B, T, H, W, D).permute(0, 2, 3, 1, 4).reshape(B * H * W, T, D)
    y = O.peg_forward(sd, 'p.', xt, geom) + xt
    return y.reshape(B, H, W, T, D).permute(0, 3, 1, 2, 4).reshape(-1, D)


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('geom', [(2, 5, 3, 4), (3, 1, 5, 7), (1, 2, 3, 6), (2, 3, 5, 1)])
def test_reference_matches_oracle(geom, mode):
    torch.manual_seed(3)
    M, D = P.ntok(geom), 8
    x = torch.randn(M, D, dtype=P.F64, requires_grad=True)
    w = torch.randn(D, 27, dtype=P.F64, requires_grad=True)
    b = torch.randn(D, dtype=P.F64, requires_grad=True)
    dy = torch.randn(M, D, dtype=P.F64)
    y = _oracle(x, w, b, geom, mode)
    y.backward(dy)
    r = P.reference(x.detach(), w.detach(), b.detach(), dy, geom, mode)
    for name, got, want in (('out', r.out, y.detach()), ('dx', r.dx, x.grad), ('dweight', r.dweight, w.grad),
                            ('dbias', r.dbias, b.grad)):
        assert (got - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item()), name
    # the separate residual tensors of the bf16 kernels enter linearly
    res, dres = torch.randn(M, D, dtype=P.F64), torch.randn(M, D, dtype=P.F64)
    r2 = P.reference(x.detach(), w.detach(), b.detach(), dy, geom, mode, res=res, dres=dres)
    assert (r2.out - (r.out - x.detach() + res)).abs().max().item() <= 1e-12
    assert (r2.dx - (r.dx - dy + dres)).abs().max().item() <= 1e-12
    assert torch.equal(r2.dweight, r.dweight)


def test_geometry_constants_match_the_kernel_file():
    """the restated launch geometry is peg.hip's, and the tiled limit it implies is W = 24 for both tap types"""
    src = open(os.path.join(REPO, 'ctpa-clip_amd', 'csrc', 'peg.hip')).read()
    for name in ('HT', 'SEG', 'SEGW', 'WNTH', 'PLANE_CH', 'XC', 'XHT', 'XNT', 'XPCH'):
        m = re.search(r'\b' + name + r' = (\d+)[,;]', src)
        assert m and int(m.group(1)) == getattr(P, name), name
    assert P.TNTH == P.HT * P.cdiv(24, P.SEG) * 8
    assert P.tiled_ok(24, 64) and not P.tiled_ok(25, 64) and not P.tiled_ok(24, 72)
    assert P.x32_tiled(24, 32) and not P.x32_tiled(25, 32) and not P.x32_tiled(24, 36)
    assert P.wgrad_slabs((1, 3, 2, 24), 64) == 1 and P.wgrad_slabs((1, 3, 2, 25), 64) == 256
    assert P.wgrad_slabs((2, 3, 5, 7), 64) == 6 and P.wgrad_slabs((2, 3, 5, 7), 72) == 256


def test_case_list_covers_the_issue():
    geoms = {c.geom for c in P.CASES if c.name.startswith('tiled') and c.D == 64}
    for g in [(1, 1, 1, 1), (3, 1, 5, 7), (2, 2, 1, 24), (1, 3, 2, 3), (2, 5, 5, 7), (1, 2, 3, 6)]:
        assert g in geoms
    for axis, need in ((1, {1, 2, 3, 5}), (2, {1, 2, 3, 4, 5, 9}), (3, {1, 3, 4, 6, 7, 24})):
        assert need <= {g[axis] for g in geoms}
    assert max(g[0] for g in geoms) > 2
    assert len({c.name for c in ALL_CASES}) == len(ALL_CASES)
    for c in P.CASES:
        if c.geom != (1, 1, 1, 1):
            assert len(set(c.geom[1:])) > 1, c.name      # no cube: mode 1 is not an axis permutation of the rows


RATIOS = {}


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('case', ALL_CASES, ids=lambda c: c.name)
def test_f32_evaluation_within_bounds(case, mode):
    """the operation in plain f32 torch on the CPU, both tap sources: max(err / bound) < 1 on every output"""
    o = P.operands(case.name, 'random')
    r16, r32 = P.references(case.name, 'random', mode)
    for tag, ref, x, res, dy, dres in (('bf16 taps', r16, o.xb, o.xf, o.dyb, o.dyf), ('f32 taps', r32, o.xf, None, o.dyf, None)):
        bd = P.bounds(ref, nslab=1)
        out = P.model_f32(x, o.w, o.bias, case.geom, mode, res=res)
        dx, dw, db = P.grads_f32(dy, x, o.w, case.geom, mode, dres=dres)
        rep = P.verify([('out', out, ref.out, bd.out, 'rows'), ('dx', dx, ref.dx, bd.dx, 'rows'),
                        ('dweight', dw, ref.dweight, bd.dweight, 'taps'), ('dbias', db, ref.dbias, bd.dbias, 'chan')],
                       case.geom, case.D, label=f'f32 CPU {case.name} mode {mode} {tag}')
        assert rep.ok(), rep.failed
        for k, v in rep.ratios.items():
            RATIOS[k] = max(RATIOS.get(k, 0.0), v)
    print('largest so far: ' + ', '.join(f'{k} {v:.3f}' for k, v in RATIOS.items()))


def test_exact_operands_are_exact_in_f32():
    """the integer / half operands: the plain f32 evaluation equals float64 exactly, on the cube too (the largest
    weight-gradient sum)"""
    for name in ('tiled-2x5x5x7-D64', 'general-2x3x5x7-D72', 'cube-D32'):
        case = P.CASE_BY_NAME[name]
        o = P.operands(name, 'exact')
        for mode in (0, 1):
            r16, _ = P.references(name, 'exact', mode)
            assert torch.equal(o.xb.float(), o.xf)
            assert r16.dweight_abs.max().item() < 2 ** 23 and r16.out_abs.max().item() < 2 ** 23
            out = P.model_f32(o.xb, o.w, o.bias, case.geom, mode, res=o.xf)
            dx, dw, db = P.grads_f32(o.dyb, o.xb, o.w, case.geom, mode, dres=o.dyf)
            assert torch.equal(out.double(), r16.out) and torch.equal(dx.double(), r16.dx)
            assert torch.equal(dw.double(), r16.dweight) and torch.equal(db.double(), r16.dbias)


FAULT_CASE = {'corner_tap': ('tiled-2x5x5x7-D64', 0), 'halo_wrap': ('tiled-2x5x5x7-D64', 0),
              'prev_batch': ('tiled-2x5x5x7-D64', 1), 'noncausal_tap': ('tiled-1x3x2x3-D64', 0),
              'mode_map': ('tiled-1x2x3x6-D64', 1), 'last_channel': ('general-2x3x5x7-D72', 0)}


@pytest.mark.parametrize('fault', P.FAULTS)
def test_planted_fault_is_caught(fault):
    """Every fault fails verify.  The local ones are planted where the input they add or drop is smallest and
    where it is largest: both fail verify; at the small site the whole-tensor norm of the older tests stays under
    its 1e-5 threshold (printed), which is the gap the per-element bound closes."""
    name, mode = FAULT_CASE[fault]
    case = P.CASE_BY_NAME[name]
    o = P.operands(name, 'random')
    ref, _ = P.references(name, 'random', mode)
    bd = P.bounds(ref, nslab=1)
    good = P.model_f32(o.xb, o.w, o.bias, case.geom, mode, res=o.xf)
    assert P.verify([('out', good, ref.out, bd.out, 'rows')], case.geom, case.D).ok()
    assert P.old_norm(good, ref.out) < P.OLD_NORM_TOL
    if fault in P.FAULTS_GLOBAL:
        bad = P.model_f32(o.xb, o.w, o.bias, case.geom, mode, res=o.xf, fault=fault)
        rep = P.verify([('out', bad, ref.out, bd.out, 'rows')], case.geom, case.D, label=f'fault {fault} on {name}')
        assert not rep.ok() and rep.ratios['out'] > 1
        return
    rows = P.view_rows(case.geom, mode)
    sites = P.fault_sites(fault, case.geom)
    mag = [o.xb.float()[rows[P.fault_source(fault, s)[0]]].abs().max().item() for s in sites]
    order = sorted(range(len(sites)), key=lambda i: mag[i])
    for which, i in (('smallest', order[0]), ('largest', order[-1])):
        bad = P.model_f32(o.xb, o.w, o.bias, case.geom, mode, res=o.xf, fault=fault, site=sites[i])
        assert int((bad != good).any(1).sum()) == 1, 'the fault touches one voxel'
        rep = P.verify([('out', bad, ref.out, bd.out, 'rows')], case.geom, case.D,
                       label=f'fault {fault} on {name} at view voxel {sites[i]} ({which} input, max |x| {mag[i]:.3g})')
        norm = P.old_norm(bad, ref.out)
        print(f'  whole-tensor norm figure {norm:.3e} (threshold {P.OLD_NORM_TOL:g})')
        assert not rep.ok() and rep.ratios['out'] > 1
        b, t, h, w = P.decode_row(rows[sites[i]], case.geom)
        assert f'(b {b}, t {t}, h {h}, w {w},' in rep.failed[0], 'verify names the voxel'
        if which == 'smallest':
            assert norm < P.OLD_NORM_TOL, 'the older norm test lets this fault through'


def test_guard_helpers():
    dev = torch.device('cpu')
    for dtype, shape in ((P.F32, (5, 12)), (P.BF16, (5, 8)), (P.F16, (3, 8)), (P.F32, (7,)), (P.F32, (2, 5, 2))):
        g = P.Guard(shape, dtype, dev)
        assert g.pad * g.buf.element_size() % 16 == 0 and g.view.shape == shape
        assert g.margins_intact() and g.unwritten() == g.n
        assert P.guard_report({'o': g}) == [f'o: {g.n} element(s) unwritten']
        g.view.copy_(torch.ones(shape))
        assert P.guard_report({'o': g}) == []
        g.view.reshape(-1)[g.n // 2] = float('nan')
        assert P.guard_report({'o': g}) == ['o: 1 NaN element(s)']
        g.view.copy_(torch.ones(shape))
        P._ints(g.view).reshape(-1)[-1] = P.SENT32 if dtype == P.F32 else P.SENT16
        assert P.guard_report({'o': g}) == ['o: 1 element(s) unwritten']
        g.view.copy_(torch.ones(shape))
        for at in (g.pad - 1, g.pad + g.n, 0, g.buf.numel() - 1):       # one element into either margin
            keep = g.buf[at].clone()
            g.buf[at] = 1.0
            assert P.guard_report({'o': g}) == ['o: a margin changed'], at
            g.buf[at] = keep
            assert P.guard_report({'o': g}) == []
    x = torch.randn(4, 8)
    gi = P.Guard(x.shape, P.F32, dev, data=x)
    assert torch.equal(gi.view, x) and torch.isnan(gi.buf[:gi.pad]).all() and torch.isnan(gi.buf[gi.pad + gi.n:]).all()
    assert P.guard_report({'x': gi}) == []
    gi.view[1, 2] += 1
    assert P.guard_report({'x': gi}) == ['x: an operand was written']
    sink = P.Guard((4, 8), P.F32, dev, live=x)
    assert torch.equal(sink.view, x) and P.guard_report({'s': sink}) == []


def test_verify_reports_taps_and_nonfinite():
    ref = torch.zeros(4, 27, dtype=P.F64)
    got = ref.clone()
    got[2, 14] = 1.0
    rep = P.verify([('dweight', got, ref, torch.full_like(ref, 1e-3), 'taps')], (1, 1, 1, 1), 4)
    assert not rep.ok() and '(c 2, tap kt 1 kh 1 kw 2)' in rep.failed[0]
    got[2, 14] = float('nan')
    assert P.verify([('dweight', got, ref, torch.full_like(ref, 1e-3), 'taps')], (1, 1, 1, 1), 4).ratios['dweight'] == float('inf')
    assert P.verify([('dbias', torch.zeros(4), torch.zeros(4), torch.zeros(4), 'chan')], (1, 1, 1, 1), 4).ok()
    assert not P.verify([('dbias', torch.full((4,), 1e-30), torch.zeros(4), torch.zeros(4), 'chan')], (1, 1, 1, 1), 4).ok()
