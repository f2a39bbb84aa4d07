"""Every kernel of peg.hip at its edges, through the C entry points on guard-banded buffers
(tests/peg_common.py): every element of out, dx, dweight and dbias against float64 within its derived bound, the
16-bit copies bit for bit, every margin untouched, no output element unwritten; the same launches on exact
integer operands with torch.equal; the reduce epilogue's accumulate and null-pointer forms; every launch repeated
bit-identically.  Each case of peg_common.CASES runs every entry point that takes its shape, in both modes; the
case notes name the kernels, and the route probes hold those notes against the library.  Each check prints
max(err / bound) per output; the module's largest per path are printed when it ends."""
import pytest
import torch

import ln_rows_common as LN
import peg_common as P

pytestmark = pytest.mark.gpu
dev = 'cuda'
RATIOS = {}


@pytest.fixture(scope='module')
def L():
    from ctclip_mi355x import _lib
    _lib.lib()
    yield _lib
    print('\nlargest error / bound per path:')
    for k in sorted(RATIOS):
        print(f'  {k}: {RATIOS[k]:.3f}')


@pytest.fixture(scope='module')
def K():
    from ctclip_mi355x import kernels
    return kernels


_GI = {}


def _inputs(name, kind):
    if (name, kind) not in _GI:
        _GI[(name, kind)] = P.guarded_inputs(P.operands(name, kind, dev))
    return _GI[(name, kind)]


def _note(path, rep):
    for k, v in rep.ratios.items():
        RATIOS[f'{path} {k}'] = max(RATIOS.get(f'{path} {k}', 0.0), v)


def _guards_ok(gi, outs, what):
    bad = P.guard_report({**vars(gi), **outs})
    assert not bad, (what, bad)


def _same(a, b, what):
    for k in a:
        assert torch.equal(P._ints(a[k].buf), P._ints(b[k].buf)), f'{what}: {k} differs between two launches'


def _check_rows(kind, path, label, name, got, ref, bound, case):
    """an [M, D] f32 output: torch.equal on exact operands, the per-element bound otherwise"""
    if kind == 'exact':
        neq = (got.double() != ref).nonzero()
        assert neq.numel() == 0, (f'{label} {name}: {neq.shape[0]} element(s) differ, first at (b, t, h, w) '
                                  f'{P.decode_row(neq[0, 0], case.geom)} c {int(neq[0, 1])}')
        return
    rep = P.verify([(name, got, ref, bound, 'rows')], case.geom, case.D, label=f'{label} {path}')
    _note(path, rep)
    assert rep.ok(), rep.failed


def _check_16(outs, f32, copies, what):
    for k, dt in copies:
        assert P.bits_equal(outs[k].view, outs[f32].view.to(dt)), f'{what}: {k} is not the rounded {f32}'


def _check_stats(L, outs, D, group, path, label):
    """the merged (mean, rstd) per row against float64 of the launch's own f32 output (ln_rows_common bounds)"""
    mr = P.merge_stats(outs['stats'], D, group)
    bad = P.guard_report({'stats': outs['stats'], **mr})
    assert not bad, (label, bad)
    outf = outs['out'].view
    b = LN.fwd_bounds(outf, None, None, P.EPS, LN.depth_peg(D, group), merged=True)
    _, mu, _, rs = LN.ln_ref(outf, None, None, P.EPS)
    zero = torch.zeros_like(mu)
    rm = P.G.ratio(mr['mean'].view.double(), mu, b['mean'])
    rr = P.G.ratio(mr['rstd'].view.double() / rs - 1, zero, b['rstd'])
    print(f'{label} {path}: mean {rm:.3f}, rstd {rr:.3f}')
    RATIOS[f'{path} mean'] = max(RATIOS.get(f'{path} mean', 0.0), rm)
    RATIOS[f'{path} rstd'] = max(RATIOS.get(f'{path} rstd', 0.0), rr)
    assert rm <= 1.0 and rr <= 1.0, (label, rm, rr)


def _check_wgrad(kind, path, label, red, ref, bd, case):
    dw, db = red['dweight'].view, red['dbias'].view
    if kind == 'exact':
        assert torch.equal(dw.double(), ref.dweight), f'{label}: dweight'
        assert torch.equal(db.double(), ref.dbias), f'{label}: dbias'
        return
    rep = P.verify([('dweight', dw, ref.dweight, bd.dweight, 'taps'), ('dbias', db, ref.dbias, bd.dbias, 'chan')],
                   case.geom, case.D, label=f'{label} {path}')
    _note(path, rep)
    assert rep.ok(), rep.failed


def _run_case(L, case, mode, kind, tag=''):
    """every entry point that takes the case's shape; tag names the cube's walk in the recorded paths"""
    geom, D = case.geom, case.D
    B, T, H, W = geom
    gi = _inputs(case.name, kind)
    r16, r32 = P.references(case.name, kind, mode, dev)
    cube = (T, H, W) == (24, 24, 24)
    label = f'{case.name} mode {mode}{tag} {kind}:'
    fam = 'cube' + tag if cube else ''
    if D % 8 == 0:      # the bf16-tap entry points
        tiled = P.tiled_ok(W, D)
        route = ((fam if tiled else '') or ('tiled' if tiled else 'general')) + ' bf16'
        nblk = L.lib().ctclip_peg_wgrad_slabs(*geom, D)
        assert nblk == P.wgrad_slabs(geom, D), (label, nblk)
        bd = P.bounds(r16, nblk)
        fw = P.launch_fwd(gi, geom, D, mode, stats=tiled)
        _guards_ok(gi, fw, label + ' fwd')
        _check_rows(kind, route + ' fwd', label, 'out', fw['out'].view, r16.out, bd.out, case)
        _check_16(fw, 'out', [('out_bf16', P.BF16)], label + ' fwd')
        if tiled and kind == 'random':
            _check_stats(L, fw, D, 64, route + ' stats', label)
        fw2 = P.launch_fwd(gi, geom, D, mode, stats=False)      # ctclip_peg_fwd: the same kernel without partials
        _guards_ok(gi, fw2, label + ' fwd (no stats)')
        _same(fw2, {k: fw[k] for k in fw2}, label + ' fwd')
        bw = P.launch_bwd_data(gi, geom, D, mode)
        _guards_ok(gi, bw, label + ' bwd_data')
        _check_rows(kind, route + ' bwd_data', label, 'dx', bw['dx'].view, r16.dx, bd.dx, case)
        _check_16(bw, 'dx', [('dx_bf16', P.BF16)], label + ' bwd_data')
        _same(P.launch_bwd_data(gi, geom, D, mode), bw, label + ' bwd_data')
        part = P.launch_bwd_weight(gi, geom, D, mode, nblk)
        _guards_ok(gi, {'part': part}, label + ' bwd_weight')
        red = P.launch_reduce(part, D)
        _guards_ok(gi, {'part': part, **red}, label + ' wgrad_reduce')
        _check_wgrad(kind, route + ' bwd_weight', label, red, r16, bd, case)
        _same({'part': P.launch_bwd_weight(gi, geom, D, mode, nblk)}, {'part': part}, label + ' bwd_weight')
    if D % 4 == 0:      # the f32-tap entry points
        xt = P.x32_tiled(W, D)
        route = (fam or ('tiled' if xt else 'naive')) + ' x32'
        bd = P.bounds(r32, 1)
        fx = P.launch_fwd_x32(gi, geom, D, mode, stats=xt)
        _guards_ok(gi, fx, label + ' fwd_x32')
        _check_rows(kind, route + ' fwd', label, 'out', fx['out'].view, r32.out, bd.out, case)
        _check_16(fx, 'out', [('out_bf16', P.BF16), ('out_f16', P.F16)], label + ' fwd_x32')
        if xt and kind == 'random':
            _check_stats(L, fx, D, 32, route + ' stats', label)
        _same(P.launch_fwd_x32(gi, geom, D, mode, stats=xt), fx, label + ' fwd_x32')
        if cube:
            bx = P.launch_bwd_data_x32(gi, geom, D, mode)
            _guards_ok(gi, bx, label + ' bwd_data_x32')
            _check_rows(kind, route + ' bwd_data', label, 'dx', bx['dx'].view, r32.dx, bd.dx, case)
            _check_16(bx, 'dx', [('dx_bf16', P.BF16)], label + ' bwd_data_x32')
            _same(P.launch_bwd_data_x32(gi, geom, D, mode), bx, label + ' bwd_data_x32')
        else:       # the x32 input gradient exists for the cube only: refused before any launch
            dx = P.Guard((P.ntok(geom), D), P.F32, dev)
            rc = L.lib().ctclip_peg_bwd_data_x32(L.ptr(gi.dyf.view), *geom, D, L.ptr(gi.w.view), mode, L.ptr(dx.view),
                                                 None, L.stream_ptr())
            assert rc == P.CT_ESHAPE and dx.unchanged()
    torch.cuda.synchronize()


# ------------------------------------------------------------------ (a) random operands, (b) exact integers, (d) repeat
@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('case', P.CASES, ids=lambda c: c.name)
def test_edges_random(L, case, mode):
    _run_case(L, case, mode, 'random')


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('case', P.CASES, ids=lambda c: c.name)
def test_edges_exact(L, case, mode):
    _run_case(L, case, mode, 'exact')


@pytest.mark.parametrize('kind', ['random', 'exact'])
@pytest.mark.parametrize('walk', ['mode0', 'mode1-canonical', 'mode1-view'])
@pytest.mark.parametrize('case', P.CUBE_CASES, ids=lambda c: c.name)
def test_cube(L, case, walk, kind):
    """the compile-time 24^3 kernels: <24, 0> (mode 0), <24, 2> (mode 1, canonical walk) and <24, 1> (mode 1 after
    ctclip_peg_set_canon1(0): the view walk)"""
    if walk != 'mode1-view':
        return _run_case(L, case, int(walk != 'mode0'), kind, tag=' ' + walk.split('-')[-1] if walk != 'mode0' else '')
    prev = L.lib().ctclip_peg_set_canon1(0)
    try:
        _run_case(L, case, 1, kind, tag=' view')
    finally:
        L.lib().ctclip_peg_set_canon1(prev)


# ------------------------------------------------------------------ route probes
def test_routes(L):
    """ctclip_peg_wgrad_slabs tells the bf16 route (B ceil(H / 2) slabs: tiled; 256: general) and the stats request
    the x32 one (refused with CT_EINVAL, before any launch, unless peg_fwd32_kernel takes the shape): the case
    notes' claims, held against the library"""
    slabs = L.lib().ctclip_peg_wgrad_slabs
    assert slabs(1, 3, 2, 24, 64) == 1 and slabs(1, 3, 2, 25, 64) == 256          # W = 24 | 25
    assert slabs(2, 3, 5, 7, 64) == 6 and slabs(2, 3, 5, 7, 72) == 256            # D = 64 | 72
    for c in P.CASES + P.CUBE_CASES:
        if c.D % 8 == 0:
            want = 'general' not in c.name and c.D % 64 == 0
            assert P.tiled_ok(c.geom[3], c.D) == want, c.name
            assert slabs(*c.geom, c.D) == (c.geom[0] * ((c.geom[2] + 1) // 2) if want else 256), c.name
        if c.D % 4 == 0 and not P.x32_tiled(c.geom[3], c.D):
            gi = _inputs(c.name, 'exact')
            M = P.ntok(c.geom)
            out, st = P.Guard((M, c.D), P.F32, dev), P.Guard((max(c.D // 32, 1), M, 2), P.F32, dev)
            rc = L.lib().ctclip_peg_fwd_x32s(L.ptr(gi.xf.view), *c.geom, c.D, L.ptr(gi.w.view), L.ptr(gi.bias.view), 0,
                                             L.ptr(out.view), None, None, None, L.ptr(st.view), None, L.stream_ptr())
            torch.cuda.synchronize()
            assert rc == P.CT_EINVAL and out.unchanged() and st.unchanged(), c.name
    assert {c.name for c in P.CASES if c.D % 4 == 0 and not P.x32_tiled(c.geom[3], c.D)} == {
        'general-1x3x2x25-D64', 'general-2x3x5x7-D72', 'general-1x2x3x5-D8', 'naive-1x2x3x5-D4', 'naive-2x3x5x7-D36',
        'naive-1x3x2x25-D32'}


# ------------------------------------------------------------------ (c) the reduce epilogue
REDUCE_CASES = ['tiled-3x1x5x7-D64', 'tiled-2x5x5x7-D128', 'general-2x3x5x7-D72']


def _sinks(D, kind):
    g = torch.Generator().manual_seed(5 + D)
    if kind == 'exact':      # integers: sink + gradient stays exact
        return (torch.randint(-100, 101, (D, 27), generator=g).float().to(dev),
                torch.randint(-100, 101, (D,), generator=g).float().to(dev))
    return torch.randn(D, 27, generator=g).to(dev), torch.randn(D, generator=g).to(dev)


def _check_acc(kind, label, got, sinks, ref, bd, case):
    """got {name: tensor} = sink + gradient: exact, or within the gradient's bound plus the one rounding of the sum"""
    spec = {'dweight': (ref.dweight, bd.dweight, 'taps'), 'dbias': (ref.dbias, bd.dbias, 'chan')}
    checks = []
    for k, t in got.items():
        gref, gbound, shape = spec[k]
        want = sinks[k].double() + gref
        if kind == 'exact':
            assert torch.equal(t.double(), want), f'{label}: {k}'
        else:
            checks.append((k, t, want, P.accumulate_bound(sinks[k], gref, gbound), shape))
    if checks:
        rep = P.verify(checks, case.geom, case.D, label=label)
        _note('reduce accumulate', rep)
        assert rep.ok(), rep.failed


@pytest.mark.parametrize('kind', ['random', 'exact'])
@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('name', REDUCE_CASES)
def test_reduce_epilogue(L, K, name, mode, kind):
    """ctclip_peg_wgrad_reduce: accumulate = 1 into non-zero sinks, either sink null (the other still right, the
    null one's buffer untouched), and the same through kernels.peg_bwd(dweight_out=, dbias_out=)"""
    case = P.CASE_BY_NAME[name]
    geom, D = case.geom, case.D
    gi, o = _inputs(name, kind), P.operands(name, kind, dev)
    ref, _ = P.references(name, kind, mode, dev)
    nblk = L.lib().ctclip_peg_wgrad_slabs(*geom, D)
    bd = P.bounds(ref, nblk)
    part = P.launch_bwd_weight(gi, geom, D, mode, nblk)
    part_bits = P._ints(part.buf).clone()
    sw, sb = _sinks(D, kind)
    sinks = {'dweight': sw, 'dbias': sb}
    zeros = {k: torch.zeros_like(v) for k, v in sinks.items()}
    label = f'{name} mode {mode} {kind}: reduce'
    red = P.launch_reduce(part, D, dw_sink=sw, db_sink=sb, accumulate=1)
    assert not P.guard_report({'part': part, **red}), label
    _check_acc(kind, label + ' accumulate', {k: g.view for k, g in red.items()}, sinks, ref, bd, case)
    for acc in (0, 1):
        for null, other in (('dweight', 'dbias'), ('dbias', 'dweight')):
            r = P.launch_reduce(part, D, dw_sink=sw, db_sink=sb, want_dw=null != 'dweight', want_db=null != 'dbias',
                                accumulate=acc)
            assert r[null].unchanged(), f'{label}: a null {null} was written'
            assert torch.equal(P._ints(part.buf), part_bits), f'{label}: the partial slabs were written'
            assert not P.guard_report(r), label
            _check_acc(kind, f'{label} accumulate {acc} null {null}', {other: r[other].view}, sinks if acc else zeros,
                       ref, bd, case)
    # through the wrapper, as training calls it
    dw_out, db_out = sw.clone(), sb.clone()
    dxf, dxb, dw, db = K.peg_bwd(o.dyb, o.dyf, o.xb, *geom, o.w, mode, dweight_out=dw_out, dbias_out=db_out)
    assert dw is dw_out and db is db_out
    _check_acc(kind, label + ' peg_bwd sinks', {'dweight': dw, 'dbias': db}, sinks, ref, bd, case)
    assert P.bits_equal(dw, red['dweight'].view) and P.bits_equal(db, red['dbias'].view)
    assert P.bits_equal(dxb, dxf.bfloat16())
    dxf2, _, dw2, db2 = K.peg_bwd(o.dyb, o.dyf, o.xb, *geom, o.w, mode)
    assert P.bits_equal(dxf2, dxf)
    _check_acc(kind, label + ' peg_bwd', {'dweight': dw2, 'dbias': db2}, zeros, ref, bd, case)
    torch.cuda.synchronize()
