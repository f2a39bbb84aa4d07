"""PEG (peg.hip) at its edges: a float64 reference written from the header of peg.hip, per-element
bounds, guard-banded buffers and the case list shared by tests/test_peg_cpu.py (checks the checks, no GPU) and
tests/test_gpu_peg_edges.py.

The operation (peg.hip header): out(v) = x(v) + bias + sum_{kt,kh,kw} w[c][kt][kh][kw] x(v + (kt-2, kh-1, kw-1)),
zero outside the (T, H, W) grid of the *view*; rows live in canonical (b, t, h, w) order.  Mode 0: view ==
canonical.  Mode 1: view position p = (h W + w) T + t  <->  canonical row t H W + h W + w.

Bounds (u = 2^-24, the f32 unit roundoff; none is fitted to a kernel's output).
  out / dx   An output is a sum of at most 29 terms: 27 products, the bias, the residual.  Every product is rounded
             once (or not at all, under an fma) and the 29 terms are joined by 28 additions in some order, so no
             term passes through more than 1 + 28 = 29 roundings: |fl - exact| <= gamma_29 sum|terms| (Higham,
             Accuracy and Stability, (4.4)), gamma_29 = 29 u / (1 - 29 u) <= 29 u SLACK.  sum|terms| is the
             absolute-value convolution |x| + |bias| + sum |w| |x_neighbour|:  bound = 29 SLACK u abs-conv.
             The same constant serves dx (28 terms, no bias) and every walk order (the rolling accumulators of
             the x32 kernel start from the bias and end with the residual: the same 29 terms).
  dweight    tap k of channel c sums n_k products dout x (n_k = the tokens whose tap k lies inside the grid),
             spread over `nslab` partial slabs that the reduce kernel then adds.  One rounding per product, at most
             n_k - 1 additions inside the slabs (empty lanes add exact zeros) and nslab across them:
             bound = (n_k + nslab) SLACK u sum|dout x|, whatever the order.  dbias: n = all tokens.
             accumulate = 1 adds one rounding of the result: + u (|sink| + |grad| + bound).
  16-bit     out_bf16 / out_f16 / dx_bf16 are the round-to-nearest-even casts of the same launch's f32 output,
             bit for bit: no tolerance."""
import functools
import types
from collections import namedtuple

import torch

import gemm_edge_common as G

BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
U = 2.0 ** -24
SLACK = G.SLACK
C_CONV = 29 * SLACK              # 27 products + bias + residual, see the docstring
PAD_ROWS = 8                     # guard rows before and after every buffer (8 rows keep 16-byte alignment)
SENT32, SENT16 = G.SENT32, G.SENT16
OLD_NORM_TOL = 1e-5              # test_gpu_ops.py test_peg: ||got - ref|| / ||ref|| over the whole tensor
CT_EINVAL, CT_ESHAPE = 1001, 1003    # common.h
EPS = 1e-5

# peg.hip's launch geometry, restated (the route probes of the GPU test hold these against the library)
HT, SEG, SEGW, TNTH, WNTH, PLANE_CH = 2, 3, 6, 128, 256, 1024
XC, XHT, XNT, XPCH = 32, 4, 256, 1280
GENERAL_SLABS = 256


def cdiv(a, b):
    return (a + b - 1) // b


def tiled_ok(W, D):
    """peg.hip tiled_ok: the bf16 plane-streaming kernels take the shape.  The thread budgets bind first:
    HT ceil(W / SEG) 8 <= TNTH and HT ceil(W / SEGW) 32 <= WNTH both give W <= 24 (the plane holds W <= 30)."""
    return (D % 64 == 0 and HT * cdiv(W, SEG) * 8 <= TNTH and (HT + 2) * (W + 2) * 8 <= PLANE_CH
            and HT * cdiv(W, SEGW) * 32 <= WNTH)


def x32_tiled(W, D):
    """ctclip_peg_fwd_x32s: peg_fwd32_kernel (W <= 24, D % 32 == 0) or the naive kernel"""
    return D % XC == 0 and XHT * cdiv(W, SEG) * 8 <= XNT and (XHT + 2) * (W + 2) * 8 <= XPCH


def wgrad_slabs(geom, D):
    B, T, H, W = geom
    return B * cdiv(H, HT) if tiled_ok(W, D) else GENERAL_SLABS


# ------------------------------------------------------------------ cases
Case = namedtuple('Case', 'name geom D note')

# (B, T, H, W) of the runtime-geometry tiled kernels: peg_tile_kernel<TR>, peg_wgrad_tile_kernel<> (D % 64 == 0)
# and peg_fwd32_kernel<> (D % 32 == 0).  HT = 2 rows per workgroup (XHT = 4 for x32), SEG = 3 / SEGW = 6 columns
# per thread, a 3-slot plane ring (2-slot for x32).
TILED_GEOMS = [
    ((1, 1, 1, 1), 'one token: T below the ring depth, H = 1 below a tile, W = 1 below a segment'),
    ((3, 1, 5, 7), 'B = 3; T = 1 (no plane is prefetched); H = 5: 2+2+1 / 4+1 tiles; W = 7: segments 3+3+1, 6+1'),
    ((2, 2, 1, 24), 'T = 2 (tq + 1 < T never true); H = 1; W = 24, the widest tiled grid, every thread busy'),
    ((1, 3, 2, 3), 'T = 3 = ring depth (each slot written once); H = HT exactly; W = SEG exactly'),
    ((2, 5, 5, 7), 'T = 5: the ring wraps; ragged H and W; two batch elements (plane 0 after the other batch)'),
    ((1, 2, 3, 6), 'H = 3: 2+1 rows; W = SEGW exactly (one wgrad segment, two conv segments)'),
    ((1, 5, 3, 4), 'W = 4 = SEG + 1: a one-column second segment'),
    ((1, 3, 5, 1), 'W = 1: both halo columns are the plane padding'),
    ((4, 2, 5, 3), 'B = 4 with a ragged last H tile: batch / tile split of blockIdx.x'),
    ((1, 5, 2, 24), 'W = 24 with the ring wrapping, H = HT: the full 128 / 256 thread items'),
    ((1, 2, 4, 7), 'H = XHT exactly (one x32 tile, two bf16 tiles)'),
    ((1, 3, 9, 4), 'H = 9: the x32 4+4+1 split (bf16 2+2+2+2+1)'),
]


def _cases():
    cs = []
    for geom, note in TILED_GEOMS:
        tag = 'x'.join(map(str, geom))
        cs.append(Case(f'tiled-{tag}-D64', geom, 64, 'bf16 peg_tile_kernel<TR> / peg_wgrad_tile_kernel<>, x32 '
                       'peg_fwd32_kernel<> (two channel blocks): ' + note))
        cs.append(Case(f'tiled-{tag}-D32', geom, 32, 'x32 peg_fwd32_kernel<> (one channel block); bf16 general '
                       'kernels (D % 64 != 0, a half-filled channel block): ' + note))
    cs += [
        Case('tiled-2x5x5x7-D128', (2, 5, 5, 7), 128, 'bf16 tiled, two 64-channel blocks (blockIdx.y = 1, the stats '
             'partial of the second group); x32 four blocks'),
        Case('tiled-1x3x2x24-D64', (1, 3, 2, 24), 64, 'W = 24: the last tiled width (route probe against W = 25)'),
        Case('general-1x3x2x25-D64', (1, 3, 2, 25), 64, 'W = 25: the first width past the tiled limit: peg_kernel<TR>, '
             'peg_wgrad_kernel (256 slabs), x32 peg_fwd32_naive_kernel'),
        Case('general-2x3x5x7-D72', (2, 3, 5, 7), 72, 'bf16 general kernels with a full and a partial (8 of 64) channel '
             'block, 210 tokens = 6 x 32 + 18; x32 naive (72 % 32 != 0)'),
        Case('tiled-2x3x5x7-D64', (2, 3, 5, 7), 64, 'the D = 72 geometry at D = 64: tiled (route probe against D = 72)'),
        Case('general-1x2x3x5-D8', (1, 2, 3, 5), 8, 'the smallest channel count of the bf16 kernels (one chunk of 8); '
             'x32 naive'),
        Case('naive-1x2x3x5-D4', (1, 2, 3, 5), 4, 'x32 naive kernel at its smallest channel count (no bf16 entry point)'),
        Case('naive-2x3x5x7-D36', (2, 3, 5, 7), 36, 'x32 naive kernel, D % 32 != 0 and D % 8 != 0'),
        Case('naive-1x3x2x25-D32', (1, 3, 2, 25), 32, 'x32 naive kernel by width: W = 25 at D = 32; bf16 general'),
    ]
    return cs


CASES = _cases()
# The compile-time cube (T = H = W = 24).  Mode 0: peg_tile_kernel<TR,24,0>, peg_fwd32_kernel<24,0,0|1>,
# peg_wgrad_tile_kernel<24,0>; mode 1: the canonical walk <.,24,2> and, after ctclip_peg_set_canon1(0), the
# view walk <.,24,1>.  The x32 input gradient (ctclip_peg_bwd_data_x32) exists only here.
CUBE_CASES = [
    Case('cube-D64', (1, 24, 24, 24), 64, 'bf16 fixed-24 kernels, one channel block; x32 fixed-24 forward and input '
         'gradient, two channel blocks'),
    Case('cube-D32', (1, 24, 24, 24), 32, 'x32 fixed-24 forward and input gradient, one channel block (bf16: general)'),
]
CASE_BY_NAME = {c.name: c for c in CASES + CUBE_CASES}


def ntok(geom):
    B, T, H, W = geom
    return B * T * H * W


# ------------------------------------------------------------------ index maps
def view_rows(geom, mode, device='cpu'):
    """[B, T, H, W] long: the canonical row of each view position"""
    B, T, H, W = geom
    thw = T * H * W
    p = torch.arange(thw, device=device)
    rows = p if mode == 0 else (p % T) * (H * W) + p // T
    return (torch.arange(B, device=device)[:, None] * thw + rows[None]).view(B, T, H, W)


def decode_row(row, geom):
    """canonical row -> (b, t, h, w)"""
    B, T, H, W = geom
    b, r = divmod(int(row), T * H * W)
    t, r = divmod(r, H * W)
    h, w = divmod(r, W)
    return b, t, h, w


def tap_counts(geom):
    """[27] the number of tokens whose tap (kt, kh, kw) lies inside the grid"""
    B, T, H, W = geom
    n = []
    for kt in range(3):
        for kh in range(3):
            for kw in range(3):
                n.append(B * max(T - abs(kt - 2), 0) * max(H - abs(kh - 1), 0) * max(W - abs(kw - 1), 0))
    return torch.tensor(n, dtype=F64)


# ------------------------------------------------------------------ float64 reference and bounds
def _pad(v, front_t, back_t):
    """[B, T, H, W, D] -> zero halo of one in h and w and (front_t, back_t) in t"""
    B, T, H, W, D = v.shape
    p = v.new_zeros(B, T + front_t + back_t, H + 2, W + 2, D)
    p[:, front_t:front_t + T, 1:H + 1, 1:W + 1] = v
    return p


def reference(x, w, bias, dout, geom, mode, res=None, dres=None):
    """The operation and its gradients in float64 by explicit index arithmetic.  x / dout [M, D]: what the conv
    taps read (canonical rows); res / dres: the residual terms where they are separate tensors (the bf16 kernels
    read the taps from the bf16 copy and the residual from f32); w [D, 27]; bias [D].  Returns out, dx, dweight
    [D, 27], dbias [D] with the sums of absolute terms *_abs that the bounds scale."""
    B, T, H, W = geom
    M, D = x.shape
    rows = view_rows(geom, mode, x.device).reshape(-1)
    d64 = lambda t: t.double()  # noqa: E731
    w, bias = d64(w).reshape(D, 27), d64(bias)
    xv = d64(x)[rows].view(B, T, H, W, D)
    dv = d64(dout)[rows].view(B, T, H, W, D)
    rv = xv if res is None else d64(res)[rows].view(B, T, H, W, D)
    drv = dv if dres is None else d64(dres)[rows].view(B, T, H, W, D)
    xp, dp = _pad(xv, 2, 0), _pad(dv, 0, 2)
    out, out_abs = rv + bias, rv.abs() + bias.abs()
    dx, dx_abs = drv.clone(), drv.abs()
    dw, dw_abs = w.new_zeros(D, 27), w.new_zeros(D, 27)
    for kt in range(3):
        for kh in range(3):
            for kw in range(3):
                k = (kt * 3 + kh) * 3 + kw
                xn = xp[:, kt:kt + T, kh:kh + H, kw:kw + W]              # x(v + (kt - 2, kh - 1, kw - 1))
                dn = dp[:, 2 - kt:2 - kt + T, 2 - kh:2 - kh + H, 2 - kw:2 - kw + W]   # dout(v - offset)
                out = out + w[:, k] * xn
                out_abs = out_abs + w[:, k].abs() * xn.abs()
                dx = dx + w[:, k] * dn
                dx_abs = dx_abs + w[:, k].abs() * dn.abs()
                dw[:, k] = (dv * xn).sum((0, 1, 2, 3))
                dw_abs[:, k] = (dv * xn).abs().sum((0, 1, 2, 3))

    def canon(v):
        o = torch.empty(M, D, dtype=F64, device=x.device)
        o[rows] = v.reshape(M, D)
        return o
    return types.SimpleNamespace(out=canon(out), out_abs=canon(out_abs), dx=canon(dx), dx_abs=canon(dx_abs),
                                 dweight=dw, dweight_abs=dw_abs, dbias=dv.sum((0, 1, 2, 3)),
                                 dbias_abs=dv.abs().sum((0, 1, 2, 3)), geom=geom, mode=mode)


def bounds(ref, nslab):
    """per-element bounds of (out, dx, dweight, dbias), see the module docstring"""
    n = tap_counts(ref.geom).to(ref.dweight.device)
    return types.SimpleNamespace(out=C_CONV * U * ref.out_abs, dx=C_CONV * U * ref.dx_abs,
                                 dweight=(n[None] + nslab) * SLACK * U * ref.dweight_abs,
                                 dbias=(ntok(ref.geom) + nslab) * SLACK * U * ref.dbias_abs)


def accumulate_bound(sink, grad_ref, grad_bound):
    """sink + grad in f32: the gradient's own bound plus one rounding of the sum"""
    return grad_bound + U * (sink.double().abs() + grad_ref.abs() + grad_bound)


def old_norm(got, ref):
    """the existing tests' figure (test_gpu_ops.py rel)"""
    return ((got.double() - ref.double()).norm() / ref.double().norm().clamp_min(1e-30)).item()


# ------------------------------------------------------------------ verify
def _where(kind, idx, geom, D):
    if kind == 'rows':
        row, c = divmod(idx, D)
        b, t, h, w = decode_row(row, geom)
        return f'(b {b}, t {t}, h {h}, w {w}, c {c})'
    if kind == 'taps':
        c, k = divmod(idx, 27)
        return f'(c {c}, tap kt {k // 9} kh {k // 3 % 3} kw {k % 3})'
    return f'(c {idx})'


def verify(checks, geom, D, label='', show=4):
    """checks: [(name, got, ref, bound, kind)], kind 'rows' ([M, D] canonical rows), 'taps' ([D, 27]) or 'chan'
    ([D]).  Returns a report: ratios {name: max err / bound over ALL elements, inf where an output is not
    finite or misses a zero bound}, failed [str] naming the worst coordinates decoded to (b, t, h, w, c) / tap;
    ok().  Prints the ratios when a label is given, so a run's log records the margins."""
    rep = types.SimpleNamespace(ratios={}, failed=[])
    for name, got, ref, bound, kind in checks:
        got, ref, bound = got.double().reshape(-1), ref.double().reshape(-1), bound.double().reshape(-1)
        assert got.shape == ref.shape == bound.shape, (name, got.shape, ref.shape, bound.shape)
        assert torch.isfinite(ref).all() and torch.isfinite(bound).all() and (bound >= 0).all(), name
        err = (got - ref).abs()
        r = torch.where(err == 0, torch.zeros_like(err), err / bound)
        r = torch.where(torch.isfinite(r), r, torch.full_like(r, float('inf')))
        rep.ratios[name] = r.max().item() if r.numel() else 0.0
        nbad = int((r > 1.0).sum())
        if nbad:
            worst = torch.argsort(r, descending=True)[:show].tolist()
            rep.failed.append(f'{name}: {nbad} element(s) over the bound; worst ' + '; '.join(
                f'{_where(kind, i, geom, D)} got {got[i].item():.9g} ref {ref[i].item():.9g} err/bound '
                f'{r[i].item():.3g}' for i in worst))
    rep.ok = lambda: not rep.failed
    if label:
        print(f'{label}: ' + ', '.join(f'{k} {v:.3f}' for k, v in rep.ratios.items())
              + ('' if rep.ok() else '  FAILED ' + ' | '.join(rep.failed)))
    return rep


def bits_equal(a, b):
    ints = lambda t: t.contiguous().view(torch.int32 if t.dtype == F32 else torch.int16)  # noqa: E731
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(ints(a), ints(b))


# ------------------------------------------------------------------ guard bands
def _ints(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


class Guard:
    """A tensor of `shape` inside a flat buffer with PAD_ROWS whole rows (a row = the trailing dimensions) before
    and after it.  data given: an operand, margins NaN.  data None: an output, margins and live region the NaN
    sentinel.  live given: an output that starts from values (an accumulate sink), margins the sentinel."""

    def __init__(self, shape, dtype, device, data=None, live=None):
        shape = tuple(shape)
        n = 1
        for s in shape:
            n *= s
        self.pad = PAD_ROWS * max(n // max(shape[0], 1), 1)
        self.n, self.shape, self.is_input = n, shape, data is not None
        if data is not None:
            self.buf = torch.full((n + 2 * self.pad,), float('nan'), dtype=dtype, device=device)
            self.view.copy_(data.reshape(shape))
        else:
            sent = SENT32 if dtype == F32 else SENT16
            self.buf = torch.full((n + 2 * self.pad,), sent, device=device,
                                  dtype=torch.int32 if dtype == F32 else torch.int16).view(dtype)
            if live is not None:
                self.view.copy_(live.reshape(shape))
        self.before = _ints(self.buf).clone()

    @property
    def view(self):
        return self.buf[self.pad:self.pad + self.n].view(self.shape)

    def margins_intact(self):
        a, b = _ints(self.buf), self.before
        return torch.equal(a[:self.pad], b[:self.pad]) and torch.equal(a[self.pad + self.n:], b[self.pad + self.n:])

    def unchanged(self):
        return torch.equal(_ints(self.buf), self.before)

    def unwritten(self):
        """elements of the live region still holding the sentinel"""
        v = _ints(self.buf)[self.pad:self.pad + self.n]
        return int((v == (SENT32 if self.buf.dtype == F32 else SENT16)).sum())

    def nans(self):
        return int(torch.isnan(self.view).sum())


def guard_report(guards, outputs=None):
    """guards: {name: Guard}.  Every margin byte-identical, every operand untouched, and for the names in
    `outputs` (default: every non-operand) no element unwritten and none NaN.  Returns the list of violations."""
    bad = []
    for k, g in guards.items():
        if g is None:
            continue
        if not g.margins_intact():
            bad.append(f'{k}: a margin changed')
        if g.is_input:
            if not g.unchanged():
                bad.append(f'{k}: an operand was written')
        elif outputs is None or k in outputs:
            if g.unwritten():
                bad.append(f'{k}: {g.unwritten()} element(s) unwritten')
            elif g.nans():
                bad.append(f'{k}: {g.nans()} NaN element(s)')
    return bad


# ------------------------------------------------------------------ operands
@functools.lru_cache(maxsize=None)
def operands(name, kind, device='cpu'):
    """kind 'random': x / dout f32 values that bf16 cannot hold (xb / dyb their bf16 copies: the bf16 kernels read
    the taps from the copy and the residual from f32, as training does), each token scaled by a power of two in
    2^0 .. 2^-15 (token magnitudes spread as a residual stream's do: a per-element bound is relative to the
    token's own neighbourhood, a whole-tensor norm to the largest tokens); weights 0.2 randn, bias 0.1 randn.
    kind 'exact': x, dout integers in [-4, 4], weights and bias multiples of 1/2 in [-2, 2].  Every product is
    a multiple of 1/2 of magnitude <= 16 and every partial sum of the largest weight-gradient sum, over the
    13,824 tokens of the 24^3 cube, has magnitude <= 13,824 x 16 = 221,184 < 2^23: multiples of 1/2 below
    2^23 are exact in f32, so every result is exact in any summation order."""
    c = CASE_BY_NAME[name]
    M, D = ntok(c.geom), c.D
    g = torch.Generator().manual_seed(sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) + (kind == 'exact'))
    if kind == 'random':
        scale = torch.ldexp(torch.ones(M, 1), -torch.randint(0, 16, (M, 1), generator=g))
        xf = (torch.randn(M, D, generator=g) + 0.25) * scale
        dyf = torch.randn(M, D, generator=g) * scale[torch.randperm(M, generator=g)]
        w = torch.randn(D, 27, generator=g) * 0.2
        bias = torch.randn(D, generator=g) * 0.1
    else:
        xf = torch.randint(-4, 5, (M, D), generator=g).float()
        dyf = torch.randint(-4, 5, (M, D), generator=g).float()
        w = torch.randint(-4, 5, (D, 27), generator=g).float() * 0.5
        bias = torch.randint(-4, 5, (D,), generator=g).float() * 0.5
        scale = torch.ones(M, 1)
    o = types.SimpleNamespace(case=c, kind=kind, xf=xf, xb=xf.bfloat16(), dyf=dyf, dyb=dyf.bfloat16(), w=w, bias=bias,
                              scale=scale.reshape(-1))
    for k in ('xf', 'xb', 'dyf', 'dyb', 'w', 'bias', 'scale'):
        setattr(o, k, getattr(o, k).to(device))
    return o


@functools.lru_cache(maxsize=None)
def references(name, kind, mode, device='cpu'):
    """(bf16-tap reference, f32-tap reference) of a case's operands; computed once, shared, never modified"""
    o = operands(name, kind, device)
    g = o.case.geom
    r16 = reference(o.xb, o.w, o.bias, o.dyb, g, mode, res=o.xf, dres=o.dyf)
    r32 = reference(o.xf, o.w, o.bias, o.dyf, g, mode)
    return r16, r32


# ------------------------------------------------------------------ the f32 restatement (CPU) and its planted faults
FAULTS_LOCAL = ('corner_tap', 'halo_wrap', 'prev_batch')      # one voxel, one tap: the magnitude follows the input there
FAULTS_GLOBAL = ('noncausal_tap', 'mode_map', 'last_channel')
FAULTS = FAULTS_LOCAL + FAULTS_GLOBAL


def fault_sites(fault, geom):
    """the view voxels (b, t, h, w) at which a local fault can be planted"""
    B, T, H, W = geom
    if fault == 'corner_tap':     # tap (kt 2, kh 2, kw 2) = offset (0, +1, +1), dropped at a corner h = w = 0
        return [(b, t, 0, 0) for b in range(B) for t in (0, T - 1)]
    if fault == 'halo_wrap':      # tap (2, 1, 0) = offset (0, 0, -1) at w = 0 reads (h - 1, W - 1) instead of zero
        return [(b, t, h, 0) for b in range(B) for t in range(T) for h in range(1, H)]
    if fault == 'prev_batch':     # tap (1, 1, 1) = offset (-1, 0, 0) at t = 0 reads batch b - 1's plane T - 1
        return [(b, 0, h, w) for b in range(1, B) for h in range(H) for w in range(W)]
    raise KeyError(fault)


def fault_source(fault, site):
    """(view voxel whose value the fault adds or drops, tap index)"""
    b, t, h, w = site
    if fault == 'corner_tap':
        return (b, t, h + 1, w + 1), 26
    if fault == 'halo_wrap':
        return (b, t, h - 1, -1), 21
    return (b - 1, -1, h, w), 13


def model_f32(x, w, bias, geom, mode, res=None, fault=None, site=None):
    """out = res + bias + conv(x) in plain f32 torch (27 shifted multiply-adds in tap order), written through a
    sentinel-filled [M, D] buffer as a kernel would.  fault: one of FAULTS, local ones at view voxel `site`."""
    B, T, H, W = geom
    M, D = x.shape
    rows = view_rows(geom, 0 if fault == 'mode_map' else mode).reshape(-1)
    x, w, bias = x.float(), w.float().reshape(D, 27), bias.float()
    xv = x[rows].view(B, T, H, W, D)
    rv = xv if res is None else res.float()[rows].view(B, T, H, W, D)
    xp = _pad(xv, 2, 0)
    acc = bias.expand(B, T, H, W, D).clone()
    for kt in range(3):
        for kh in range(3):
            for kw in range(3):
                k = (kt * 3 + kh) * 3 + kw
                if fault == 'noncausal_tap' and k == 4:      # tap (0, 1, 1) reads t - 1 instead of t - 2
                    xn = xp[:, 1:1 + T, kh:kh + H, kw:kw + W]
                else:
                    xn = xp[:, kt:kt + T, kh:kh + H, kw:kw + W]
                term = w[:, k] * xn
                if fault in FAULTS_LOCAL and k == fault_source(fault, site)[1]:
                    term = term.clone()
                    src = fault_source(fault, site)[0]
                    val = w[:, k] * xv[src]
                    term[site] = 0 if fault == 'corner_tap' else val
                acc = acc + term
    acc = acc + rv
    out = torch.full((M, D), SENT32, dtype=torch.int32).view(F32)
    out[rows] = acc.reshape(M, D)
    if fault == 'last_channel':
        _ints(out)[:, D - 1] = SENT32
    return out


def grads_f32(dout, x, w, geom, mode, dres=None):
    """(dx, dweight, dbias) in plain f32 torch, the weight gradient as one sum per tap"""
    B, T, H, W = geom
    M, D = x.shape
    rows = view_rows(geom, mode).reshape(-1)
    w = w.float().reshape(D, 27)
    xv, dv = x.float()[rows].view(B, T, H, W, D), dout.float()[rows].view(B, T, H, W, D)
    drv = dv if dres is None else dres.float()[rows].view(B, T, H, W, D)
    xp, dp = _pad(xv, 2, 0), _pad(dv, 0, 2)
    acc = torch.zeros_like(dv)
    dw = torch.zeros(D, 27)
    for kt in range(3):
        for kh in range(3):
            for kw in range(3):
                k = (kt * 3 + kh) * 3 + kw
                acc = acc + w[:, k] * dp[:, 2 - kt:2 - kt + T, 2 - kh:2 - kh + H, 2 - kw:2 - kw + W]
                dw[:, k] = (dv * xp[:, kt:kt + T, kh:kh + H, kw:kw + W]).sum((0, 1, 2, 3))
    dx = torch.empty(M, D)
    dx[rows] = (acc + drv).reshape(M, D)
    return dx, dw, dv.sum((0, 1, 2, 3))


# ------------------------------------------------------------------ the C entry points under guards (GPU)
def _L():
    from ctclip_mi355x import _lib
    return _lib


def _g(t):
    return Guard(t.shape, t.dtype, t.device, data=t)


def guarded_inputs(o):
    """every operand of a case as a NaN-padded Guard (built once per case; the launches never write them)"""
    return types.SimpleNamespace(xf=_g(o.xf), xb=_g(o.xb), dyf=_g(o.dyf), dyb=_g(o.dyb), w=_g(o.w), bias=_g(o.bias))


def launch_fwd(gi, geom, D, mode, stats=False):
    """ctclip_peg_fwd / ctclip_peg_fwd_stats (argument order of _lib.py).  Returns {name: Guard}."""
    L = _L()
    M, dev = ntok(geom), gi.xf.buf.device
    outs = {'out': Guard((M, D), F32, dev), 'out_bf16': Guard((M, D), BF16, dev)}
    a = [L.ptr(gi.xb.view), L.ptr(gi.xf.view), *geom, D, L.ptr(gi.w.view), L.ptr(gi.bias.view), mode,
         L.ptr(outs['out'].view), L.ptr(outs['out_bf16'].view)]
    if stats:
        outs['stats'] = Guard((D // 64, M, 2), F32, dev)
        L.call('ctclip_peg_fwd_stats', *a, L.ptr(outs['stats'].view), L.stream_ptr())
    else:
        L.call('ctclip_peg_fwd', *a, L.stream_ptr())
    return outs


def launch_fwd_x32(gi, geom, D, mode, stats=False):
    """ctclip_peg_fwd_x32s with the bf16 and fp16 copies and the status word (must stay 0: values in fp16 range)"""
    L = _L()
    M, dev = ntok(geom), gi.xf.buf.device
    outs = {'out': Guard((M, D), F32, dev), 'out_bf16': Guard((M, D), BF16, dev), 'out_f16': Guard((M, D), F16, dev)}
    if stats:
        outs['stats'] = Guard((D // 32, M, 2), F32, dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    L.call('ctclip_peg_fwd_x32s', L.ptr(gi.xf.view), *geom, D, L.ptr(gi.w.view), L.ptr(gi.bias.view), mode,
           L.ptr(outs['out'].view), L.ptr(outs['out_bf16'].view), L.ptr(outs['out_f16'].view), None,
           L.ptr(outs['stats'].view) if stats else None, L.ptr(status), L.stream_ptr())
    assert int(status.item()) == 0, 'fp16 range flag raised'
    return outs


def merge_stats(stats, D, group):
    """ctclip_ln_stats_merge on a guarded partial buffer -> guarded (mean, rstd)"""
    L = _L()
    ng, M, _ = stats.shape
    dev = stats.buf.device
    outs = {'mean': Guard((M,), F32, dev), 'rstd': Guard((M,), F32, dev)}
    L.call('ctclip_ln_stats_merge', L.ptr(stats.view), ng, M, D, EPS, L.ptr(outs['mean'].view),
           L.ptr(outs['rstd'].view), L.stream_ptr())
    return outs


def launch_bwd_data(gi, geom, D, mode):
    L = _L()
    M, dev = ntok(geom), gi.xf.buf.device
    outs = {'dx': Guard((M, D), F32, dev), 'dx_bf16': Guard((M, D), BF16, dev)}
    L.call('ctclip_peg_bwd_data', L.ptr(gi.dyb.view), L.ptr(gi.dyf.view), *geom, D, L.ptr(gi.w.view), mode,
           L.ptr(outs['dx'].view), L.ptr(outs['dx_bf16'].view), L.stream_ptr())
    return outs


def launch_bwd_data_x32(gi, geom, D, mode):
    L = _L()
    M, dev = ntok(geom), gi.xf.buf.device
    outs = {'dx': Guard((M, D), F32, dev), 'dx_bf16': Guard((M, D), BF16, dev)}
    L.call('ctclip_peg_bwd_data_x32', L.ptr(gi.dyf.view), *geom, D, L.ptr(gi.w.view), mode, L.ptr(outs['dx'].view),
           L.ptr(outs['dx_bf16'].view), L.stream_ptr())
    return outs


def launch_bwd_weight(gi, geom, D, mode, nblk):
    """ctclip_peg_bwd_weight -> the guarded partial slabs [nblk, D, 28]"""
    L = _L()
    part = Guard((nblk, D, 28), F32, gi.xf.buf.device)
    L.call('ctclip_peg_bwd_weight', L.ptr(gi.dyb.view), L.ptr(gi.xb.view), *geom, D, mode, L.ptr(part.view), nblk,
           L.stream_ptr())
    return part


def launch_reduce(part, D, dw_sink=None, db_sink=None, want_dw=True, want_db=True, accumulate=0):
    """ctclip_peg_wgrad_reduce into guarded sinks (fresh sentinel ones, or starting from dw_sink / db_sink values);
    want_dw / want_db False passes that pointer as null and returns its guard untouched for inspection"""
    L = _L()
    dev = part.buf.device
    outs = {'dweight': Guard((D, 27), F32, dev, live=dw_sink), 'dbias': Guard((D,), F32, dev, live=db_sink)}
    L.call('ctclip_peg_wgrad_reduce', L.ptr(part.view), part.shape[0], D, L.ptr(outs['dweight'].view) if want_dw else None,
           L.ptr(outs['dbias'].view) if want_db else None, accumulate, L.stream_ptr())
    return outs
