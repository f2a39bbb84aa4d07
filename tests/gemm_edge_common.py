"""GEMM epilogues at ragged edges: guard-banded buffers, float64 references and per-element
bounds shared by tests/test_gemm_edge_cpu.py (checks the checks, no GPU) and tests/test_gpu_gemm_edges.py.

Every operand is a view into a NaN-padded buffer (PAD_R spare rows, PAD_C spare columns) and every output a
view into a sentinel-filled one with the same margins, so a read past an operand shows as a non-finite
result and a store past an output as a changed margin.  Bounds are derived in DESIGN §32; none is fitted
to a GPU result."""
import math
import types

import torch

BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
PAD_R, PAD_C = 32, 64
SENT32, SENT16 = 0x7FC0BEEF, 0x7FC5      # NaN bit patterns (f32; bf16 and fp16 alike)
U23, U24 = 2.0 ** -23, 2.0 ** -24        # accumulator unit (holds for truncating adds, an assumption); f32 half-ulp
SLACK = 1.0 + 2.0 ** -10                 # second-order terms of a chain of f32 roundings
R16 = {BF16: (2.0 ** -9, 0.0), F16: (2.0 ** -12, 2.0 ** -25)}   # half-ulp (relative, subnormal) of a 16-bit store
GELU_SLOPE = 1.13                        # sup |gelu'| = 1.12891
L2N_REL = 2.0 ** -19                     # f32 chain of the head l2norm: 32 squares summed, sqrt, rcp, two products < 32 u

# The device's GELU (common.h erf_fast: Abramowitz & Stegun 7.1.26 on v_rcp / v_exp) restated in f32 on the
# host (gelu_dev_f32 below), maximum absolute error against float64 erf-GELU and its derivative over every
# bf16 value in [-16, 16], measured by test_gemm_edge_cpu.py::test_gelu_allowance (which recomputes them);
# the allowance is twice that: the device's exp / rcp may differ from the host's by an ulp.
GELU_ERR_MEASURED = 4.45e-7       # measured 4.4449e-07 (at |x| near 16, where 0.5 x (1 + erf) rounds in f32)
DGELU_ERR_MEASURED = 2.68e-7      # measured 2.6760e-07
GELU_ALLOW = 2 * GELU_ERR_MEASURED
DGELU_ALLOW = 2 * DGELU_ERR_MEASURED
GELU_RANGE = 16.0

OLD_NORM_F32, OLD_NORM_16 = 1e-5, 1e-2   # the whole-matrix relative Frobenius thresholds of the older GEMM tests


# ------------------------------------------------------------------ GELU: the kernel's formula and float64
def gelu_dev_f32(x):
    """(gelu, gelu') as common.h gelu_erf_and_grad computes them, in f32 (no fused multiply-adds here)."""
    x = x.float()
    f = lambda v: torch.tensor(v, dtype=F32, device=x.device)  # noqa: E731
    a = (x * f(0.70710678118654752)).abs()
    t = 1.0 / (a * f(0.3275911) + f(1.0))
    y = t * f(1.061405429) + f(-1.453152027)
    y = y * t + f(1.421413741)
    y = y * t + f(-0.284496736)
    y = y * t + f(0.254829592)
    y = y * t
    e = torch.exp(-a * a)
    erf = torch.copysign(f(1.0) - y * e, x)
    half = f(0.5) * (f(1.0) + erf)
    return f(0.5) * x * (f(1.0) + erf), x * (f(0.39894228040143268) * e) + half


def gelu64(x):
    x = x.double()
    cdf = 0.5 * (1 + torch.erf(x / math.sqrt(2)))
    pdf = torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
    return x * cdf, cdf + x * pdf


def measure_gelu_error():
    """max |gelu_dev_f32 - float64| over every bf16 value in [-16, 16]: (gelu, derivative)"""
    x = torch.arange(-32768, 32768, dtype=torch.int32).to(torch.int16).view(BF16)
    x = x[torch.isfinite(x.float()) & (x.float().abs() <= GELU_RANGE)]
    g, dg = gelu_dev_f32(x)
    g64, dg64 = gelu64(x)
    return (g.double() - g64).abs().max().item(), (dg.double() - dg64).abs().max().item()


# ------------------------------------------------------------------ buffers
def _ints(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def pad_in(x):
    """x copied into a buffer with PAD_R spare rows and PAD_C spare columns of NaN (1-D: PAD_C spare
    elements); the returned view has the buffer's row stride."""
    if x.dim() == 1:
        buf = torch.full((x.numel() + PAD_C,), float('nan'), dtype=x.dtype, device=x.device)
        buf[:x.numel()] = x
        return buf[:x.numel()]
    r, c = x.shape
    buf = torch.full((r + PAD_R, c + PAD_C), float('nan'), dtype=x.dtype, device=x.device)
    buf[:r, :c] = x
    return buf[:r, :c]


class Out:
    """One guarded output: `buf` [rows + PAD_R, cols + PAD_C] (slabs: [lead + 1, rows, cols + PAD_C], the
    kernels' slab stride being rows * ldc) filled with the sentinel, the live region optionally with data."""

    def __init__(self, rows, cols, dtype, device, live=None, lead=0):
        self.rows, self.cols, self.lead = rows, cols, lead
        shape = (lead + 1, rows, cols + PAD_C) if lead else (rows + PAD_R, cols + PAD_C)
        ints = torch.full(shape, SENT32 if dtype == F32 else SENT16, device=device,
                          dtype=torch.int32 if dtype == F32 else torch.int16)
        self.buf = ints.view(dtype)
        if live is not None:
            self.view.copy_(live)

    @property
    def view(self):
        return self.buf[:self.lead, :, :self.cols] if self.lead else self.buf[:self.rows, :self.cols]

    def like(self, buf):
        o = Out.__new__(Out)
        o.rows, o.cols, o.lead, o.buf = self.rows, self.cols, self.lead, buf
        return o

    def margin_intact(self, before):
        a, b = _ints(self.buf).clone(), _ints(before).clone()
        for t in (a, b):
            if self.lead:
                t[:self.lead, :, :self.cols] = 0
            else:
                t[:self.rows, :self.cols] = 0
        return torch.equal(a, b)


def pack(outs):
    """every whole buffer of a dict of Outs as one byte tensor (what a variant run hands back)"""
    return torch.cat([outs[k].buf.reshape(-1).view(torch.uint8) for k in sorted(outs)])


def unpack(packed, outs):
    res, off = {}, 0
    for k in sorted(outs):
        n = outs[k].buf.numel() * outs[k].buf.element_size()
        res[k] = outs[k].like(packed[off:off + n].view(outs[k].buf.dtype).view(outs[k].buf.shape))
        off += n
    return res


# ------------------------------------------------------------------ cases
KINDS_NEED_N64 = ('geglu', 'argmax', 'argmax_f16', 'l2n')


def slab_ranges(K, split, kstep, family):
    """the K range of each slab: gemm256.hip make_plan (whole steps shared out) / gemm.hip ctclip_gemm
    (ceil(K / split) rounded up to the 64-deep step)"""
    if family == 256:
        kper = (K // kstep + split - 1) // split * kstep
    else:
        kper = ((K + split - 1) // split + 63) // 64 * 64
    return [(min(K, z * kper), min(K, (z + 1) * kper)) for z in range(split)]


_OPERANDS = {}


def operands(M, N, K, dt, device, tie=False, hilo=False):
    """A [M, K], B [N, K] (live values, shared by every case of the shape) with their float64 product P,
    |A| |B| and the accumulator bound E = K 2^-23 (|A| |B|)."""
    key = (M, N, K, dt, str(device), tie, hilo)
    if key not in _OPERANDS:
        g = torch.Generator().manual_seed(7919 * M + 31 * N + K)
        A = torch.randn(M, K, generator=g).to(dt).to(device)
        B = (torch.randn(N, K, generator=g) * 0.05).to(dt).to(device)
        B2 = (torch.randn(N, K, generator=g) * 0.05 * 2.0 ** -8).to(dt).to(device) if hilo else None
        if tie:      # exact ties: a later column of the first and of the last 64-column group repeats an earlier one
            for g0 in (0, (N - 1) // 64 * 64):
                hi = min(g0 + 40, N - 1)
                B[hi] = B[g0 + 5]
        Bs = B.double() + (B2.double() if hilo else 0)
        Ba = B.double().abs() + (B2.double().abs() if hilo else 0)
        P = A.double() @ Bs.t()
        Pabs = A.double().abs() @ Ba.t()
        _OPERANDS[key] = types.SimpleNamespace(A=A, B=B, B2=B2, P=P, Pabs=Pabs, E=(2 * K if hilo else K) * U23 * Pabs)
    return _OPERANDS[key]


def make_case(kind, M, N, K, ak, bk, device, family, split=None, seed=0):
    """Everything one launch needs: padded operand views in the asked layout, the epilogue's padded inputs,
    the keyword arguments of kernels._gemm_raw and a factory of fresh guarded outputs."""
    dt = F16 if kind == 'argmax_f16' else BF16
    tie = kind in ('argmax', 'argmax_f16')
    op = operands(M, N, K, dt, device, tie=tie, hilo=kind == 'hilo')
    c = types.SimpleNamespace(kind=kind, M=M, N=N, K=K, ak=ak, bk=bk, family=family, op=op, device=device, split=1)
    lay = lambda X, kc: pad_in(X if kc else X.t().contiguous())  # noqa: E731
    c.Am, c.Bm = lay(op.A, ak), lay(op.B, bk)
    c.B2m = lay(op.B2, bk) if kind == 'hilo' else None
    g = torch.Generator().manual_seed(1 + seed + 13 * M + N)
    rnd = lambda *s, scale=1.0: (torch.randn(*s, generator=g) * scale).to(device)  # noqa: E731
    kw = {}
    if kind in ('res', 'res_shadow', 'bf16', 'gelu', 'hilo', 'split3'):
        c.bias = pad_in(rnd(N, scale=0.02))
        kw['bias'] = c.bias
    if kind in ('res', 'res_shadow', 'split3'):
        c.R = pad_in(rnd(M, N))
        kw.update(R=c.R, ldr=c.R.stride(0))
    if kind == 'acc':
        c.C0 = rnd(M, N)
        kw['accumulate'] = True
    if kind in ('slabs', 'split3'):
        c.split = split or (2 if kind == 'slabs' else 3)
        c.ranges = slab_ranges(K, c.split, 64, family)
        kw['split_k'] = c.split
    if kind == 'gelu':
        kw['act'] = 1
    if kind == 'geglu':
        kw['act'] = 2
    if tie:
        kw['act'] = 3
    if kind == 'l2n':
        c.n2 = max(64, (N // 2 + 32) // 64 * 64)
        c.scale = pad_in(torch.rand(32, generator=g).to(device) + 0.5)
        kw.update(act=5, bias=c.scale, n2=c.n2)
    if kind in ('geglu_bwd', 'geglu_bwd_h16'):
        hd = F16 if kind == 'geglu_bwd_h16' else BF16
        c.h = pad_in(rnd(M, 2 * N).to(hd))
        kw.update(act=4, R=c.h, ldr=c.h.stride(0))
    if kind == 'gelu_bwd':
        c.pre = pad_in(rnd(M, N).bfloat16())
        kw.update(act=6, R=c.pre, ldr=c.pre.stride(0))
    if kind == 'hilo':
        kw['B2'] = c.B2m
    if kind == 'split3':
        kw = {'split_k': c.split}      # the GEMM writes slabs; bias / R / GELU belong to the combine
    c.kw = kw
    return c


def new_outs(c):
    M, N, d = c.M, c.N, c.device
    o = lambda rows, cols, dtype, **k: Out(rows, cols, dtype, d, **k)  # noqa: E731
    kind = c.kind
    if kind in ('rows', 'res', 'hilo'):
        return {'C': o(M, N, F32)}
    if kind == 'res_shadow':
        return {'C': o(M, N, F32), 'C2': o(M, N, BF16)}
    if kind == 'acc':
        return {'C': o(M, N, F32, live=c.C0)}
    if kind == 'slabs':
        return {'C': o(M, N, F32, lead=c.split), 'Cr': o(M, N, F32)}
    if kind == 'split3':
        return {'C': o(M, N, F32, lead=c.split), 'Cr': o(M, N, F32), 'C2': o(M, N, BF16)}
    if kind in ('bf16', 'gelu_bwd'):
        return {'C': o(M, N, BF16)}
    if kind == 'gelu':
        return {'C': o(M, N, BF16), 'C2': o(M, N, BF16)}
    if kind == 'geglu':
        return {'C': o(M, N, BF16), 'C2': o(M, N // 2, BF16)}
    if kind in ('argmax', 'argmax_f16'):
        ng = (N + 63) // 64
        return {'C': o(M, 2 * ng, F32), 'C2': o(M, ng, F32)}     # (value, index) pairs; the second-best score
    if kind == 'l2n':
        return {'C': o(M, N, BF16), 'C2': o(M, c.n2, BF16)}
    if kind in ('geglu_bwd', 'geglu_bwd_h16'):
        return {'C': o(M, 2 * N, BF16)}
    raise KeyError(kind)


def launch(Kmod, c, outs):
    """the case through kernels._gemm_raw (and, for the slab kinds, the reduction / the fused combine)"""
    C = outs['C']
    kw = dict(c.kw)
    argmax = c.kind in ('argmax', 'argmax_f16')
    ldc = C.buf.stride(-2) // (2 if argmax else 1)
    if 'C2' in outs and c.kind != 'split3':
        kw.update(C2=outs['C2'].view, ldc2=outs['C2'].buf.stride(0))
    Kmod._gemm_raw(c.M, c.N, c.K, c.Am, c.Am.stride(0), c.ak, c.Bm, c.Bm.stride(0), c.bk, C.view, ldc, **kw)
    if c.kind == 'slabs':
        from ctclip_mi355x._lib import call, ptr, stream_ptr
        call('ctclip_reduce_slabs', ptr(C.view), c.split, c.M, c.N, ldc, ptr(outs['Cr'].view), outs['Cr'].buf.stride(0),
             1, 0, stream_ptr())
    if c.kind == 'split3':
        from ctclip_mi355x import _lib
        a = Kmod._gemm_args(c.M, c.N, c.K, None, None, outs['Cr'].view, act=1, bias=c.bias, R=c.R, C2=outs['C2'].view)
        _lib.call('ctclip_reduce_slabs_ep', _lib.ptr(C.view), c.split, c.M, c.N, ldc, _lib.ctypes.byref(a),
                  _lib.stream_ptr())


# ------------------------------------------------------------------ float64 references and bounds
def _r16(ref, e, dtype=BF16):
    """e plus half an ulp of the 16-bit store of a value within e of ref: 2^-9 (bf16; fp16 2^-12) of the power
    of two that closes the binade of |ref| + e.  (2^-9 |ref| itself is below round-to-nearest's own error for
    every value in the lower half of a binade: test_gemm_edge_cpu.py::test_half_ulp_is_of_the_binade.)"""
    rel, sub = R16[dtype]
    x = ref.abs() + e
    top = torch.where(x > 0, torch.ldexp(torch.ones_like(x), torch.frexp(x).exponent), torch.zeros_like(x))
    return e + rel * top + sub


def expected(c, outs):
    """[(name, output (float64), reference, bound)] for every element-wise checked output, and
    [(name, a, b)] pairs that must agree bit for bit.  References that the kernel defines on a stored
    16-bit output (GEGLU's g on h, the l2norm on q) read that output's bits."""
    op, M, N = c.op, c.M, c.N
    P, E, aP = op.P, op.E, op.P.abs()
    v = {k: o.view for k, o in outs.items()}
    chk, bits = [], []
    kind = c.kind
    d64 = lambda t: t.double()  # noqa: E731
    xa = getattr(c, 'extra_adds', 0)     # slab sums of the wrapper's automatic split-K (kernels._auto_split)
    if kind == 'rows':
        chk.append(('C', d64(v['C']), P, E))
    elif kind in ('res', 'res_shadow', 'hilo'):
        b, R = d64(c.bias), d64(c.R) if kind != 'hilo' else torch.zeros_like(P)
        e = E + ((1 if kind == 'hilo' else 2) + xa) * U24 * SLACK * (aP + E + b.abs() + R.abs())
        chk.append(('C', d64(v['C']), P + b + R, e))
        if kind == 'res_shadow':
            bits.append(('C2 = bf16(C)', v['C2'], v['C'].bfloat16()))
    elif kind == 'acc':
        C0 = d64(c.C0)
        chk.append(('C', d64(v['C']), C0 + P, E + U24 * SLACK * (aP + E + C0.abs())))
    elif kind in ('slabs', 'split3'):
        A64, B64 = d64(op.A), d64(op.B)
        sumE, sumabs = torch.zeros_like(P), torch.zeros_like(P)
        for z, (k0, k1) in enumerate(c.ranges):
            Pz = A64[:, k0:k1] @ B64[:, k0:k1].t()
            Ez = (k1 - k0) * U23 * (A64[:, k0:k1].abs() @ B64[:, k0:k1].abs().t())
            chk.append((f'slab {z}', d64(v['C'][z]), Pz, Ez))
            sumE += Ez
            sumabs += Pz.abs()
        if kind == 'slabs':
            chk.append(('sum', d64(v['Cr']), P, sumE + (c.split - 1) * U24 * SLACK * (sumabs + sumE)))
        else:
            b, R = d64(c.bias), d64(c.R)
            pre = P + b + R
            e = sumE + (c.split + 1) * U24 * SLACK * (sumabs + sumE + b.abs() + R.abs())
            assert pre.abs().max() + e.max() <= GELU_RANGE
            chk.append(('pre (C2)', d64(v['C2']), pre, _r16(pre, e)))
            chk.append(('gelu (C)', d64(v['Cr']), gelu64(pre)[0], GELU_SLOPE * e + GELU_ALLOW))
    elif kind in ('bf16', 'gelu'):
        b = d64(c.bias)
        pre = P + b
        e = E + (1 + xa) * U24 * SLACK * (aP + E + b.abs())
        if kind == 'bf16':
            chk.append(('C', d64(v['C']), pre, _r16(pre, e)))
        else:
            assert pre.abs().max() + e.max() <= GELU_RANGE
            ref = gelu64(pre)[0]
            chk.append(('pre (C2)', d64(v['C2']), pre, _r16(pre, e)))
            chk.append(('gelu (C)', d64(v['C']), ref, _r16(ref, GELU_SLOPE * e + GELU_ALLOW)))
    elif kind == 'geglu':
        chk.append(('h (C)', d64(v['C']), P, _r16(P, E)))
        hv = d64(v['C']).view(M, N // 64, 2, 32)          # g is defined on the stored, bf16-rounded h
        x, gt = hv[:, :, 0], hv[:, :, 1]
        ref = (gelu64(gt)[0] * x).reshape(M, N // 2)
        e = (GELU_ALLOW * x.abs()).reshape(M, N // 2) + U24 * SLACK * ref.abs()
        chk.append(('g (C2)', d64(v['C2']), ref, _r16(ref, e)))
    elif kind == 'l2n':
        chk.append(('q (C)', d64(v['C']), P, _r16(P, E)))
        qv = d64(v['C'][:, :c.n2]).view(M, c.n2 // 32, 32)   # qn is defined on the stored, bf16-rounded q
        nrm = qv.square().sum(-1, keepdim=True).sqrt().clamp_min(1e-12)
        ref = (qv / nrm * d64(c.scale)).reshape(M, c.n2)
        chk.append(('qn (C2)', d64(v['C2']), ref, _r16(ref, L2N_REL * ref.abs())))
    elif kind in ('geglu_bwd', 'geglu_bwd_h16'):
        # dg = bf16(acc) is never stored: the reference keeps P and the bound carries that rounding
        G = N
        ed = _r16(P, E).view(M, G // 32, 32)
        d, ad = P.view(M, G // 32, 32), (aP + _r16(P, E)).view(M, G // 32, 32)
        hv = d64(c.h).view(M, G // 32, 2, 32)
        h0, h1 = hv[:, :, 0], hv[:, :, 1]
        if kind == 'geglu_bwd_h16':     # [gelu(gate) | x gelu'(gate)]: two products
            ox, og = d * h0, d * h1
            ex, eg = ed * h0.abs() + U24 * SLACK * ox.abs(), ed * h1.abs() + U24 * SLACK * og.abs()
        else:                           # [x | gate]
            assert h1.abs().max() <= GELU_RANGE
            ge, dge = gelu64(h1)
            ox, og = d * ge, d * h0 * dge
            ex = ed * ge.abs() + ad * GELU_ALLOW + U24 * SLACK * ox.abs()
            eg = ed * (h0 * dge).abs() + ad * h0.abs() * DGELU_ALLOW + 2 * U24 * SLACK * og.abs()
        ref = torch.stack([ox, og], 2).reshape(M, 2 * G)
        e = torch.stack([ex, eg], 2).reshape(M, 2 * G)
        chk.append(('dh (C)', d64(v['C']), ref, _r16(ref, e)))
    elif kind == 'gelu_bwd':
        pre = d64(c.pre)
        assert pre.abs().max() <= GELU_RANGE
        dge = gelu64(pre)[1]
        ref = P * dge
        e = E * dge.abs() + (aP + E) * DGELU_ALLOW + U24 * SLACK * ref.abs()
        chk.append(('C', d64(v['C']), ref, _r16(ref, e)))
    else:
        raise KeyError(kind)
    return chk, bits


def check_argmax(c, C, C2, P=None, E=None):
    """act 3: C [M, 2 ng] (value, index) pairs, C2 [M, ng] the group's second-best score.  Returns the ratios
    {name: max err / bound} and the list of broken structural rules."""
    M, N = c.M, c.N
    P = c.op.P if P is None else P
    E = c.op.E if E is None else E
    ng = (N + 63) // 64
    fill = lambda T, val: torch.cat([T, T.new_full((M, ng * 64 - N), val)], 1).view(M, ng, 64)  # noqa: E731
    Pg, Eg = fill(P, float('-inf')), fill(E, 0.0).amax(-1)
    top2 = Pg.topk(2, -1).values
    val = C[:, 0::2].double()
    idx = C[:, 1::2].contiguous().view(torch.int32).long()
    col0 = torch.arange(ng, device=C.device) * 64
    bad = []
    inside = (idx >= col0) & (idx < (col0 + 64).clamp_max(N))
    if not inside.all():
        bad.append('index outside its 64-column group or at / beyond N')
    chosen = Pg.gather(-1, (idx - col0).clamp(0, 63).unsqueeze(-1)).squeeze(-1)
    for g0 in (0, (N - 1) // 64 * 64):      # the exact ties of operands(tie=True): the first maximum wins
        if (idx == min(g0 + 40, N - 1)).any():
            bad.append(f'tie: column {min(g0 + 40, N - 1)} returned, column {g0 + 5} holds the same score')
    ratios = {'value': ratio(val, top2[..., 0], Eg), 'chosen column': ratio(chosen, top2[..., 0], 2 * Eg)}
    sec, sref = C2.double(), top2[..., 1]
    lone = torch.isinf(sref)                 # a group of one column has no second-best: -inf
    if not torch.equal(sec[lone], sref[lone]):
        bad.append('second-best of a one-column group is not -inf')
    ratios['second'] = ratio(torch.where(lone, 0.0, sec), torch.where(lone, 0.0, sref), Eg)
    return ratios, bad


def ratio(out, ref, bound):
    """max over ALL elements of |out - ref| / bound; inf where either is not finite or a zero bound is missed"""
    err = (out - ref).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound)
    r = torch.where(torch.isfinite(r), r, torch.full_like(r, float('inf')))
    return r.max().item()


def old_norm(out, ref):
    """the older tests' figure: relative Frobenius error over the whole matrix"""
    return ((out.double() - ref).norm() / ref.norm().clamp_min(1e-30)).item()


def verify(c, outs, before, label=''):
    """Every check of one run: {'guard': [names of outputs whose margin changed], 'ratios': {name: max
    err / bound}, 'bits': [...], 'rules': [...]}; ok() tells whether all hold."""
    rep = types.SimpleNamespace(guard=[k for k in sorted(outs) if not outs[k].margin_intact(before[k])],
                                ratios={}, bits=[], rules=[])
    if c.kind in ('argmax', 'argmax_f16'):
        rep.ratios, rep.rules = check_argmax(c, outs['C'].view, outs['C2'].view)
    else:
        chk, bits = expected(c, outs)
        rep.ratios = {name: ratio(out, ref, bound) for name, out, ref, bound in chk}
        rep.bits = [name for name, a, b in bits if not torch.equal(_ints(a.contiguous()), _ints(b.contiguous()))]
    rep.ok = lambda: not rep.guard and not rep.bits and not rep.rules and all(r <= 1.0 for r in rep.ratios.values())
    rep.failed = ([f'guard({k})' for k in rep.guard] + [f'bound({k}: {r:.3g})' for k, r in rep.ratios.items() if not r <= 1.0]
                  + [f'bits({k})' for k in rep.bits] + [f'rule({k})' for k in rep.rules])
    if label:
        print(f'{label}: ' + ', '.join(f'{k} {r:.3f}' for k, r in rep.ratios.items())
              + ('' if rep.ok() else '  FAILED ' + '; '.join(rep.failed)))
    return rep


# ------------------------------------------------------------------ the f32 restatement (CPU)
def restate(c, outs, acc=None, bias=None):
    """The GEMM with its epilogue in plain torch f32 on the rounded operands, written through the guarded
    views as a kernel would (test_gemm_edge_cpu.py seeds its faults into this).  acc / bias: substitutes for
    the f32 product and the bias vector (faults)."""
    op, M, N, kind = c.op, c.M, c.N, c.kind
    v = {k: o.view for k, o in outs.items()}
    Bf = op.B.float() + (op.B2.float() if kind == 'hilo' else 0)
    if kind == 'hilo':
        acc = op.A.float() @ op.B.float().t() + op.A.float() @ op.B2.float().t()
    elif acc is None:
        acc = op.A.float() @ Bf.t()
    b = bias if bias is not None else getattr(c, 'bias', None)
    rb = lambda t: t.bfloat16().float()  # noqa: E731
    if kind == 'rows':
        v['C'].copy_(acc)
    elif kind in ('res', 'res_shadow'):
        v['C'].copy_(acc + b + c.R)
        if kind == 'res_shadow':
            v['C2'].copy_(v['C'].bfloat16())
    elif kind == 'hilo':
        v['C'].copy_(acc + b)
    elif kind == 'acc':
        v['C'].copy_(v['C'] + acc)
    elif kind in ('slabs', 'split3'):
        A, s = op.A.float(), torch.zeros(M, N)
        for z, (k0, k1) in enumerate(c.ranges):
            v['C'][z].copy_(A[:, k0:k1] @ Bf[:, k0:k1].t())
            s = s + v['C'][z]
        if kind == 'slabs':
            v['Cr'].copy_(s)
        else:
            pre = s + b + c.R
            v['C2'].copy_(pre.bfloat16())
            v['Cr'].copy_(gelu_dev_f32(pre)[0])
    elif kind == 'bf16':
        v['C'].copy_((acc + b).bfloat16())
    elif kind == 'gelu':
        v['C2'].copy_((acc + b).bfloat16())
        v['C'].copy_(gelu_dev_f32(acc + b)[0].bfloat16())
    elif kind == 'geglu':
        v['C'].copy_(acc.bfloat16())
        hv = rb(acc).view(M, N // 64, 2, 32)
        v['C2'].copy_((gelu_dev_f32(hv[:, :, 1])[0] * hv[:, :, 0]).reshape(M, N // 2).bfloat16())
    elif kind in ('argmax', 'argmax_f16'):
        ng = (N + 63) // 64
        g = torch.cat([acc, acc.new_full((M, ng * 64 - N), float('-inf'))], 1).view(M, ng, 64)
        best = g.max(-1)
        hit = g == best.values.unsqueeze(-1)
        first = torch.where(hit, torch.arange(64).expand_as(hit), torch.full_like(hit, 64, dtype=torch.long)).amin(-1)
        idx = (first + torch.arange(ng) * 64).to(torch.int32)
        v['C'][:, 0::2] = best.values
        v['C'][:, 1::2] = idx.view(F32)
        v['C2'].copy_(g.topk(2, -1).values[..., 1])
    elif kind == 'l2n':
        v['C'].copy_(acc.bfloat16())
        qv = rb(acc)[:, :c.n2].view(M, c.n2 // 32, 32)
        nrm = qv.square().sum(-1, keepdim=True).sqrt().clamp_min(1e-12)
        v['C2'].copy_(((qv * (1.0 / nrm)) * c.scale).reshape(M, c.n2).bfloat16())
    elif kind in ('geglu_bwd', 'geglu_bwd_h16'):
        d = rb(acc).view(M, N // 32, 32)
        hv = c.h.float().view(M, N // 32, 2, 32)
        if kind == 'geglu_bwd_h16':
            o = torch.stack([d * hv[:, :, 0], d * hv[:, :, 1]], 2)
        else:
            ge, dge = gelu_dev_f32(hv[:, :, 1])
            o = torch.stack([d * ge, d * hv[:, :, 0] * dge], 2)
        v['C'].copy_(o.reshape(M, 2 * N).bfloat16())
    elif kind == 'gelu_bwd':
        v['C'].copy_((acc * gelu_dev_f32(c.pre)[1]).bfloat16())
    else:
        raise KeyError(kind)
