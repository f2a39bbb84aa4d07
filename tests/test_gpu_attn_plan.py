"""Every kernel the attention launch plan (attn.hip make_plan) can reach by shape, against a float64
reference of the same operation built from the exact bf16 inputs: non-square CPB grids, the base
L = 576 layout and the layouts just outside it, bias with a key mask / without a bias gradient,
head dim 64 with bias, and the plain kernels with several (sequence, head) pairs per workgroup
(pp > 1, ragged last workgroup, dropout).  Also both bias-gradient paths (atomics / workspace) and
the memory around every output.

Metric (attn_common.attn_compare): per (sequence, head) block max|got - ref| / max|ref| for O, dQ,
dK, dV (dU: per head row; LSE: absolute, natural log), worst block, against the same figure of a
torch emulation of a bf16 pipeline on the same inputs: err <= max(3 E_emul, 2^-8), LSE
err <= min(max(3 E_emul, 2^-16), 2e-3); plus the suite's Frobenius bounds (8e-3 / 2e-2).

Measured on an MI355X, err / E_emul per output (x 1e-3; LSE absolute, natural log), and the kernels
each case launched (forward / dQ / dK,dV; rocprofv3 --kernel-trace):

case                               O         LSE        dQ        dK        dV        dU  kernels
base_16x36                   4.0/3.3   1.65/0.59   6.0/5.6   5.2/4.1   3.5/3.5   1.3/1.6  Run3Cinit/FramesDma/FramesDma
base_36x16                   4.0/3.6   1.50/0.69   4.9/4.9   3.9/3.4   4.9/4.1   1.4/1.1  Run3Cinit/FramesDma/FramesDma
base_8x72                    3.6/2.9   1.54/0.61   4.3/5.1   5.4/3.8   3.2/3.4   0.8/0.7  Run3Cinit/FramesDma/FramesDma
run_4x16                     3.2/3.1   1.82/0.98   6.5/5.6   4.7/4.5   5.0/4.0   2.3/1.2  Run3Cinit/FramesRun/Run
run_16x4                     3.0/3.0   1.63/1.33   6.9/6.9   5.5/5.5   3.7/3.5   1.9/1.7  Run3Cinit/FramesRun/Run
gen_5x7                      3.4/3.5   <.01/1.04   4.5/6.1   4.5/4.5   4.0/4.5   1.7/1.6  Bias32/Frames/Bias32
gen_7x5                      5.3/3.2   <.01/0.92   4.9/5.6   4.6/4.6   3.9/3.9   3.9/1.6  Bias32/Frames/Bias32
gen_3x4                      3.3/3.2   <.01/0.98   4.5/4.5   3.5/4.4   3.9/4.4   2.0/1.8  Bias32/Frames/Bias32
off_base_nseq1               3.5/2.7   0.86/0.54   3.8/3.6   2.7/2.7   2.8/2.8   0.6/0.5  Run3Cinit/FramesDma/Run
off_base_interleaved         3.4/2.5   1.03/0.53   3.8/3.9   5.4/5.4   4.8/4.8   0.8/1.6  Run3Cinit/FramesRun/Run
bias_no_dbias_6x6            3.0/3.4   <.01/0.96   3.2/3.1   4.8/4.8   4.1/4.1         -  Bias32/Bias32/Bias32
bias_no_dbias_8x8            3.6/3.4   1.18/0.85   3.7/3.7   3.3/3.3   3.7/3.7         -  Run3Cinit/Bias32/Run
bias_kmask_8x8               3.8/3.4   <.01/1.32   4.6/4.6   3.6/3.9   4.1/4.9   3.0/3.2  Bias32/Bias32/Bias32
bias_kmask_6x6               3.2/2.8   <.01/1.26   5.2/5.1   6.4/6.6   4.5/4.5   2.3/1.5  Bias32/Bias32/Bias32
bias_kmask_8x8_leftpad       4.0/3.3   <.01/1.21   5.6/4.6   3.6/4.1   3.3/3.3   2.7/3.1  Bias32/Bias32/Bias32
bias_kmask_6x6_leftpad       4.3/3.4   <.01/1.23   3.4/4.3   4.0/4.6   3.9/4.6   3.5/2.5  Bias32/Bias32/Bias32
bias_d64_6x6                 3.8/2.6   <.01/1.05   3.7/3.7   3.6/4.8   4.3/4.3   1.4/2.3  Bias64/Bias64/Bias64
bias_d64_8x8                 4.3/2.7   <.01/0.95   5.5/4.9   6.0/4.1   3.6/3.6   2.5/2.7  Bias64/Bias64/Bias64
plain32_l40                  4.7/4.7   <.01/0.63   4.1/4.1   3.9/3.9   4.3/3.9         -  Plain32 x 3
plain32_mask_l20             3.8/4.4   <.01/1.03   3.9/6.3   4.6/4.6   5.4/5.0         -  Plain32 x 3
plain32_l128_bert            4.6/5.3   <.01/1.18   3.7/4.0   3.8/4.0   5.2/5.2         -  Plain32 x 3
plain32_l128_bert_leftpad    5.2/4.0   <.01/1.25   3.4/4.2   3.5/3.5   5.6/5.3         -  Plain32 x 3
plain64_l24                  4.5/4.3   <.01/1.21   3.8/3.7   4.7/4.5   4.3/4.8         -  Plain64 x 3
plain64_l9                   3.6/3.5   <.01/0.99   4.9/3.7   3.8/3.8   3.5/4.0         -  Plain64 x 3
plain64_drop_l40             4.4/4.4   <.01/0.54   4.1/4.1   3.8/3.8   3.8/3.8         -  Plain64 x 3
small_h4_l24                 4.2/4.2   <.01/0.78   4.5/3.9   4.3/4.3   5.0/5.0         -  SmallCoop/Fused/SmallCoop
small_h3_l5                  3.4/3.7   <.01/1.09   4.8/4.5   4.3/5.3   4.1/4.1         -  Small/Fused/Small

dU by path (test_dbias_paths), err / E_emul x 1e-3, atomic = workspace to the digits shown:
  run_4x16         2.3/1.2
  gen_5x7_h4       2.5/2.1
  base_16x36_h4    2.3/0.9

Worst ratio err / E_emul: the C-init forward's LSE, 1.2 - 2.8 (unbiased: mean error < 1e-5), against the
2e-3 cap; every other output stays below 2.6 x E_emul, most at 1.0 - 1.3.

FwdK Run1 / Run2 / Run3 / Run3Smax are reached only through the ctclip_attn_set_fwd_* setters
(test_gpu_ops.py covers them), never by shape; every other FwdK / DqK / DkvK value is in the table.
With the parent's run_ok (no key-mask term) bias_kmask_8x8 and bias_kmask_8x8_leftpad launched
Run3Cinit / Bias32 / Run, which have no key-validity table: O err 1.6, LSE err 5.5.
"""
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import attn_common as A
from test_gpu_dropout import keep_mask

pytestmark = pytest.mark.gpu
dev = 'cuda'
BF16, F32 = torch.bfloat16, torch.float32
SENT16, SENT32 = 0x5AA5, 0x5AA55AA5   # sentinel bit patterns (bf16: 3.7e16, f32: 2.3e16: loud if read)


@pytest.fixture(scope='module')
def K():
    from ctclip_mi355x import kernels
    return kernels


def _lens(L):
    return (L, L - 13, 5)


# id -> (grid or None, L, H, D, nseq, seq layout, extras).  seq: 'frames' = (1, L, 0, 1); 'temporal' = (HW, T HW, 1,
# HW) with HW = nseq; 'interleaved' = (2, 2 L, 1, 2)
SPECS = {
    # base layout, L = 576 (Run3Cinit / FramesDma / FramesDma)
    'base_16x36': dict(grid=(16, 36), H=2, nseq=3),
    'base_36x16': dict(grid=(36, 16), H=2, nseq=3),
    'base_8x72': dict(grid=(8, 72), H=2, nseq=2),
    # row-run kernels off L = 576 (Run3Cinit / FramesRun / Run)
    'run_4x16': dict(grid=(4, 16), H=4, nseq=3),
    'run_16x4': dict(grid=(16, 4), H=4, nseq=3),
    # general bias kernels (Bias32 / Frames / Bias32): padded keys, one partial query block
    'gen_5x7': dict(grid=(5, 7), H=3, nseq=2),
    'gen_7x5': dict(grid=(7, 5), H=3, nseq=2),
    'gen_3x4': dict(grid=(3, 4), H=2, nseq=3),
    # 24 x 24 outside the base layout
    'off_base_nseq1': dict(grid=(24, 24), H=2, nseq=1),
    'off_base_interleaved': dict(grid=(24, 24), H=2, nseq=2, seq='interleaved'),
    'bias_no_dbias_6x6': dict(grid=(6, 6), H=2, nseq=3, dbias=False),
    'bias_no_dbias_8x8': dict(grid=(8, 8), H=2, nseq=3, dbias=False),
    'bias_kmask_8x8': dict(grid=(8, 8), H=2, nseq=3, mask='right'),
    'bias_kmask_6x6': dict(grid=(6, 6), H=2, nseq=3, mask='right'),
    'bias_kmask_8x8_leftpad': dict(grid=(8, 8), H=2, nseq=3, mask='left'),
    'bias_kmask_6x6_leftpad': dict(grid=(6, 6), H=2, nseq=3, mask='left'),
    'bias_d64_6x6': dict(grid=(6, 6), H=2, nseq=3, D=64),
    'bias_d64_8x8': dict(grid=(8, 8), H=2, nseq=3, D=64),
    # plain kernels, pp pairs per workgroup
    'plain32_l40': dict(L=40, H=3, nseq=3, seq='temporal'),                    # pp = 2, 9 pairs: ragged last workgroup
    'plain32_mask_l20': dict(L=20, H=3, nseq=3, mask='right'),                 # pp = 4 (the small kernels refuse masks)
    'plain32_l128_bert': dict(L=128, H=3, nseq=3, mask='bert', qmag=0.3),      # pp = 1
    'plain32_l128_bert_leftpad': dict(L=128, H=3, nseq=3, mask='bert_left'),
    'plain64_l24': dict(L=24, H=3, nseq=3, D=64, mask='right'),                # pp = 4
    'plain64_l9': dict(L=9, H=3, nseq=3, D=64),                                # pp = 8
    'plain64_drop_l40': dict(L=40, H=3, nseq=3, D=64, drop=(0.1, 987654321)),  # pp = 2
    # the one-wave-per-pair kernels (L <= 32, D = 32, no bias / mask): cooperative stores when H % 4 == 0
    'small_h4_l24': dict(L=24, H=4, nseq=5, seq='temporal'),
    'small_h3_l5': dict(L=5, H=3, nseq=3, seq='temporal'),                     # 9 pairs: ragged last workgroup
    # H % 4 == 0 twins for the bias-gradient workspace (taken only when H * nbins % 4 == 0, and nbins is odd)
    'gen_5x7_h4': dict(grid=(5, 7), H=4, nseq=2),
    'base_16x36_h4': dict(grid=(16, 36), H=4, nseq=2),
}
MAIN = [c for c in SPECS if not c.endswith('_h4')]
_CACHE = {}


def case(cid):
    """inputs (q, k, v column slices of wider buffers: ld != H * D), float64 reference and bf16
    emulation of one case, computed once and shared read-only by the tests"""
    if cid in _CACHE:
        return _CACHE[cid]
    sp = SPECS[cid]
    torch.manual_seed(1000 + list(SPECS).index(cid))
    grid = sp.get('grid')
    L = grid[0] * grid[1] if grid else sp['L']
    H, D, nseq = sp['H'], sp.get('D', 32), sp['nseq']
    HD = H * D
    kind = sp.get('seq', 'frames')
    seq = {'frames': (1, L, 0, 1), 'temporal': (nseq, L * nseq, 1, nseq), 'interleaved': (2, 2 * L, 1, 2)}[kind]
    M = nseq * L
    rows = A._gather_rows(*seq, nseq, L, dev)
    assert sorted(rows.reshape(-1).tolist()) == list(range(M))
    u = bins = None
    if grid:
        u, bins = A._cpb_table(H, *grid, dev)
    kmask = None
    mk = sp.get('mask')
    if mk:
        lens = torch.tensor([128, 77, 5] if mk.startswith('bert') else _lens(L))
        ar = torch.arange(L)[None, :]
        kmask = ((ar >= (L - lens)[:, None]) if mk.endswith('left') else (ar < lens[:, None])).int().to(dev)
    qbuf = (torch.randn(M, HD + 8, device=dev) * sp.get('qmag', 0.18)).bfloat16()
    kvbuf = (torch.randn(M, 2 * HD + 16, device=dev) * 0.18).bfloat16()
    q, k, v = qbuf[:, :HD], kvbuf[:, 8:8 + HD], kvbuf[:, 8 + HD:8 + 2 * HD]
    do = torch.randn(M, HD, device=dev).bfloat16()
    drop, keep = sp.get('drop', (0.0, 0)), None
    if drop[0] > 0:
        ar = lambda n, *shape: torch.arange(n, device=dev).reshape(*shape)
        idx = ((ar(nseq, -1, 1, 1, 1) * H + ar(H, 1, -1, 1, 1)) * L + ar(L, 1, 1, -1, 1)) * L + ar(L, 1, 1, 1, -1)
        keep = keep_mask(idx, drop[1], drop[0]).float() * float(np.float32(1.0) / (np.float32(1.0) - np.float32(drop[0])))
    scale = 8.0 if grid else 1.0 / math.sqrt(D)
    ref = A.attn_ref64(q, k, v, do, rows, H, D, scale, u, bins, kmask, keep)
    emul = A.attn_emul_bf16(q, k, v, do, rows, H, D, scale, u, bins, kmask, keep)
    c = SimpleNamespace(id=cid, L=L, H=H, D=D, HD=HD, nseq=nseq, M=M, seq=seq, rows=rows, u=u, bins=bins, kmask=kmask,
                        q=q, k=k, v=v, do=do, drop=drop, scale=scale, ref=ref, emul=emul, dbias=sp.get('dbias', True),
                        kw=dict(L=L, H=H, D=D, nseq=nseq, scale=scale, seq=seq, bias_u=u, grid=grid or (0, 0),
                                kmask=kmask, dropout=drop))
    _CACHE[cid] = c
    return c


def _sentinel(shape, dtype):
    t = torch.empty(shape, device=dev, dtype=dtype)
    t.view(torch.int16 if dtype == BF16 else torch.int32).fill_(SENT16 if dtype == BF16 else SENT32)
    return t


def _out_bufs(c, n):
    """n outputs as column slices [:M, 8 : 8 + HD] of sentinel-filled [M + 16, HD + 16] buffers"""
    bufs = [_sentinel((c.M + 16, c.HD + 16), BF16) for _ in range(n)]
    return bufs, [b[:c.M, 8:8 + c.HD] for b in bufs]


def _untouched(buf, c):
    """every element of the wider buffer outside its [:M, 8 : 8 + HD] slice still holds the sentinel"""
    b = buf.view(torch.int16).clone()
    b[:c.M, 8:8 + c.HD] = SENT16
    return bool((b == SENT16).all())


def _du(c):
    return torch.zeros_like(c.u) if c.u is not None and c.dbias else None


@pytest.mark.parametrize('cid', MAIN)
def test_plan_case(K, cid):
    c = case(cid)
    o, lse = K.attn_fwd(c.q, c.k, c.v, **c.kw)
    bufs, (dq, dk, dv) = _out_bufs(c, 3)
    du = _du(c)
    K.attn_bwd(c.q, c.k, c.v, o, lse, c.do, dq, dk, dv, dbias_u=du, **c.kw)
    A.attn_check(dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv, du=du), c.ref, c.emul, c.rows, c.H, c.D, cid)
    assert all(_untouched(b, c) for b in bufs)


# --------------------------------------------------------------------------- bias-gradient paths
def _bwd_args(K, c, o, lse, du):
    """ctclip_attn_args of the backward with buffers of its own; dbias_ws stays NULL (atomic binning)"""
    dq, dk, dv = (torch.empty(c.M, c.HD, device=dev, dtype=BF16) for _ in range(3))
    delta = torch.empty(c.H, c.M, device=dev, dtype=F32)
    kw = {n: x for n, x in c.kw.items() if n != 'dropout'}
    a = K._attn_args(c.q, c.k, c.v, o, M=c.M, lse=lse, dout=c.do, dq=dq, dk=dk, dv=dv, delta=delta, dbias_u=du,
                     dropout=c.drop, **kw)
    return a, (dq, dk, dv, delta)


@pytest.mark.parametrize('cid', ['run_4x16', 'gen_5x7_h4', 'base_16x36_h4'])
def test_dbias_paths(K, cid):
    """dU binned with atomics (dbias_ws NULL) and through the workspace (K.attn_bwd) both meet the
    float64 tolerance; two workspace runs are bit-identical; both paths ACCUMULATE into dbias_u, as
    include/ctclip_hip.h documents."""
    from ctclip_mi355x import _lib
    c = case(cid)
    o, lse = K.attn_fwd(c.q, c.k, c.v, **c.kw)
    dq, dk, dv = (torch.empty(c.M, c.HD, device=dev, dtype=BF16) for _ in range(3))

    def ws_run(du):
        K.attn_bwd(c.q, c.k, c.v, o, lse, c.do, dq, dk, dv, dbias_u=du, **c.kw)
        return du

    def atomic_run(du):
        a, bufs = _bwd_args(K, c, o, lse, du)
        assert not a.dbias_ws
        _lib.call('ctclip_attn_bwd', _lib.ctypes.byref(a), _lib.stream_ptr())
        return du
    probe, _ = _bwd_args(K, c, o, lse, torch.zeros_like(c.u))
    assert _lib.lib().ctclip_attn_bwd_ws_floats(_lib.ctypes.byref(probe)) > 0, 'the wrapper would not take the workspace'
    du_a = atomic_run(torch.zeros_like(c.u))
    du_w, du_w2 = ws_run(torch.zeros_like(c.u)), ws_run(torch.zeros_like(c.u))
    res = {}
    for name, du in (('atomic', du_a), ('workspace', du_w)):
        res[name] = A.attn_check(dict(du=du), c.ref, c.emul, c.rows, c.H, c.D, f'{cid} {name}')['du']
    assert torch.equal(du_w, du_w2)
    # a known non-zero table is added to, not overwritten: (result - table) is the gradient again, to the
    # f32 rounding of the sums at the table's magnitude (|T| <= 1, a few dozen partial adds: < 1e-5 absolute)
    T = ((torch.arange(c.u.numel(), device=dev) % 17).float() / 16 - 0.5).reshape(c.u.shape)
    rowmax = c.ref['du'].abs().amax(-1).min().item()
    for name, run in (('atomic', atomic_run), ('workspace', ws_run)):
        got = run(T.clone()) - T
        err = A.row_err(got, c.ref['du'])
        print(f'{cid} {name} prefilled: err {err:.3e}')
        assert err <= res[name]['tol'] + 1e-5 / rowmax, (name, err)


# ------------------------------------------------------------------------------ untouched memory
@pytest.mark.parametrize('cid', ['base_16x36', 'gen_5x7', 'plain32_l40', 'plain64_l9'])
def test_untouched_memory(K, cid):
    """o, dq, dk, dv as column slices of wider sentinel-filled buffers with 16 spare rows, lse and
    delta inside longer sentinel-filled vectors: after the forward and backward (C ABI, caller's
    buffers) every element outside the outputs is bit-unchanged, and the outputs are right."""
    from ctclip_mi355x import _lib
    c = case(cid)
    bufs, (o, dq, dk, dv) = _out_bufs(c, 4)
    n = c.H * c.M
    vecs = [_sentinel((n + 64,), F32) for _ in range(2)]
    lse, delta = (x[32:32 + n].view(c.H, c.M) for x in vecs)
    du = _du(c)
    kw = {n_: x for n_, x in c.kw.items() if n_ != 'dropout'}
    a = K._attn_args(c.q, c.k, c.v, o, M=c.M, lse=lse, dout=c.do, dq=dq, dk=dk, dv=dv, delta=delta, dbias_u=du,
                     dropout=c.drop, **kw)
    _lib.call('ctclip_attn_fwd', _lib.ctypes.byref(a), _lib.stream_ptr())
    _lib.call('ctclip_attn_bwd', _lib.ctypes.byref(a), _lib.stream_ptr())
    A.attn_check(dict(o=o, lse=lse, dq=dq, dk=dk, dv=dv, du=du), c.ref, c.emul, c.rows, c.H, c.D, f'{cid} own buffers')
    for name, b in zip(('o', 'dq', 'dk', 'dv'), bufs):
        assert _untouched(b, c), name
    for name, x in zip(('lse', 'delta'), vecs):
        w = x.view(torch.int32)
        assert bool((w[:32] == SENT32).all()) and bool((w[32 + n:] == SENT32).all()), name
        assert bool(torch.isfinite(x[32:32 + n]).all()), name
