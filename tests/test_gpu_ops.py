"""Each HIP kernel family vs a plain torch fp32 reference of the same op (GPU).
The references restate the oracle's semantics (oracle/ctclip_oracle.py) on the same inputs."""
import math

import pytest
import torch
import torch.nn.functional as F

from attn_common import _attn_ref, _cpb_table, _gather_rows
from oracle import ctclip_oracle as O

pytestmark = pytest.mark.gpu
dev = 'cuda'


@pytest.fixture(scope='module')
def K():
    from ctclip_mi355x import kernels
    return kernels


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


# ----------------------------------------------------------------------------- LayerNorm
@pytest.mark.parametrize('D,eps,bias', [(512, 1e-5, False), (512, 1e-5, True), (768, 1e-12, True), (64, 1e-5, True)])
def test_layernorm(K, D, eps, bias):
    torch.manual_seed(0)
    x = torch.randn(1000, D, device=dev) * 3 + 1
    g = torch.randn(D, device=dev) * 0.1 + 1
    b = torch.randn(D, device=dev) * 0.1 if bias else None
    yb, yf, mean, rstd = K.layernorm_fwd(x, g, b, eps, out_f32=True)
    xr = x.clone().requires_grad_(True)
    gr = g.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True) if bias else None
    ref = F.layer_norm(xr, (D,), gr, br, eps)
    assert rel(yf, ref) < 1e-6
    assert rel(yb, ref) < 4e-3
    dy = torch.randn_like(x)
    res = torch.randn_like(x)
    ref.backward(dy)
    dxf, dxb, dg, db = K.layernorm_bwd(dy, x, mean, rstd, g, dres=res, want_beta=bias)
    assert rel(dxf, xr.grad + res) < 1e-5
    assert rel(dg, gr.grad) < 1e-5
    if bias:
        assert rel(db, br.grad) < 1e-5


def test_l2norm_scale(K):
    torch.manual_seed(1)
    H, D = 8, 32
    x = torch.randn(777, 512, device=dev).bfloat16()   # use the k half of a kv-like buffer
    sc = torch.randn(D, device=dev) * 0.1 + 1
    y = K.l2norm_scale_fwd(x[:, :256], H, D, sc)
    xr = x[:, :256].float().reshape(-1, H, D).requires_grad_(True)
    scr = sc.clone().requires_grad_(True)
    ref = F.normalize(xr, dim=-1) * scr
    assert rel(y.reshape(-1, H, D), ref) < 4e-3
    dy = torch.randn(777, 256, device=dev).bfloat16()
    ref.backward(dy.float().reshape(-1, H, D))
    dx = torch.empty(777, 512, device=dev, dtype=torch.bfloat16)
    ds = K.l2norm_scale_bwd(x[:, :256], dy, H, D, sc, dx[:, :256])
    assert rel(dx[:, :256].reshape(-1, H, D), xr.grad) < 8e-3
    assert rel(ds, scr.grad) < 1e-4


# ----------------------------------------------------------------------------- PEG
def _peg_ref(x, w, b, shape, mode):
    """x canonical (b t h w) rows [M, D] f32; returns out (with residual) via the oracle."""
    B, T, H, W = shape
    D = x.shape[1]
    sd = {'p.dsconv.weight': w, 'p.dsconv.bias': b}
    if mode == 0:
        xs = x.reshape(B * T, H * W, D)
        return (O.peg_forward(sd, 'p.', xs, shape) + xs).reshape(-1, D)
    xt = x.reshape(B, T, H, W, D).permute(0, 2, 3, 1, 4).reshape(B * H * W, T, D)
    y = O.peg_forward(sd, 'p.', xt, shape) + xt
    return y.reshape(B, H, W, T, D).permute(0, 3, 1, 2, 4).reshape(-1, D)


@pytest.mark.parametrize('mode', [0, 1])
def test_peg_bwd_x32(K, mode):
    """The input gradient from the f32 dout (ctclip_peg_bwd_data_x32: the transposed conv in f32, the
    view-space walk run backward in t, the canonical temporal walk forward) against an f64 reference
    with a dout that bf16 cannot hold: closer than the bf16-tap tile kernel, which reads the conv
    taps from dout's bf16 copy; the weight / bias gradients are unchanged.  Both walks of mode 1."""
    from ctclip_mi355x import _lib
    torch.manual_seed(21 + mode)
    shape, D = (2, 24, 24, 24), 128
    M = 2 * 24 ** 3
    xb = torch.randn(M, D, device=dev).bfloat16()
    w = torch.randn(D, 1, 3, 3, 3, device=dev) * 0.2
    b = torch.randn(D, device=dev) * 0.1
    dyf = torch.randn(M, D, device=dev)
    xr = xb.double().requires_grad_(True)
    _peg_ref(xr, w.double(), b.double(), shape, mode).backward(dyf.double())
    res = {}
    for x32 in (True, False):
        old = K._PEG_BWD_X32
        K._PEG_BWD_X32 = x32
        try:
            res[x32] = K.peg_bwd(dyf.bfloat16(), dyf, xb, *shape, w, mode)
        finally:
            K._PEG_BWD_X32 = old
    e32, e16 = rel(res[True][0], xr.grad), rel(res[False][0], xr.grad)
    print(f'PEG input gradient mode {mode}: x32 rel {e32:.2e}, bf16-tap {e16:.2e}')
    assert e32 < 1e-6 and e32 < 0.1 * e16
    assert rel(res[True][1].float(), res[True][0]) < 4e-3       # the bf16 copy of dx
    assert torch.equal(res[True][2], res[False][2]) and torch.equal(res[True][3], res[False][3])
    if mode == 1:   # the view-order walk of the same gradient
        prev = _lib.lib().ctclip_peg_set_canon1(0)
        try:
            alt = K.peg_bwd(dyf.bfloat16(), dyf, xb, *shape, w, mode)
        finally:
            _lib.lib().ctclip_peg_set_canon1(prev)
        assert rel(alt[0], xr.grad) < 1e-6


def test_peg_canonical_walk_matches_view_walk(K):
    """Mode 1 on the 24^3 cube: the canonical-order walk (default) against the view-order walk."""
    from ctclip_mi355x import _lib
    torch.manual_seed(9)
    shape, D = (2, 24, 24, 24), 128
    M = 2 * 24 ** 3
    xb = torch.randn(M, D, device=dev).bfloat16()
    w = torch.randn(D, 1, 3, 3, 3, device=dev) * 0.2
    b = torch.randn(D, device=dev) * 0.1
    dy = torch.randn(M, D, device=dev).bfloat16()
    outs = []
    for on in (1, 0):
        old = _lib.lib().ctclip_peg_set_canon1(on)
        try:
            outs.append((K.peg_fwd(xb, xb.float(), *shape, w, b, 1), K.peg_bwd(dy, dy.float(), xb, *shape, w, 1)))
        finally:
            _lib.lib().ctclip_peg_set_canon1(old)
    (f1, b1), (f0, b0) = outs
    assert rel(f1[0], f0[0]) < 1e-6 and rel(b1[0], b0[0]) < 1e-6
    assert rel(b1[2], b0[2]) < 1e-5 and rel(b1[3], b0[3]) < 1e-5


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('shape,D', [((2, 6, 5, 7), 128),      # plane-streaming path, ragged h tile / w segment
                                     ((1, 24, 24, 24), 512),   # base token grid (480^2 x 240 volume)
                                     ((2, 24, 24, 24), 128),   # two volumes (mode 1: canonical walk)
                                     ((1, 3, 4, 40), 64),      # W > 24 (tiled_ok's limit): general path
                                     ((2, 2, 3, 4), 24)])      # D % 64 != 0: general path
def test_peg(K, mode, shape, D):
    torch.manual_seed(2)
    M = shape[0] * shape[1] * shape[2] * shape[3]
    xb = torch.randn(M, D, device=dev).bfloat16()
    xf = xb.float()
    w = torch.randn(D, 1, 3, 3, 3, device=dev) * 0.2
    b = torch.randn(D, device=dev) * 0.1
    outf, outb = K.peg_fwd(xb, xf, *shape, w, b, mode)
    xr = xf.clone().requires_grad_(True)
    wr = w.clone().requires_grad_(True)
    br = b.clone().requires_grad_(True)
    ref = _peg_ref(xr, wr, br, shape, mode)
    assert rel(outf, ref) < 1e-5
    dy = torch.randn(M, D, device=dev).bfloat16()
    ref.backward(dy.float())
    dxf, dxb, dw, db = K.peg_bwd(dy, dy.float(), xb, *shape, w, mode)
    assert rel(dxf, xr.grad) < 1e-5
    assert rel(dw, wr.grad.reshape(D, 27)) < 1e-5
    assert rel(db, br.grad) < 1e-5


@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('shape,D', [((2, 6, 5, 7), 128), ((1, 24, 24, 24), 512), ((2, 24, 24, 24), 64),
                                     ((8, 24, 24, 24), 512), ((1, 3, 4, 40), 64), ((2, 2, 3, 4), 24)])
def test_peg_x32(K, mode, shape, D):
    """The f32-tap PEG forward (ctclip_peg_fwd_x32): f32 x (not bf16-representable) against the torch
    fp32 conv, its 16-bit copies the casts of its f32 output, and the LayerNorm statistics of the
    output rows (32-channel groups merged) against torch."""
    torch.manual_seed(12)
    M = shape[0] * shape[1] * shape[2] * shape[3]
    xf = torch.randn(M, D, device=dev) + 0.25
    w = torch.randn(D, 1, 3, 3, 3, device=dev) * 0.2
    b = torch.randn(D, device=dev) * 0.1
    tiled = D % 32 == 0 and shape[3] <= 24
    outf, outb, outh, mean, rstd = K.peg_fwd_x32(xf, *shape, w, b, mode, stats=tiled, want_f16=True)
    ref = _peg_ref(xf, w, b, shape, mode)
    assert rel(outf, ref) < 1e-5
    # repeat: bit-identical (the plane ring has no read / overwrite race; the temporal map's walk
    # reads the previous plane's centre row in the step that overwrites its slot)
    for _ in range(3):
        assert torch.equal(K.peg_fwd_x32(xf, *shape, w, b, mode)[0], outf)
    assert torch.equal(outb, outf.bfloat16()) and torch.equal(outh, outf.half())
    if tiled:
        var, mu = torch.var_mean(outf.double(), dim=1, unbiased=False)
        assert rel(mean, mu) < 1e-5
        assert rel(rstd, torch.rsqrt(var + 1e-5)) < 1e-5


# ----------------------------------------------------------------------------- attention
@pytest.mark.parametrize('case', ['spatial', 'spatial_small', 'spatial_8x8', 'temporal', 'temporal_l5_h3', 'temporal_l32', 'bert',
                                  'bert_leftpad'])
def test_attention(K, case):
    torch.manual_seed(3)
    if case.startswith('spatial'):
        # 24 x 24 and 8 x 8 take the row-run bias path (Wg % 4 == 0, L % 32 == 0), 6 x 6 the general one
        gh = gw = {'spatial': 24, 'spatial_small': 6, 'spatial_8x8': 8}[case]
        L, H, D, nseq = gh * gw, 8, 32, 3
        M = nseq * L
        seq = (1, L, 0, 1)
        scale = 8.0
        u, bins = _cpb_table(H, gh, gw)
        bias = u[:, bins]
        kmask = None
        grid = (gh, gw)
    elif case.startswith('temporal'):
        # fused short-sequence kernels (attn_small_*): L <= 32, one wave per (sequence, head);
        # ragged pair counts (nseq * H not a multiple of the 4 waves of a workgroup)
        B, T, HW, H = {'temporal': (2, 24, 20, 8), 'temporal_l5_h3': (1, 5, 7, 3), 'temporal_l32': (3, 32, 3, 8)}[case]
        L, D, nseq = T, 32, B * HW
        M = B * T * HW
        seq = (HW, T * HW, 1, HW)
        scale, u, bias, kmask, grid = 8.0, None, None, None, (0, 0)
    else:
        B, L, H, D = 3, 128, 12, 64
        nseq, M = B, B * 128
        seq = (1, L, 0, 1)
        scale, u, bias, grid = 1 / 8, None, None, (0, 0)
        lens = torch.tensor([128, 77, 5])
        kmask = (torch.arange(L)[None, :] < lens[:, None]).int().to(dev)
        if case == 'bert_leftpad':
            # leading masked keys (left padding): whole first key chunks of -inf scores, which the
            # lazy online-softmax rescale must still start from (exp2(-inf - -inf))
            kmask = (torch.arange(L)[None, :] >= (L - lens)[:, None]).int().to(dev)
    rows = _gather_rows(*seq, nseq, L)
    q = (torch.randn(M, H * D, device=dev) * (0.3 if case == 'bert' else 0.18)).bfloat16()
    kv = (torch.randn(M, 2 * H * D, device=dev) * 0.18).bfloat16()
    k, v = kv[:, :H * D], kv[:, H * D:]
    o, lse = K.attn_fwd(q, k, v, L=L, H=H, D=D, nseq=nseq, scale=scale, seq=seq, bias_u=u, grid=grid, kmask=kmask)
    qr, kr, vr = q.float().requires_grad_(True), k.float().requires_grad_(True), v.float().requires_grad_(True)
    ur = u.clone().requires_grad_(True) if u is not None else None
    ref = _attn_ref(qr, kr, vr, rows, H, D, scale, ur[:, bins] if u is not None else None, kmask)
    assert rel(o, ref) < 8e-3, rel(o, ref)
    do = torch.randn(M, H * D, device=dev).bfloat16()
    ref.backward(do.float())
    dq = torch.empty(M, H * D, device=dev, dtype=torch.bfloat16)
    dkv = torch.empty(M, 2 * H * D, device=dev, dtype=torch.bfloat16)
    du = torch.zeros_like(u) if u is not None else None
    K.attn_bwd(q, k, v, o, lse, do, dq, dkv[:, :H * D], dkv[:, H * D:], L=L, H=H, D=D, nseq=nseq, scale=scale,
               seq=seq, bias_u=u, dbias_u=du, grid=grid, kmask=kmask)
    assert rel(dq, qr.grad) < 2e-2, rel(dq, qr.grad)
    assert rel(dkv[:, :H * D], kr.grad) < 2e-2, rel(dkv[:, :H * D], kr.grad)
    assert rel(dkv[:, H * D:], vr.grad) < 2e-2, rel(dkv[:, H * D:], vr.grad)
    if u is not None:
        assert rel(du, ur.grad) < 2e-2, rel(du, ur.grad)


def test_attention_rejects_unaligned_rows(K):
    """Rows 16-B aligned (ld % 8 == 0) are part of the attention C-ABI contract (ctclip_hip.h: the
    kernels load and store 8 head-dim elements per lane): anything else fails loudly (CT_EALIGN)."""
    from ctclip_mi355x import _lib
    M, H, D, L = 48, 8, 32, 24
    q = torch.zeros(M, 260, device=dev, dtype=torch.bfloat16)[:, :H * D]      # ld 260
    kv = torch.zeros(M, 2 * H * D, device=dev, dtype=torch.bfloat16)
    with pytest.raises(_lib.KernelError):
        K.attn_fwd(q, kv[:, :H * D], kv[:, H * D:], L=L, H=H, D=D, nseq=M // L, scale=8.0, seq=(1, L, 0, 1))
    o, _ = K.attn_fwd(q.contiguous(), kv[:, :H * D], kv[:, H * D:], L=L, H=H, D=D, nseq=M // L, scale=8.0,
                      seq=(1, L, 0, 1))
    assert torch.isfinite(o.float()).all()


# ----------------------------------------------------------------------------- VQ
def test_vq_select_and_pool(K):
    torch.manual_seed(4)
    M, D, C = 3000, 512, 8192
    x = torch.randn(M, D, device=dev)
    cb = F.normalize(torch.randn(C, D, device=dev), dim=-1)
    xn = F.normalize(x, dim=-1)
    # near-ties inside one 64-code group that bf16 cannot order: rows 0..63 each get two codes
    # (group 2i, in-group slots 5 and 9) at cosine ~0.9998 with them, 1e-5..1e-4 apart -- the bf16
    # GEMM scores both the same, so only the full-group f32 re-score finds the winner
    g = torch.Generator(device=dev).manual_seed(11)
    for i in range(64):
        for slot in (5, 9):
            cb[128 * i + slot] = F.normalize(xn[i] + 0.02 * F.normalize(torch.randn(D, device=dev, generator=g),
                                                                        dim=0), dim=0)
    nt = C // 64
    cand = torch.empty(M, nt, 2, device=dev)
    cand2 = torch.empty(M, nt, device=dev)
    K.gemm_raw(M, C, D, xn.bfloat16(), D, True, cb.bfloat16(), D, True, cand, nt, C2=cand2, ldc2=nt,
               act=K.ACT_ARGMAX)
    idx, xno = K.vq_select(cand, x, cb, cand2=cand2)
    s64 = F.normalize(x.double(), dim=-1) @ cb.double().t()
    top2 = s64.topk(2, dim=1).values
    ref = s64.argmax(1)
    tie = (top2[:, 0] - top2[:, 1]) < 1e-6        # only f32-level ties may differ
    assert (idx.long() != ref)[~tie].sum().item() == 0
    # the fp16 scoring path (round 6, functional.vq_assign's default): fp16 l2norm(x) against the
    # fp16 codebook image, re-score margin 4e-3 -- the same exact f32 argmax, on the 8-phase kernel
    # (M = 3000) and the 128-tile one (M = 200)
    for Mh in (M, 200):
        candh = torch.empty(Mh, nt, 2, device=dev)
        cand2h = torch.empty(Mh, nt, device=dev)
        K.gemm_raw(Mh, C, D, K.vq_l2norm_h16(x[:Mh]), D, True, K.split_f16(cb)[0], D, True, candh, nt, C2=cand2h,
                   ldc2=nt, act=K.ACT_ARGMAX)
        idx_h, _ = K.vq_select(candh, x[:Mh], cb, margin=4e-3, cand2=cand2h)
        assert (idx_h.long() != ref[:Mh])[~tie[:Mh]].sum().item() == 0
    # group winners only (cand2 = None) miss some of the in-group near-ties: the case the full-group
    # re-score exists for
    idx_w, _ = K.vq_select(cand, x, cb)
    print('near-tie rows resolved only by the full-group re-score:',
          (idx_w.long()[:64] != ref[:64]).sum().item(), 'of 64')
    assert rel(xno, xn) < 1e-6
    B, T, HW = 3, 10, 100
    pooled, pooled_b = K.vq_pool(idx, cb, B, T, HW)
    refp = cb[idx.long()].reshape(B, T, HW, D).mean(1).reshape(B, -1)
    assert rel(pooled, refp) < 1e-6
    # EMA restatement vs oracle
    bins = torch.zeros(C, device=dev)
    esum = torch.zeros(C, D, device=dev, dtype=torch.int64)
    K.vq_ema_accum(idx, xno, bins, esum)
    # fixed-point sums: order-independent, so equal to the 2^-40-rounded rows summed on the host
    fx = torch.zeros(C, D, dtype=torch.int64).index_add_(0, idx.long().cpu(),
                                                         torch.round(xno.cpu().double() * 2 ** 40).long())
    assert torch.equal(esum.cpu(), fx)
    assert torch.equal(bins.cpu(), torch.bincount(idx.long().cpu(), minlength=C).float())
    # the code-sorted kernels: the same statistics bit for bit, on these rows and on a skewed index
    # set (most rows on three codes, as from an untrained codebook) at the step's row count; the
    # work buffer's count region is left zero, so a second call accumulates again
    work = torch.zeros(2 * C + 2 * M, device=dev, dtype=torch.int32)
    bins_s = torch.zeros(C, device=dev)
    esum_s = torch.zeros(C, D, device=dev, dtype=torch.int64)
    K.vq_ema_accum(idx, xno, bins_s, esum_s, work=work)
    assert torch.equal(esum_s, esum) and torch.equal(bins_s, bins)
    assert work[:C].abs().sum().item() == 0
    Mb = 110592
    gsk = torch.Generator(device=dev).manual_seed(12)
    ids = torch.randint(0, C, (Mb,), device=dev, generator=gsk, dtype=torch.int32)
    hotm = torch.rand(Mb, device=dev, generator=gsk) < 0.9
    hot = torch.tensor([7, 4000, 8191], device=dev, dtype=torch.int32)
    ids[hotm] = hot[torch.randint(0, 3, (int(hotm.sum().item()),), device=dev, generator=gsk)]
    xs = F.normalize(torch.randn(Mb, D, device=dev, generator=gsk), dim=-1)
    for ix in (ids, torch.randint(0, C, (Mb,), device=dev, generator=gsk, dtype=torch.int32)):
        b0, e0 = torch.zeros(C, device=dev), torch.zeros(C, D, device=dev, dtype=torch.int64)
        K.vq_ema_accum(ix, xs, b0, e0)
        wk = torch.zeros(2 * C + 2 * Mb, device=dev, dtype=torch.int32)
        b1, e1 = torch.zeros(C, device=dev), torch.zeros(C, D, device=dev, dtype=torch.int64)
        K.vq_ema_accum(ix, xs, b1, e1, work=wk)
        K.vq_ema_accum(ix, xs, b1, e1, work=wk)     # twice: statistics double exactly
        assert torch.equal(b1, 2 * b0) and torch.equal(e1, 2 * e0)
    emb = cb.clone()
    cs = torch.zeros(C, device=dev)
    K.vq_ema_finalize(bins, esum, 0.8, emb, cs)
    _, _, ne, ncs = O.vq_forward(x.cpu(), cb.cpu()[None], torch.zeros(1, C), True, 0.8, force_ind=idx.cpu())
    assert rel(emb.cpu(), ne[0]) < 1e-5
    assert rel(cs.cpu(), ncs[0]) < 1e-6
    # non-finite tokens: the row maps to code 0 and its normalised row is zero, so the
    # EMA statistics stay finite and code 0's direction is untouched by it
    xbad = x[:128].clone()
    xbad[3] = float('nan')
    xbad[7, 5] = float('inf')
    cb_ = cb.bfloat16()
    cand_b = torch.empty(128, nt, 2, device=dev)
    cand2_b = torch.empty(128, nt, device=dev)
    K.gemm_raw(128, C, D, F.normalize(xbad, dim=-1).bfloat16(), D, True, cb_, D, True, cand_b, nt, C2=cand2_b,
               ldc2=nt, act=K.ACT_ARGMAX)
    idb, xnb = K.vq_select(cand_b, xbad, cb, cand2=cand2_b)
    assert idb[3].item() == 0 and idb[7].item() == 0
    assert torch.isfinite(xnb).all() and xnb[3].abs().sum().item() == 0 and xnb[7].abs().sum().item() == 0
    assert torch.equal(idb[:3], idx[:3])
    # ... and flags the sticky step status word (CT_STATUS_VQ_NONFINITE = 8), cleared here so the
    # trainer tests that follow in the same process start from a clean word
    assert int(K.status_word(dev).item()) & 8
    K.reset_ln_status(dev)
    bins_b = torch.zeros(C, device=dev)
    esum_b = torch.zeros(C, D, device=dev, dtype=torch.int64)
    K.vq_ema_accum(idb, xnb, bins_b, esum_b)
    emb_b = cb.clone()
    K.vq_ema_finalize(bins_b, esum_b, 0.8, emb_b, torch.zeros(C, device=dev))
    assert torch.isfinite(emb_b).all()


def _seq_f32_scores(xn, rows_cb):
    """x_n . w in f32 as vq.hip's score_seq sums it: k = 0 .. D-1, one fused multiply-add per term
    (each fma emulated in f64: the product is exact there, the sum rounds twice only at an f32
    midpoint, ~2^-29 per term)."""
    d = torch.zeros(rows_cb.shape[0], dtype=torch.float64, device=xn.device)
    xd, wd = xn.double(), rows_cb.double()
    for k in range(xn.shape[-1]):
        d = (xd[..., k] * wd[:, k] + d).float().double()
    return d


def test_vq_select_order_independent(K):
    """Round 6: vq_select's index is the argmax of the SEQUENTIAL f32 dot product (ties to the lowest
    code) whatever the GEMM that proposed the candidates -- bf16 operands with margin 2e-2 or fp16
    with 4e-3 give the same index on every row, sub-ulp near-ties and exact duplicate codes included."""
    torch.manual_seed(5)
    M, D, C = 2048, 512, 8192
    x = torch.randn(M, D, device=dev)
    cb = F.normalize(torch.randn(C, D, device=dev), dim=-1)
    xn = F.normalize(x, dim=-1)
    g = torch.Generator(device=dev).manual_seed(12)
    # rows 0..127: two codes (one group or two) within ~1e-7 of each other in f64 -- about one f32
    # ulp at 0.9998; rows 128..191: an exact duplicate of the winning code at a higher index
    for i in range(128):
        base = F.normalize(xn[i] + 0.02 * F.normalize(torch.randn(D, device=dev, generator=g), dim=0), dim=0)
        tweak = base + 1e-7 * torch.randn(D, device=dev, generator=g)
        cb[64 * i + 3] = base
        cb[64 * ((i + i % 2) % 128) + 7] = F.normalize(tweak, dim=0)   # same group (even i) or the next
    for i in range(128, 192):
        w = F.normalize(xn[i] + 0.02 * F.normalize(torch.randn(D, device=dev, generator=g), dim=0), dim=0)
        cb[64 * (i - 128) + 11] = w
        cb[64 * (i - 128 + 64) + 11] = w
    nt = C // 64
    cand = torch.empty(M, nt, 2, device=dev)
    cand2 = torch.empty(M, nt, device=dev)
    K.gemm_raw(M, C, D, xn.bfloat16(), D, True, cb.bfloat16(), D, True, cand, nt, C2=cand2, ldc2=nt,
               act=K.ACT_ARGMAX)
    idx_b, xno = K.vq_select(cand, x, cb, cand2=cand2)
    candh = torch.empty(M, nt, 2, device=dev)
    cand2h = torch.empty(M, nt, device=dev)
    K.gemm_raw(M, C, D, K.vq_l2norm_h16(x), D, True, K.split_f16(cb)[0], D, True, candh, nt, C2=cand2h,
               ldc2=nt, act=K.ACT_ARGMAX)
    idx_h, _ = K.vq_select(candh, x, cb, margin=4e-3, cand2=cand2h)
    assert torch.equal(idx_b, idx_h)
    # the near-tie and duplicate rows against the sequential f32 sum of the kernel's own x_n: the
    # winner among the 8 best f64 codes (every code within the select's window is among them)
    s64 = xno.double() @ cb.double().t()
    top = s64[:192].topk(8, dim=1).indices
    seq = torch.stack([_seq_f32_scores(xno[r], cb[top[r]]) for r in range(192)])
    best = seq.max(1, keepdim=True).values
    win = torch.where(seq == best, top, torch.full_like(top, C)).min(1).values   # ties: lowest code
    assert torch.equal(idx_b[:192].long(), win)
    assert (idx_b[128:192].long() == 64 * torch.arange(64, device=dev) + 11).all()   # the lower duplicate
    ties = (seq.topk(2, dim=1).values[:, 0] - seq.topk(2, dim=1).values[:, 1] == 0).sum().item()
    print(f'order-independent select: {M} rows, bf16 vs fp16 candidates identical; {ties} of 192 '
          'constructed rows tie exactly in f32 (lowest code wins)')


# ----------------------------------------------------------------------------- loss
@pytest.mark.parametrize('Bg', [2, 8, 64])
def test_clip_loss(K, Bg):
    torch.manual_seed(5)
    t = torch.randn(Bg, 512, device=dev)
    i = torch.randn(Bg, 512, device=dev)
    lt = torch.tensor([1.0], device=dev)
    loss, dt, di, dlt, tn, inn, sim = K.clip_loss(t, i, lt)
    tr, ir, ltr = t.clone().requires_grad_(True), i.clone().requires_grad_(True), lt.clone().requires_grad_(True)
    ref = O.infonce(F.normalize(tr, dim=-1), F.normalize(ir, dim=-1), ltr[0])
    ref.backward()
    assert abs(loss.item() - ref.item()) < 1e-5
    assert rel(dt, tr.grad) < 1e-4
    assert rel(di, ir.grad) < 1e-4
    assert abs(dlt.item() - ltr.grad.item()) < 1e-4 * max(1, abs(ltr.grad.item()))
    sc = K.clip_scores(t, i, lt)
    assert rel(sc, (F.normalize(t, dim=-1) * F.normalize(i, dim=-1)).sum(-1) * math.e) < 1e-6


# ----------------------------------------------------------------------------- sgemm / CPB
def test_sgemm_cpb_mlp(K):
    torch.manual_seed(6)
    x = O.cpb_rel_pos(24, 24).reshape(-1, 2)
    rel_u = torch.unique(x, dim=0).to(dev)
    w0, b0 = torch.randn(512, 2, device=dev), torch.randn(512, device=dev) * 0.1
    w1, b1 = torch.randn(512, 512, device=dev) / 22, torch.randn(512, device=dev) * 0.1
    h1 = K.slinear(rel_u, w0, b0, act=1)
    h2 = K.slinear(h1, w1, b1, act=1)
    ref = F.leaky_relu(F.linear(F.leaky_relu(F.linear(rel_u, w0, b0), 0.1), w1, b1), 0.1)
    assert rel(h2, ref) < 1e-5
    g = torch.randn_like(h2)
    dz = K.smm(g, w1, act=2, aux=h1)          # dh1 * leaky'(h1)
    ref2 = (g @ w1) * torch.where(h1 > 0, 1.0, 0.1)
    assert rel(dz, ref2) < 1e-5
    dw = K.smm(g.t(), h1)                     # K = 2,209: split-K slabs
    assert rel(dw, g.t() @ h1) < 1e-5
    du = torch.randn(8, h2.shape[0], device=dev)
    dw2 = K.smm(du, h2)                       # 8 x 512, K = 2,209 (one row of tiles)
    assert rel(dw2, du @ h2) < 1e-5
    acc = torch.randn(8, 512, device=dev)
    ref_acc = acc + du @ h2
    K.smm(du, h2, out=acc, accumulate=True)
    assert rel(acc, ref_acc) < 1e-5


def test_sgemm_exact_integers(K):
    """Small-integer operands: every product and partial sum is exact in f32, so the MFMA path
    must reproduce the fp64 result bit for bit (catches row/column swaps and lost K slices)."""
    torch.manual_seed(9)
    for (M, N, Kd) in [(70, 33, 45), (128, 64, 2209), (5, 300, 17)]:
        a = torch.randint(-3, 4, (M, Kd), device=dev).float()
        b = torch.randint(-3, 4, (N, Kd), device=dev).float()
        y = K.slinear(a, b)
        assert torch.equal(y, (a.double() @ b.double().t()).float())
        y2 = K.smm(a.t().contiguous().t(), b.t())   # column-major A view
        assert torch.equal(y2, (a.double() @ b.double().t()).float())


# ----------------------------------------------------------------------------- patch embed
@pytest.mark.parametrize('size,f32', [(40, False),     # strip path, ragged 2-patch group
                                      (160, False),    # strip path, full groups
                                      (100, False),    # Wg = 5: ragged group of 1 -> gather path
                                      (80, True)])     # f32 [-1, 1] video input
def test_patch_ln(K, size, f32):
    torch.manual_seed(7)
    hu = torch.randint(-1200, 1201, (2, 1, 20, size, size), dtype=torch.int16, device=dev)
    from ctclip_mi355x import layers
    offs = layers.patch_offsets(1, 10, 20, 20, size, size).to(dev)
    v = O.normalize_hu(hu.cpu())
    xh = K.patch_ln(v.to(dev) if f32 else hu, not f32, 10, 20, offs)
    b, c, f, hh, ww = v.shape
    g = size // 20
    x = v.reshape(b, c, 2, 10, g, 20, g, 20).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(-1, 4000)
    ref = F.layer_norm(x, (4000,), eps=1e-5)
    assert rel(xh.cpu(), ref) < 4e-3
    # bf16 of the f32 LN of identical inputs: every element within one bf16 ulp
    assert ((xh.cpu().float() - ref).abs() <= ref.abs() * 2 ** -7 + 1e-6).all()
    # padded row stride (the patch-embed GEMM's K = 4032): same values, zero pad columns
    xp = K.patch_ln(v.to(dev) if f32 else hu, not f32, 10, 20, offs, ld=4032)
    assert torch.equal(xp[:, :4000].cpu(), xh.cpu())
    assert (xp[:, 4000:] == 0).all()


def test_embed(K):
    torch.manual_seed(8)
    ids = torch.randint(0, 100, (3, 16), device=dev)
    word = torch.randn(100, 64, device=dev)
    pos = torch.randn(32, 64, device=dev)
    typ = torch.randn(2, 64, device=dev)
    out = K.embed_fwd(ids, word, pos, typ[0])
    ref = word[ids] + pos[:16][None] + typ[0]
    assert rel(out.reshape(3, 16, 64), ref) < 1e-6
    dx = torch.randn(48, 64, device=dev)
    dw, dp, dt = torch.zeros_like(word), torch.zeros_like(pos), torch.zeros(64, device=dev)
    K.embed_bwd(ids, dx, dw, dp, dt)
    refw = torch.zeros_like(word).index_add_(0, ids.reshape(-1), dx)
    assert rel(dw, refw) < 1e-6
    assert rel(dp[:16], dx.reshape(3, 16, 64).sum(0)) < 1e-6
    assert rel(dt, dx.sum(0)) < 1e-6


@pytest.mark.parametrize('B,L,V,Hd', [(8, 128, 50, 768), (2, 600, 3000, 1200), (1, 1, 10, 4)])
def test_embed_bwd_padding_and_reproducible(K, B, L, V, Hd):
    """Ragged reports: pad id 0 gets no word-table gradient (transformers BertEmbeddings builds
    the table with padding_idx = pad_token_id; torch F.embedding(padding_idx=0) is the
    reference); many repeated ids (V small); no float atomics, so repeated calls are bit-equal;
    accumulates into existing .grad."""
    g = torch.Generator(device=dev).manual_seed(B * 1000 + L)
    ids = torch.randint(1, V, (B, L), device=dev, generator=g)
    for b in range(B):
        ids[b, L - L // (b + 2):] = 0                  # ragged tails of pad id 0
    word = torch.randn(V, Hd, device=dev, generator=g, requires_grad=True)
    pos = torch.randn(L + 3, Hd, device=dev, generator=g, requires_grad=True)
    typ = torch.randn(2, Hd, device=dev, generator=g, requires_grad=True)
    dx = torch.randn(B * L, Hd, device=dev, generator=g)
    x = torch.nn.functional.embedding(ids, word, padding_idx=0) + pos[:L][None] + typ[0]
    x.backward(dx.reshape(B, L, Hd))
    base = [torch.randn(V, Hd, device=dev, generator=g), torch.randn(L + 3, Hd, device=dev, generator=g),
            torch.randn(Hd, device=dev, generator=g)]
    outs = []
    for _ in range(3):
        dw, dp, dt = (t.clone() for t in base)
        K.embed_bwd(ids, dx, dw, dp, dt, pad_id=0)
        outs.append((dw, dp, dt))
    for o in outs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(o, outs[0]))
    dw, dp, dt = outs[0]
    assert torch.equal(dw[0], base[0][0])               # pad row untouched
    assert rel(dw - base[0], word.grad) < 1e-6
    assert rel(dp - base[1], pos.grad) < 1e-6
    assert rel(dt - base[2], typ.grad[0]) < 1e-6
    # only the tables asked for
    dw2 = base[0].clone()
    K.embed_bwd(ids, dx, dw2, None, None, pad_id=0)
    assert torch.equal(dw2, dw)


def test_adam_and_norm(K):
    torch.manual_seed(9)
    n = 100003
    p = torch.randn(n, device=dev)
    g = torch.randn(n, device=dev)
    m = torch.zeros(n, device=dev)
    v = torch.zeros(n, device=dev)
    out = torch.empty(2, device=dev)
    K.grad_norm(g, 0.5, out)
    assert abs(out[0].item() - g.norm().item()) < 1e-3 * g.norm().item()
    pr = p.clone().requires_grad_(True)
    opt = torch.optim.Adam([pr], lr=1e-3, betas=(0.9, 0.99), eps=1e-8)
    pr.grad = g * out[1]
    opt.step()
    pb = torch.empty(n, device=dev, dtype=torch.bfloat16)
    K.adam(p, g, m, v, lr=1e-3, b1=0.9, b2=0.99, eps=1e-8, wd=0.0, step=1, coef=out, p_bf16=pb)
    assert rel(p, pr.detach()) < 1e-6
    assert rel(pb, p) < 4e-3


@pytest.mark.gpu
def test_adam_unaligned_slices_and_zero_grad(K):
    """Arena slices at every 16-B phase and ragged lengths (the vector body's scalar head and
    tail), the bf16 shadow, the fused zero_grad, and nothing outside the slice touched."""
    torch.manual_seed(10)
    N = 4099
    for off in range(4):
        for n in (1, 3, 5, 1027, N - 8):
            p = torch.randn(N, device=dev)
            g = torch.randn(N, device=dev)
            m = torch.randn(N, device=dev) * 0.1
            v = torch.rand(N, device=dev) * 0.1
            pb = torch.zeros(N, device=dev, dtype=torch.bfloat16)
            coef = torch.tensor([1.0, 0.37], device=dev)
            p0, g0, m0, v0 = p.clone(), g.clone(), m.clone(), v.clone()
            sl = slice(off, off + n)
            K.adam(p[sl], g[sl], m[sl], v[sl], lr=1e-3, b1=0.9, b2=0.99, eps=1e-8, wd=0.0, step=3, coef=coef,
                   p_bf16=pb[sl], zero_grad=True)
            gi = g0[sl] * 0.37
            mi = 0.9 * m0[sl] + 0.1 * gi
            vi = 0.99 * v0[sl] + 0.01 * gi * gi
            bc1, bc2 = 1 - 0.9 ** 3, (1 - 0.99 ** 3) ** 0.5
            pi = p0[sl] - (1e-3 / bc1) * mi / (vi.sqrt() / bc2 + 1e-8)
            assert rel(m[sl], mi) < 1e-6 and rel(v[sl], vi) < 1e-6 and rel(p[sl], pi) < 1e-6
            assert torch.equal(pb[sl], p[sl].to(torch.bfloat16))
            assert torch.count_nonzero(g[sl]).item() == 0
            out = torch.ones(N, dtype=torch.bool, device=dev)
            out[sl] = False
            assert torch.equal(p[out], p0[out]) and torch.equal(g[out], g0[out])
            assert torch.equal(m[out], m0[out]) and torch.equal(v[out], v0[out])
            assert torch.count_nonzero(pb[out].float()).item() == 0


def test_reduce_slabs_multi_bit_identical(K):
    """Batched parameter-gradient reductions (kernels.reduce_param_partials, one launch for many
    jobs, 32+ jobs split over launches): bit-identical to one ctclip_reduce_slabs per job."""
    from ctclip_mi355x import _lib
    torch.manual_seed(7)
    jobs, refs = [], []
    for i in range(40):
        nb, D = (1024, 512) if i % 3 == 0 else ((2048, 32) if i % 3 == 1 else (64, 768))
        part = torch.randn(nb, D, device='cuda')
        out = torch.randn(D, device='cuda')
        ref = out.clone()
        K.reduce_slabs(part.view(nb, 1, D), ref.view(1, D), accumulate=bool(i % 2))
        jobs.append((part, out, bool(i % 2)))
        refs.append(ref)
    arr = (_lib.SlabJob * len(jobs))()
    for i, (part, out, acc) in enumerate(jobs):
        arr[i].slabs, arr[i].nslab, arr[i].cols = part.data_ptr(), part.shape[0], part.shape[1]
        arr[i].out, arr[i].accumulate = out.data_ptr(), int(acc)
    assert _lib.lib().ctclip_reduce_slabs_multi(arr, len(jobs), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    for (_, out, _), ref in zip(jobs, refs):
        assert torch.equal(out, ref)


def test_deferred_reductions_shared_output(K):
    """Two queued reductions into the SAME output (a parameter used twice in one pass):
    flush_reductions splits them over successive launches so neither update is lost, and the C-ABI
    refuses one call holding both."""
    from ctclip_mi355x import _lib
    torch.manual_seed(9)
    out = torch.randn(512, device='cuda')
    p1, p2 = torch.randn(64, 512, device='cuda'), torch.randn(96, 512, device='cuda')
    ref = out.clone()
    K.reduce_slabs(p1.view(64, 1, 512), ref.view(1, 512), accumulate=True)
    K.reduce_slabs(p2.view(96, 1, 512), ref.view(1, 512), accumulate=True)
    st = torch.cuda.current_stream()
    K._DEFERRED[st.cuda_stream] = (st, [(p1, out, True), (p2, out, True)])
    K.flush_reductions()
    torch.cuda.synchronize()
    assert torch.equal(out, ref)
    arr = (_lib.SlabJob * 2)()
    for i, p in enumerate((p1, p2)):
        arr[i].slabs, arr[i].nslab, arr[i].cols = p.data_ptr(), p.shape[0], 512
        arr[i].out, arr[i].accumulate = out.data_ptr(), 1
    assert _lib.lib().ctclip_reduce_slabs_multi(arr, 2, st.cuda_stream) == 1001


def test_attention_fwd_query_blocks_bit_identical(K):
    """The spatial forward kernel processing 1, 2 or 3 query blocks per wave together
    (ctclip_attn_set_fwd_qb) gives bit-identical outputs and LSE at the base 24 x 24 grid; the
    static-bound softmax (ctclip_attn_set_fwd_smax) matches the online max to rounding, and falls
    back to it (bit-identical) where the bound's span is too wide."""
    from ctclip_mi355x import _lib
    torch.manual_seed(5)
    gh = gw = 24
    L, H, D, nseq = gh * gw, 8, 32, 5
    M = nseq * L
    u, _ = _cpb_table(H, gh, gw)
    q = F.normalize(torch.randn(M, H, D, device=dev), dim=-1).reshape(M, H * D).bfloat16()
    kv = (torch.randn(M, 2 * H * D, device=dev) * 0.18).bfloat16()
    lib = _lib.lib()

    def run(qv):
        return K.attn_fwd(qv, kv[:, :H * D], kv[:, H * D:], L=L, H=H, D=D, nseq=nseq, scale=8.0,
                          seq=(1, L, 0, 1), bias_u=u, grid=(gh, gw))
    outs = []
    old, old_s = lib.ctclip_attn_set_fwd_qb(1), lib.ctclip_attn_set_fwd_smax(0)
    old_c = lib.ctclip_attn_set_fwd_cinit(0)     # the round-5 score chain: bit-identical across QB
    try:
        for qb in (1, 2, 3):
            lib.ctclip_attn_set_fwd_qb(qb)
            outs.append(run(q))
        for o, lse in outs[1:]:
            assert torch.equal(o, outs[0][0]) and torch.equal(lse, outs[0][1])
        # static-bound softmax (3 blocks): the same softmax, f32-level rounding differences only
        lib.ctclip_attn_set_fwd_smax(1)
        o_s, lse_s = run(q)
        assert rel(o_s, outs[0][0]) < 6e-3 and (lse_s - outs[0][1]).abs().max().item() < 1e-4   # bf16 o: 1-ulp flips
        # query norms large enough that the bound's span exceeds 64: the kernel keeps the online max
        # for those groups (bit-identical to the online kernel)
        q3 = (q.float() * 3).bfloat16()
        lib.ctclip_attn_set_fwd_smax(0)
        o_ref3 = run(q3)
        lib.ctclip_attn_set_fwd_smax(1)
        o_s3 = run(q3)
        assert torch.equal(o_s3[0], o_ref3[0]) and torch.equal(o_s3[1], o_ref3[1])
    finally:
        lib.ctclip_attn_set_fwd_qb(old)
        lib.ctclip_attn_set_fwd_smax(old_s)
        lib.ctclip_attn_set_fwd_cinit(old_c)


@pytest.mark.parametrize('gh', [24, 8])
def test_attention_fwd_cinit(K, gh):
    """The C-init spatial forward (round 6: bias as the MFMA accumulator input from the reversed
    1/scale table, one fma + exp2 per score, row sums by an all-ones MFMA over the bf16 P) against the
    round-5 chain and the f64 reference: O within bf16 rounding of the old kernel, closer or as close
    to the reference; the LSE within 2e-3 (the sum of the bf16-rounded P the PV product uses)."""
    from ctclip_mi355x import _lib
    torch.manual_seed(6)
    L, H, D, nseq = gh * gh, 8, 32, 4
    M = nseq * L
    u, bins = _cpb_table(H, gh, gh)
    q = F.normalize(torch.randn(M, H, D, device=dev), dim=-1).reshape(M, H * D).bfloat16()
    kv = torch.randn(M, 2 * H * D, device=dev)
    kv[:, :H * D] = F.normalize(kv[:, :H * D].reshape(M, H, D), dim=-1).reshape(M, H * D)
    kv = kv.bfloat16()
    lib = _lib.lib()
    args = dict(L=L, H=H, D=D, nseq=nseq, scale=8.0, seq=(1, L, 0, 1), bias_u=u, grid=(gh, gh))
    old = lib.ctclip_attn_set_fwd_cinit(0)
    try:
        o0, lse0 = K.attn_fwd(q, kv[:, :H * D], kv[:, H * D:], **args)
        lib.ctclip_attn_set_fwd_cinit(1)
        o1, lse1 = K.attn_fwd(q, kv[:, :H * D], kv[:, H * D:], **args)
    finally:
        lib.ctclip_attn_set_fwd_cinit(old)
    rows = _gather_rows(1, L, 0, 1, nseq, L)
    ref = _attn_ref(q.double(), kv[:, :H * D].double(), kv[:, H * D:].double(), rows, H, D, 8.0,
                    u[:, bins].double())
    e0, e1 = rel(o0, ref), rel(o1, ref)
    dl = (lse1 - lse0).abs().max().item()
    print(f'cinit {gh}x{gh}: O rel vs f64 {e1:.3e} (round-5 chain {e0:.3e}), |dLSE| max {dl:.2e}')
    assert rel(o1, o0) < 6e-3 and e1 < 1.1 * e0 + 1e-4 and dl < 2e-3
