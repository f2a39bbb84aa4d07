"""Every kernel that computes or consumes per-row LayerNorm statistics, on the hard row families of
ln_rows_common (large offsets, constant rows, outlier columns, tiny / large scale, block steps, single
spikes), against float64 on the bits the kernel reads.  Every assertion is per row and per element
under the bounds derived in ln_rows_common's docstring from each kernel's summation order; a failure
names the family, the row and the column.  The families are interleaved (every 8 consecutive rows hold
all of them), so no wave, row group or GEMM strip sees one family only.

Kernels: norm.hip ln_fwd / ln_bwd (every CPL the host switch instantiates: D = 64, 512 -> CPL 1,
768 -> 2, 4000 -> 8 forward only), patch.hip (strip, gather and f32 bodies, fp16 / x3 copies),
peg.hip group partials + ln_stats_merge (64- and 32-channel groups), gemm256.hip EP_LN_FWD / EP_LN_BWD
(the exchange between the two workgroups of a row block) and EP_TR_QKV_LNFOLD.

The largest error / bound ratio per (kernel, family) is printed when the module ends."""
import functools

import pytest
import torch

import ln_rows_common as C

pytestmark = pytest.mark.gpu
dev = 'cuda'
RATIOS = {}
F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16


@pytest.fixture(scope='module')
def K():
    from ctclip_mi355x import kernels
    prev = kernels.LN_FUSED_BWD
    kernels.LN_FUSED_BWD = True      # the fused backward form is opt-in in the model
    kernels.reset_ln_status()
    yield kernels
    kernels.LN_FUSED_BWD = prev
    kernels.reset_ln_status()
    print('\nlargest error / bound per (kernel, family):\n' + C.format_ratios(RATIOS))


@functools.lru_cache(maxsize=None)
def _rows(D, seed, dtype, rows):
    x, labels = C.hard_rows(D, seed=seed, dtype=dtype, rows=rows)
    return x.to(dev), labels


@functools.lru_cache(maxsize=None)
def _params(D, seed):
    g = torch.Generator().manual_seed(77 + seed)
    return (1 + 0.2 * torch.randn(D, generator=g)).to(dev), (0.1 * torch.randn(D, generator=g)).to(dev)


def _randn(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale).to(dev)


def _status(K):
    return int(K.status_word(torch.device(dev, torch.cuda.current_device())).item())


def _check_stats(what, mean, rstd, x, eps, b, labels):
    _, mr, _, rr = C.ln_ref(x, None, None, eps)
    C.check(f'{what} mean', mean, mr, b['mean'], labels, RATIOS)
    C.check(f'{what} rstd', rstd.double() / rr - 1, torch.zeros_like(rr), b['rstd'], labels, RATIOS)


# ----------------------------------------------------------------------------- norm.hip
@pytest.mark.parametrize('bias', [False, True])
@pytest.mark.parametrize('eps', [1e-5, 1e-12])
@pytest.mark.parametrize('xdt', [F32, BF16])
@pytest.mark.parametrize('D', [64, 512, 768, 4000])
def test_layernorm_fwd(K, D, xdt, eps, bias):
    """R = 67 rows (a ragged last wave group at every RPW); the two eps use different seeds, which
    rotates the variants: together they place the outlier at every listed column."""
    x, labels = _rows(D, 0 if eps == 1e-5 else 5, xdt, 67)
    gamma, beta = _params(D, 0)
    beta = beta if bias else None
    K.reset_ln_status()
    yb, yf, mean, rstd, (yh, yl) = K.layernorm_fwd(x.to(xdt), gamma, beta, eps, out_f32=True, out_x3=True)
    torch.cuda.synchronize()
    yr = C.ln_ref(x, gamma, beta, eps)[0]
    b = C.fwd_bounds(x, gamma, beta, eps, C.depth_ln(D))
    C.check('layernorm_fwd yf', yf, yr, b['y'], labels, RATIOS)
    _check_stats('layernorm_fwd', mean, rstd, x, eps, b, labels)
    C.check('layernorm_fwd yb', yb.float(), yr, b['y'] + C.out16_slack(yr.abs() + b['y'], BF16), labels, RATIOS)
    C.check('layernorm_fwd y16', yh.float(), yr, b['y'] + C.out16_slack(yr.abs() + b['y'], F16), labels, RATIOS)
    C.check('layernorm_fwd x3', yh.double() + yl.double(), yf, C.x3_slack(yf), labels, RATIOS)
    assert _status(K) == 0, 'CT_STATUS_F16_RANGE (or another status bit) set by finite, normalised rows'
    K.reset_ln_status()


@pytest.mark.parametrize('bias', [False, True])
@pytest.mark.parametrize('eps', [1e-5, 1e-12])
@pytest.mark.parametrize('dyt', [F32, BF16])
@pytest.mark.parametrize('xdt', [F32, BF16])
@pytest.mark.parametrize('D', [64, 512, 768])
def test_layernorm_bwd(K, D, xdt, dyt, eps, bias):
    x, labels = _rows(D, 0 if eps == 1e-5 else 5, xdt, 67)
    gamma, _ = _params(D, 0)
    _, _, mean, rstd = K.layernorm_fwd(x.to(xdt), gamma, None, eps)        # the kernel's own statistics
    dy = _randn((67, D), 31, 0.1).to(dyt)
    dres = _randn((67, D), 32)
    dxf, dxb, dg, db = K.layernorm_bwd(dy, x.to(xdt), mean, rstd, gamma, dres=dres, want_beta=bias)
    torch.cuda.synchronize()
    dx_ref, dg_ref, db_ref = C.ln_bwd_ref(dy, x, mean, rstd, gamma, dres)
    bx, bg, bb = C.bwd_bounds(dy, x, mean, rstd, gamma, dx_ref, C.depth_ln(D))
    C.check('layernorm_bwd dx', dxf, dx_ref, bx, labels, RATIOS)
    C.check('layernorm_bwd dxb', dxb.float(), dx_ref, bx + C.out16_slack(dx_ref.abs() + bx, BF16), labels, RATIOS)
    C.check_cols('layernorm_bwd dgamma', dg, dg_ref, bg, RATIOS)
    if bias:
        C.check_cols('layernorm_bwd dbeta', db, db_ref, bb, RATIOS)
    else:
        assert db is None


# ----------------------------------------------------------------------------- patch.hip
_PATTERNS = ('pad', 'clip', 'split_t', 'split_h', 'split_w', 'voxel_first', 'voxel_last', 'ramp', 'base')


def _patch(name, g):
    p = torch.full((10, 20, 20), 40, dtype=torch.int64)
    if name == 'pad':
        p[:] = -1000
    elif name == 'clip':
        p[:] = 1500                       # above the clip: 1.0 after the clamp
    elif name == 'split_t':
        p[:5] = -1000
    elif name == 'split_h':
        p[:, :10] = -1000
    elif name == 'split_w':
        p[:, :, :10] = -1000
    elif name == 'voxel_first':
        p[0, 0, 0] = -1000
    elif name == 'voxel_last':
        p[-1, -1, -1] = 400
    elif name == 'ramp':
        p = torch.linspace(-1200, 1200, 4000).round().long().view(10, 20, 20)
    else:
        p = torch.randint(-1200, 1201, (10, 20, 20), generator=g)
    return p


@functools.lru_cache(maxsize=None)
def _patch_volume(size, rot, ch):
    """int16 HU (1, ch, 20 / ch, size, size), PT = 10 / ch (pd = 4000 either way), whose patch k (token
    order t, hg, wg) holds pattern (k + rot) in its (c pt p1 p2) element order."""
    g = torch.Generator().manual_seed(size + rot)
    n, pt = size // 20, 10 // ch
    hu = torch.empty(1, ch, 2 * pt, size, size, dtype=torch.int64)
    labels = []
    k = 0
    for t in range(2):
        for hg in range(n):
            for wg in range(n):
                name = _PATTERNS[(k + rot) % len(_PATTERNS)]
                hu[0, :, t * pt:(t + 1) * pt, hg * 20:(hg + 1) * 20, wg * 20:(wg + 1) * 20] = \
                    _patch(name, g).view(ch, pt, 20, 20)
                labels.append(f'{name}:{k}')
                k += 1
    return hu.to(torch.int16), labels


@pytest.mark.parametrize('f32', [False, True])
@pytest.mark.parametrize('size,rot,ch', [(40, 0, 1),     # strip20 body (ragged 2-patch group), patterns 0 .. 7
                                         (40, 8, 1),     # ... the same 8 patches starting at `base`
                                         (100, 0, 1),    # Wg = 5, 50 patches: int16 -> gather body (a ragged
                                                         # group of 20 int16 is no 16-B multiple); f32 -> strip20
                                         (40, 4, 2)])    # two channels, PT = 5: gather body, int16 AND f32
def test_patch_ln(K, size, rot, ch, f32):
    """A constant patch's float64 LayerNorm is exactly 0 (beta with the affine), so on the pad / clip
    patches the assertion bounds the deviation from that by the formula's first term alone.
    Bodies reached: patch_ln_strip20_kernel<false / true>, patch_ln_kernel with int16 and with f32 input
    (a single-channel f32 volume with P = 20 always meets the strip condition, so the f32 gather needs the
    two-channel volume), and f32path.hip's patch_ln_f32.  The general patch_ln_strip_kernel (P != 20) is
    not reached: every shape here has the model's P = 20."""
    from ctclip_mi355x import layers
    hu, labels = _patch_volume(size, rot, ch)
    pt = 10 // ch
    v = hu.float().clamp(-1000, 1000) / 1000            # the f32 values the kernel normalises (exact division)
    vid = (v if f32 else hu).to(dev)
    offs = layers.patch_offsets(ch, pt, 20, 2 * pt, size, size).to(dev)
    n = size // 20
    x = v.reshape(1, ch, 2, pt, n, 20, n, 20).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(-1, 4000).to(dev)
    if size == 100:
        assert set(C.family_of(l) for l in labels) == set(_PATTERNS)
    yr = C.ln_ref(x, None, None, 1e-5)[0]
    b = C.fwd_bounds(x, None, None, 1e-5, C.depth_patch(4000))
    xb, (hi, lo) = K.patch_ln(vid, not f32, pt, 20, offs, want_x3=True)
    xb2, h2 = K.patch_ln(vid, not f32, pt, 20, offs, want_f16=True)
    torch.cuda.synchronize()
    assert torch.equal(xb2, xb) and torch.equal(h2, hi)
    C.check('patch_ln bf16', xb.float(), yr, b['y'] + C.out16_slack(yr.abs() + b['y'], BF16), labels, RATIOS)
    C.check('patch_ln f16', hi.float(), yr, b['y'] + C.out16_slack(yr.abs() + b['y'], F16), labels, RATIOS)
    C.check('patch_ln x3', hi.double() + lo.double(), yr, b['y'] + C.x3_slack(yr.abs() + b['y']), labels, RATIOS)
    gamma, beta = _params(4000, 1)
    ya = K.patch_ln_f32(vid, not f32, pt, 20, offs, gamma, beta)
    torch.cuda.synchronize()
    ba = C.fwd_bounds(x, gamma, beta, 1e-5, C.depth_patch(4000))
    C.check('patch_ln_f32', ya, C.ln_ref(x, gamma, beta, 1e-5)[0], ba['y'], labels, RATIOS)


# ----------------------------------------------------------------------------- peg.hip + ln_stats_merge
def _peg_weights(D, xf):
    """Conv weights under which every output row keeps its input's family.  The families are interleaved
    token by token, so a const or tiny row has `large` and `offset` neighbours: a weight of 1e-3 would
    leak 0.2 - 0.5 of per-channel noise into it.  The taps are scaled so that the whole conv term, 27
    products of at most max|w| max|x|, stays below 2^-27, a quarter ulp of the smallest const value
    (0.3371, ulp 2^-25): out = fl(x + conv) is then x itself on const rows and x to one rounding
    elsewhere.  No bias: a per-channel bias would break a const row as well."""
    w0 = _randn((D, 1, 3, 3, 3), 41)
    s = 2.0 ** -27 / (27 * w0.abs().max().item() * xf.abs().max().item())
    return (w0 * s).contiguous(), torch.zeros(D, device=dev)


def _assert_rows_keep_family(outf, xf, labels, eps=1e-5):
    """On the kernel's own f32 output: every element is its input to one rounding plus the conv term's
    2^-27; const rows still have var <= 4 u^2 x^2 and tiny rows var << eps."""
    assert ((outf.double() - xf.double()).abs() <= C.U * xf.double().abs() + 2.0 ** -27).all()
    var = outf.double().var(1, unbiased=False)
    seen = set()
    for i, l in enumerate(labels):
        f = C.family_of(l)
        if f == 'const':
            assert var[i].item() <= 4 * C.U ** 2 * xf[i, 0].item() ** 2, (l, i, var[i].item())
            seen.add(f)
        elif f == 'tiny':
            assert var[i].item() < 1e-2 * eps, (l, i, var[i].item())
            seen.add(f)
        elif f == 'spike':
            assert (outf[i].abs() > 2.0 ** -26).sum().item() == 1, (l, i)
            seen.add(f)
    assert seen == {'const', 'tiny', 'spike'}


@pytest.mark.parametrize('form', ['stats', 'x32'])
@pytest.mark.parametrize('mode', [0, 1])
@pytest.mark.parametrize('shape,D', [((2, 6, 5, 7), 128), ((1, 4, 4, 4), 512)])
def test_peg_stats(K, shape, D, mode, form):
    """The statistics against float64 of the kernel's own f32 output rows: the group partials and
    ln_stats_merge alone.  The conv term is scaled below the rows' own rounding (_peg_weights), and the
    test asserts on the kernel's output that const rows reach the partials with var = 0 and tiny rows
    with var << eps: the rstd = eps^-1/2 case."""
    M = shape[0] * shape[1] * shape[2] * shape[3]
    xf, labels = _rows(D, 2, F32, M)
    w, bias = _peg_weights(D, xf)
    if form == 'stats':
        outf, _, mean, rstd = K.peg_fwd_stats(xf.bfloat16(), xf, *shape, w, bias, mode)
        group = 64
    else:
        outf, _, _, mean, rstd = K.peg_fwd_x32(xf, *shape, w, bias, mode, stats=True)
        group = 32
    torch.cuda.synchronize()
    assert mean is not None and rstd is not None
    _assert_rows_keep_family(outf, xf, labels)
    b = C.fwd_bounds(outf, None, None, 1e-5, C.depth_peg(D, group), merged=True)
    _check_stats(f'peg_{form}', mean, rstd, outf, 1e-5, b, labels)


# ----------------------------------------------------------------------------- gemm256.hip EP_LN_FWD / BWD
@pytest.mark.parametrize('dt', [BF16, F16])
def test_linear_residual_ln(K, dt):
    """M = 2048, K = 256, N = 512: the hard rows are the f32 residual, the GEMM term 1e-2 of each row's
    rms.  step:256 rows have their whole variance in the term exchanged between the two workgroups."""
    M, Kd = 2048, 256
    res, labels = _rows(512, 0, F32, M)
    gamma, beta = _params(512, 2)
    scale = 2e-2 * res.pow(2).mean(1, keepdim=True).sqrt()
    o = (_randn((M, Kd), 51, 0.5) * scale).to(dt)
    W = _randn((512, Kd), 52, Kd ** -0.5).to(dt)
    K.reset_ln_status()
    with K.ln_guard():
        out = K.linear_residual_ln(o, W, res, gamma, beta, 1e-5, y16=dt == F16)
    assert out is not None, 'fused form refused at a fusable shape'
    torch.cuda.synchronize()
    x1f, x1b, y, mean, rstd = out[:5]
    x1_ref = res.double() + o.double() @ W.double().t()
    C.check('linear_residual_ln x1', x1f, x1_ref, C.dot_bound(o, W, x1_ref), labels, RATIOS)
    assert torch.equal(x1b, x1f.bfloat16())
    yr = C.ln_ref(x1f, gamma, beta, 1e-5)[0]                        # of the kernel's own x1
    b = C.fwd_bounds(x1f, gamma, beta, 1e-5, C.DEPTH_GEMM_LN, merged=True)
    _check_stats('linear_residual_ln', mean, rstd, x1f, 1e-5, b, labels)
    C.check('linear_residual_ln y', y.float(), yr, b['y'] + C.out16_slack(yr.abs() + b['y'], BF16), labels, RATIOS)
    if dt == F16:
        C.check('linear_residual_ln y16', out[5].float(), yr, b['y'] + C.out16_slack(yr.abs() + b['y'], F16),
                labels, RATIOS)
    assert K.ln_fused_status() == 0
    K.reset_ln_status()


def test_matmul_nn_ln_bwd(K):
    """M = 2048, N = 256.  The kernel normalises with dy = bf16(its own f32 product); the reference is the
    float64 product, and that rounding (2^-8 |dy| + the accumulation bound) is propagated per element."""
    M, N = 2048, 256
    x, labels = _rows(512, 0, BF16, M)
    gamma, _ = _params(512, 2)
    xb = x.bfloat16()
    _, _, mean, rstd = K.layernorm_fwd(xb, gamma, None, 1e-5)
    dy = _randn((M, N), 61, 0.1).bfloat16()
    W = _randn((N, 512), 62, N ** -0.5).bfloat16()
    dres = _randn((M, 512), 63)
    dg = torch.zeros(512, device=dev)
    db = torch.zeros(512, device=dev)
    K.reset_ln_status()
    with K.ln_guard():
        out = K.matmul_nn_ln_bwd(dy, W, xb, mean, rstd, gamma, dres, dgamma_out=dg, dbeta_out=db)
    assert out is not None, 'fused form refused at a fusable shape'
    K.flush_reductions()
    torch.cuda.synchronize()
    dxf, dxb = out
    dyl = dy.double() @ W.double()
    ddy = C.BF16_U * dyl.abs() + C.dot_bound(dy, W.t().contiguous())
    dx_ref, dg_ref, db_ref = C.ln_bwd_ref(dyl, x, mean, rstd, gamma, dres)
    bx, bg, bb = C.bwd_bounds(dyl, x, mean, rstd, gamma, dx_ref, C.DEPTH_GEMM_LN, ddy=ddy)
    C.check('matmul_nn_ln_bwd dx', dxf, dx_ref, bx, labels, RATIOS)
    assert torch.equal(dxb, dxf.bfloat16())
    C.check_cols('matmul_nn_ln_bwd dgamma', dg, dg_ref, bg, RATIOS)
    C.check_cols('matmul_nn_ln_bwd dbeta', db, db_ref, bb, RATIOS)
    assert K.ln_fused_status() == 0
    K.reset_ln_status()


# ----------------------------------------------------------------------------- EP_TR_QKV_LNFOLD
@pytest.mark.parametrize('stats,M', [('exact', 512), ('exact', 331), ('peg', 512)])
def test_qkv_lnfold(K, stats, M):
    """K = 512, nq = 256.  ctclip_gemm_qkv_lnfold2 requires only M > 0: M = 331 = 8 * 41 + 3 is one full
    256-row tile and a ragged one (the epilogue reads mean / rstd of clamped rows there and must store
    nothing past row M), M = 512 two full tiles (the PEG grid 1 x 8 x 8 x 8).
    The fold computes rstd (x . w' - mean cs): beyond |mean| / sigma = 2^16 / K^1.5 = 5.7 (ln_rows_common:
    where rstd K u |mean| sum|w'| passes 2^-8 |q| with sum|w'| <= sqrt(K) ||w'||) its cancellation, not
    the bf16 rounding of the output, sets the error bound -- all of `offset`, `const` and `step`.
    exact: mean / rstd are the f32 rounding of the float64 statistics of the bf16 rows; the reference is
    the float64 LayerNorm.  peg: x, mean, rstd as the model feeds them (peg_fwd_stats: bf16 rows, the
    statistics of their f32 originals, the conv term below the rows' rounding so that const rows arrive
    with var = 0 and rstd = eps^-1/2); the reference normalises the bf16 rows with those statistics."""
    Kd, nq = 512, 256
    gamma, _ = _params(512, 3)
    Wq = _randn((nq, Kd), 71, Kd ** -0.5)
    Wkv = _randn((512, Kd), 72, Kd ** -0.5).bfloat16()
    qs, ks = 1 + _randn((32,), 73, 0.1), 1 + _randn((32,), 74, 0.1)
    if stats == 'exact':
        x, labels = _rows(512, 0, BF16, M)
        _, m64, _, r64 = C.ln_ref(x, None, None, 1e-5)
        mean, rstd = m64.float(), r64.float()
        xhat = (x.double() - m64[:, None]) * r64[:, None]
    else:
        xf, labels = _rows(512, 0, F32, M)
        w, bias = _peg_weights(512, xf)
        of, ob, mean, rstd = K.peg_fwd_stats(xf.bfloat16(), xf, 1, 8, 8, 8, w, bias, 0)
        _assert_rows_keep_family(of, xf, labels)
        x = ob.float()
        xhat = (x.double() - mean.double()[:, None]) * rstd.double()[:, None]
    Wp, cs, scales = K.pack_qkv_fold(Wq, gamma, Wkv, qs, ks)
    wf = Wp[:nq]
    assert torch.equal(wf, (Wq * gamma).bfloat16()) and torch.equal(Wp[nq:], Wkv)
    # guard rows behind the outputs: a ragged last tile must not store past row M
    out = torch.full((M + 8, 768), 7.0, device=dev, dtype=BF16)
    out2 = torch.full((M + 8, 512), 7.0, device=dev, dtype=BF16)
    qkv, _ = K.linear_qkv_lnfold(x.bfloat16(), Wp, cs, mean, rstd, scales, nq, 512, out=out[:M], out2=out2[:M])
    torch.cuda.synchronize()
    assert (out[M:] == 7.0).all() and (out2[M:] == 7.0).all(), 'stored past row M'
    q_ref = xhat @ wf.double().t()
    C.check(f'qkv_lnfold[{stats} {M}] q', qkv[:, :nq].float(), q_ref, C.fold_bound(x, wf, mean, rstd, q_ref), labels,
            RATIOS)
    kv_ref = x.double() @ Wkv.double().t()
    bkv = C.dot_bound(x, Wkv)
    C.check(f'qkv_lnfold[{stats} {M}] kv', qkv[:, nq:].float(), kv_ref, bkv + C.out16_slack(kv_ref.abs() + bkv, BF16),
            labels, RATIOS)
