"""Shared helpers of the LayerNorm row-statistics tests (a plain module, imported by
test_ln_rows_cpu.py and test_gpu_ln_rows.py): hard row families, float64 references and per-element
error bounds derived from each kernel's own summation order.

Row families (``hard_rows``)
    base     randn (control)
    offset   randn * s + m with |m| / s in {10, 100, 1000}, both signs
    const    one value in every column: -1.0 (its D-fold sum is exact in f32) and 0.3371 (it is not)
    outlier  randn plus one column at 200 sigma, at columns 0, D-1, 7|8 (lane chunk), 255|256 (GEMM
             tile halves), 31|32 and 63|64 (PEG channel groups)
    tiny     sigma = 1e-4: var << 1e-5, and with eps = 1e-12 BERT's case
    large    sigma = 1e3
    step     +a / -a in alternating blocks of c columns, c in {8, 32, 64, 256, 16, 128}, plus
             randn * 1e-3 a: the block means differ by 2a and the Chan d^2 term of the level that
             merges c-column groups carries the whole variance
    spike    exactly one non-zero column
Row i has family ``families[i % len(families)]`` and variant ``(i // len(families) + seed)``
modulo the family's variant count, so every block of len(families) consecutive rows (8 by default:
every wave, RPW group and GEMM row chunk) holds every family and different seeds rotate the variants.

Bounds.  u = 2^-24 is the f32 unit roundoff; a sum in which no element passes through more than
``depth`` additions has |fl(sum) - sum| <= depth u sum|x_i| (Higham, Accuracy and Stability,
(4.4), gamma_n ~ n u), whatever the order.  The depths follow from the code:
    norm.hip ln_fwd / ln_bwd   a lane adds its CPL = ceil(D / 512) chunks of 8 in sequence, then
                               the 6-level xor tree of the wave:          depth = 8 CPL + 6
    patch.hip                  a lane adds ceil(pd / 64) elements in sequence (gather form; the strip
                               forms add 32 pairs), then the wave tree:   depth = ceil(pd / 64) + 6
    gemm256.hip EP_LN_FWD/BWD  8 sequential adds per lane, then 6 pairwise levels (3 across lanes,
                               2 across wave columns, 1 across the two tiles):  depth = 8 + 6
    peg.hip + ln_stats_merge   8 (4) sequential adds and a 3-level tree per 64 (32)-channel group,
                               then ng = D / 64 (D / 32) sequential adds:  depth = 11 + ng (7 + ng)
With A = sum|x_i| / D, X = max|x_i|, v = var(x) (biased), w = v + eps, r = w^-1/2 (all float64 of
the bits the kernel reads):

  mean (absolute)    dm = (depth + 2) u A            (+1 for 1 / D, +1 for the product with it)
  two-pass variance  the kernel sums fl((x - m^)^2); sum (x - m^)^2 = D (v + (m^ - m)^2) exactly, the
                     mean error enters SQUARED:
                     dw = dm^2 + (depth + 6) u (v + dm^2 + eps)
  merged (mean, M2)  (Chan et al.; EP_LN_FWD, ln_stats_merge): the between-group terms n/2 d^2 use
                     differences of computed group means, each off by at most E = (depth + 2) u X,
                     so the error is LINEAR in E (Cauchy-Schwarz over the groups):
                     dw = 4 E sqrt(v) + 5 E^2 + (depth + 8) u (v + eps)
  rstd (relative)    the computed w^ lies in [max(w - dw, eps (1 - u)), w + dw] (the computed variance
                     is a sum of squares, never negative), so
                     rho = max(sqrt(w / lo) - 1, 1 - sqrt(w / hi)) + 4 u
                     (4 u: rsqrtf within 2 ulp; no first-order expansion, dw may exceed w on const rows)
  y_j                y = (x - m^) r^ g_j + b_j: one subtraction, two products, one sum:
                     dy_j = |g_j| r (1 + rho) dm + |y_j - b_j| (rho + 4 u) + u |y_j|
                     (a const row has y_j - b_j = 0 and v = 0: only the first term is left, r = eps^-1/2
                     times the rounding of the mean)
  16-bit outputs     + 2^-8 |y| (bf16), + 2^-11 |y| + 2^-25 (fp16, subnormal spacing 2^-24); the
                     split-fp16 pair hi + lo against the f32 value: 2^-22 |y| + 2^-25

  backward           dx = r (g - s1 - xh s2) + dres, g = dy gamma, xh = (x - mean) r on the kernel's own
                     f32 mean / rstd, s1 = mean(g), s2 = mean(g xh):
                     ds1 = (depth + 3) u mean|g|,  ds2 = (depth + 6) u mean|g xh|
                     ddx_j = r (ds1 + |xh_j| ds2 + 6 u (|g_j| + |s1| + |xh_j s2|)) + u |dx_j|
                     dgamma_j = sum_r dy xh:  (R + 3) u sum_r |dy_rj xh_rj|;  dbeta_j: R u sum_r |dy_rj|
                     (R rows: the bound grows with the row count)

  fold               q^ = rs (acc - mu cs): acc the f32 accumulation of the K products x_k w'_k, cs the
                     f32 row sum of w' (depth 8 K / 512 + 6 <= 14 at K = 512), mu / rs the f32 statistics:
                     dq = rs (K u sum_k |x_k w'_k| + 16 u |mu| sum_k |w'_k|) + 3 u |q| + 2^-8 |q|
                     On rows with |mean| >> sigma, sum|x_k w'_k| ~ |mean| sum|w'_k|: the first term is
                     the cancellation rs K u |mean| sum|w'_k|.  With |q| ~ ||w'||_2 and sum|w'_k| <=
                     sqrt(K) ||w'||_2 it passes the bf16 rounding 2^-8 |q| at
                     |mean| / sigma = 2^-8 / (K^1.5 u) = 2^16 / K^1.5  (5.7 at K = 512).

No constant above comes from a GPU result."""
import torch

U = 2.0 ** -24
BF16_U = 2.0 ** -8
F16_U = 2.0 ** -11
F16_SUB = 2.0 ** -25
FAMILIES = ('base', 'offset', 'const', 'outlier', 'tiny', 'large', 'step', 'spike')
STEP_CUTS = (8, 32, 64, 256, 16, 128)
OLD_NORM_TOL_BF16 = 4e-3     # the existing tests' relative Frobenius bound for 16-bit outputs


def fold_crossover(K):
    """|mean| / sigma beyond which the fold's cancellation term exceeds its bf16 output rounding."""
    return 2.0 ** 16 / K ** 1.5


def depth_ln(D):
    return 8 * ((D + 511) // 512) + 6


def depth_patch(pd):
    return (pd + 63) // 64 + 6


DEPTH_GEMM_LN = 8 + 6


def depth_peg(D, group):
    return (11 if group == 64 else 7) + D // group


def _variants(family, D):
    if family == 'offset':
        return [(10.0, 1.0), (100.0, -1.0), (1000.0, 1.0), (10.0, -1.0), (100.0, 1.0), (1000.0, -1.0)]
    if family == 'const':
        return [-1.0, 0.3371]
    if family == 'outlier':
        out = []
        for c in (0, D - 1, 7, 8, 255, 256, 31, 32, 63, 64):
            if 0 <= c < D and c not in out:
                out.append(c)
        return out
    if family == 'step':
        return [c for c in STEP_CUTS if c < D]
    if family == 'spike':
        return [(0, 1.0), (D - 1, -250.0), (8 % D, 3e-3)]
    return [None]


def hard_rows(D, families=FAMILIES, seed=0, dtype=torch.float32, rows=None):
    """([R, D] float32 CPU matrix whose values are exact in ``dtype``, [R] labels 'family:variant').
    rows: R (default: one full cycle of the family with the most variants)."""
    g = torch.Generator().manual_seed(1000 + seed)
    nf = len(families)
    if rows is None:
        rows = nf * max(len(_variants(f, D)) for f in families)
    x = torch.empty(rows, D, dtype=torch.float64)
    labels = []
    for i in range(rows):
        fam = families[i % nf]
        var = _variants(fam, D)
        v = var[(i // nf + seed) % len(var)]
        z = torch.randn(D, generator=g, dtype=torch.float64)
        if fam == 'base':
            r = z
        elif fam == 'offset':
            r = z + v[0] * v[1]
        elif fam == 'const':
            r = torch.full((D,), v, dtype=torch.float64)
        elif fam == 'outlier':
            r = z.clone()
            r[v] += 200.0
        elif fam == 'tiny':
            r = z * 1e-4
        elif fam == 'large':
            r = z * 1e3
        elif fam == 'step':
            sign = 1.0 - 2.0 * ((torch.arange(D) // v) % 2).double()
            r = 3.0 * sign + z * 3e-3
        elif fam == 'spike':
            r = torch.zeros(D, dtype=torch.float64)
            r[v[0]] = v[1]
        else:
            raise ValueError(fam)
        x[i] = r
        labels.append(f'{fam}:{v}')
    return x.float().to(dtype).float(), labels


def family_of(label):
    return label.split(':')[0]


# ----------------------------------------------------------------------------- float64 references
def ln_ref(x, gamma=None, beta=None, eps=1e-5):
    """float64 LayerNorm of the rows of x: (y, mean, var, rstd)."""
    x = x.double()
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    rstd = (var + eps).rsqrt()
    y = (x - mean[:, None]) * rstd[:, None]
    if gamma is not None:
        y = y * gamma.double()
    if beta is not None:
        y = y + beta.double()
    return y, mean, var, rstd


def ln_bwd_ref(dy, x, mean, rstd, gamma, dres=None):
    """float64 LayerNorm backward on the given (the kernel's own f32) mean / rstd: (dx, dgamma, dbeta)."""
    dy, x, mean, rstd = dy.double(), x.double(), mean.double()[:, None], rstd.double()[:, None]
    xh = (x - mean) * rstd
    g = dy * gamma.double()
    dx = rstd * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    if dres is not None:
        dx = dx + dres.double()
    return dx, (dy * xh).sum(0), dy.sum(0)


# ----------------------------------------------------------------------------- bounds
def fwd_bounds(x, gamma, beta, eps, depth, merged=False):
    """Per-row and per-element bounds of a LayerNorm forward over the rows of x (the module docstring's
    formulas).  merged: the (mean, M2) merge form.  Returns dict(mean [R] absolute, rstd [R] relative,
    y [R, D] absolute) in float64."""
    x = x.double()
    y, mean, var, rstd = ln_ref(x, gamma, beta, eps)
    A = x.abs().mean(1)
    dm = (depth + 2) * U * A
    if merged:
        E = (depth + 2) * U * x.abs().amax(1)
        dw = 4 * E * var.sqrt() + 5 * E ** 2 + (depth + 8) * U * (var + eps)
    else:
        dw = dm ** 2 + (depth + 6) * U * (var + dm ** 2 + eps)
    w = var + eps
    lo = torch.clamp(w - dw, min=eps * (1 - U))
    rho = torch.maximum((w / lo).sqrt() - 1, 1 - (w / (w + dw)).sqrt()) + 4 * U
    ag = torch.ones(x.shape[1], dtype=torch.float64, device=x.device) if gamma is None else gamma.double().abs()
    yc = y if beta is None else y - beta.double()
    yb = ag * (rstd * (1 + rho) * dm)[:, None] + yc.abs() * (rho[:, None] + 4 * U)
    yb = yb + U * (y.abs() + yb)       # the last rounding is of the computed value
    return dict(mean=dm, rstd=rho, y=yb)


def out16_slack(y, dtype):
    """Half an ulp of a 16-bit output's own value."""
    y = y.double().abs()
    if dtype == torch.bfloat16:
        return BF16_U * y
    return F16_U * y + F16_SUB


def x3_slack(y):
    return 2.0 ** -22 * y.double().abs() + F16_SUB


def bwd_bounds(dy, x, mean, rstd, gamma, dx_ref, depth, ddy=None):
    """Bounds of (dx [R, D], dgamma [D], dbeta [D]).  ddy: an additional per-element uncertainty of dy
    (the fused GEMM's bf16 rounding of its own product), propagated linearly."""
    dy, x, mean, rstd = dy.double(), x.double(), mean.double()[:, None], rstd.double()[:, None]
    R = x.shape[0]
    xh = (x - mean) * rstd
    ag = gamma.double().abs()
    g = dy * gamma.double()
    s1 = g.mean(1, keepdim=True)
    s2 = (g * xh).mean(1, keepdim=True)
    ds1 = (depth + 3) * U * g.abs().mean(1, keepdim=True)
    ds2 = (depth + 6) * U * (g * xh).abs().mean(1, keepdim=True)
    dx = rstd * (ds1 + xh.abs() * ds2 + 6 * U * (g.abs() + s1.abs() + (xh * s2).abs()))
    dx = dx + U * (dx_ref.double().abs() + dx)      # the last rounding is of the computed value
    dgam = (R + 3) * U * (dy * xh).abs().sum(0)
    dbet = R * U * dy.abs().sum(0)
    if ddy is not None:
        e = ddy.double() * ag
        dx = dx + rstd * (e + e.mean(1, keepdim=True) + xh.abs() * (e * xh.abs()).mean(1, keepdim=True))
        dgam = dgam + (ddy.double() * xh.abs()).sum(0)
        dbet = dbet + ddy.double().sum(0)
    return dx, dgam, dbet


def dot_bound(a, b, out=None):
    """|fl(a @ b^T) - a @ b^T| for an f32 accumulation of K exact products in any order: K u |a| @ |b|^T
    (+ 2 u |out| for an f32 epilogue's product and sum)."""
    K = a.shape[1]
    bd = K * U * (a.double().abs() @ b.double().abs().t())
    if out is not None:
        bd = bd + 2 * U * out.double().abs()
    return bd


def fold_bound(x, wf, mean, rstd, q_ref):
    """The folded-LayerNorm projection's bound (module docstring): x [M, K] bf16 values, wf [nq, K] the
    bf16 folded weight, mean / rstd the f32 statistics fed to the kernel, q_ref the float64 result."""
    K = x.shape[1]
    ax, aw = x.double().abs(), wf.double().abs()
    rs, mu = rstd.double()[:, None], mean.double().abs()[:, None]
    q = q_ref.double().abs()
    f32 = rs * (K * U * (ax @ aw.t()) + 16 * U * mu * aw.sum(1)[None]) + 3 * U * q
    return f32 + BF16_U * (q + f32)        # the bf16 rounding is of the computed value


# ----------------------------------------------------------------------------- per-element check
def check(what, got, ref, bound, labels, ratios=None):
    """Assert |got - ref| <= bound element-wise ([R] or [R, D]); the message names the family, row and
    column of the worst element.  Records the largest error / bound ratio per family in ``ratios``
    [(what, family)] and returns the overall largest."""
    assert got is not None, f'{what}: no output'
    got, ref, bound = got.double(), ref.double(), bound.double()
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    assert torch.isfinite(got).all(), f'{what}: non-finite output'
    assert torch.isfinite(ref).all(), f'{what}: non-finite reference'
    assert torch.isfinite(bound).all() and (bound >= 0).all(), f'{what}: bound not finite and non-negative'
    err = (got - ref).abs()
    ratio = err / bound.clamp_min(1e-300)
    ratio = torch.where(err == 0, torch.zeros_like(ratio), ratio)
    per_row = ratio.reshape(ratio.shape[0], -1).amax(1).cpu()
    fams = sorted(set(family_of(l) for l in labels))
    if ratios is not None:
        for f in fams:
            rows = [i for i, l in enumerate(labels) if family_of(l) == f]
            ratios[(what, f)] = max(ratios.get((what, f), 0.0), per_row[rows].max().item())
    worst = per_row.max().item()
    if worst > 1.0:
        i = int(per_row.argmax())
        j = int(ratio.reshape(ratio.shape[0], -1)[i].argmax())
        e = err.reshape(err.shape[0], -1)[i, j].item()
        b = bound.reshape(bound.shape[0], -1)[i, j].item()
        raise AssertionError(f'{what}: family {labels[i]} row {i} column {j}: |err| {e:.3e} > bound {b:.3e} '
                             f'(ratio {worst:.2f}; got {got.reshape(got.shape[0], -1)[i, j].item():.9g}, '
                             f'ref {ref.reshape(ref.shape[0], -1)[i, j].item():.9g})')
    return worst


def check_cols(what, got, ref, bound, ratios=None):
    """Per-column form (parameter gradients): names the column."""
    got, ref, bound = got.double(), ref.double(), bound.double()
    assert got.shape == ref.shape == bound.shape, (what, got.shape, ref.shape, bound.shape)
    assert torch.isfinite(got).all(), f'{what}: non-finite output'
    assert torch.isfinite(ref).all(), f'{what}: non-finite reference'
    assert torch.isfinite(bound).all() and (bound >= 0).all(), f'{what}: bound not finite and non-negative'
    err = (got - ref).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300))
    worst = ratio.max().item()
    if ratios is not None:
        ratios[(what, 'all')] = max(ratios.get((what, 'all'), 0.0), worst)
    if worst > 1.0:
        j = int(ratio.argmax())
        raise AssertionError(f'{what}: column {j}: |err| {err[j].item():.3e} > bound {bound[j].item():.3e} '
                             f'(ratio {worst:.2f})')
    return worst


def format_ratios(ratios):
    kernels = sorted(set(k for k, _ in ratios))
    fams = [f for f in FAMILIES + ('all',) if any((k, f) in ratios for k in kernels)]
    fams += sorted(set(f for _, f in ratios) - set(fams))
    lines = ['| kernel | ' + ' | '.join(fams) + ' |', '|---|' + '---|' * len(fams)]
    for k in kernels:
        lines.append(f'| {k} | ' + ' | '.join(f'{ratios[(k, f)]:.3f}' if (k, f) in ratios else '' for f in fams) + ' |')
    return '\n'.join(lines)


# ----------------------------------------------------------------------------- f32 restatements
def _tree64(v):
    """The wave's xor tree (offsets 32 .. 1) over the last dimension of 64 lanes, in f32."""
    for o in (32, 16, 8, 4, 2, 1):
        idx = torch.arange(64) ^ o
        v = v + v[..., idx]
    return v


def two_pass_f32(x, gamma, beta, eps):
    """f32 restatement of norm.hip ln_fwd_kernel: the row in CPL chunks of 8 per lane (column
    (c * 64 + lane) * 8 + j), a lane's sequential sum over its chunks, the wave's xor tree; then the
    same for the squared deviations.  Returns (y, mean, rstd) in f32."""
    x = x.float()
    R, D = x.shape
    cpl = (D + 511) // 512
    xp = torch.zeros(R, cpl * 512, dtype=torch.float32)
    xp[:, :D] = x
    inb = torch.zeros(cpl * 512, dtype=torch.bool)
    inb[:D] = True
    v = xp.view(R, cpl, 64, 8)
    inb = inb.view(cpl, 64, 8)
    invD = torch.tensor(1.0, dtype=torch.float32) / D
    s = torch.zeros(R, 64, dtype=torch.float32)
    for c in range(cpl):
        for j in range(8):
            s = s + v[:, c, :, j]
    mean = _tree64(s)[:, 0] * invD
    q = torch.zeros(R, 64, dtype=torch.float32)
    for c in range(cpl):
        for j in range(8):
            d = torch.where(inb[c, :, j], v[:, c, :, j] - mean[:, None], torch.zeros(()))
            q = q + d * d
    rstd = torch.rsqrt(_tree64(q)[:, 0] * invD + torch.tensor(eps, dtype=torch.float32))
    y = (x - mean[:, None]) * rstd[:, None]
    if gamma is not None:
        y = y * gamma.float()
    if beta is not None:
        y = y + beta.float()
    return y, mean, rstd


def one_pass_f32(x, gamma, beta, eps):
    """f32 one-pass E[x^2] - E[x]^2 (what none of the kernels may do)."""
    x = x.float()
    D = x.shape[1]
    mean = x.sum(1) / D
    var = ((x * x).sum(1) / D - mean * mean).clamp_min(0)
    rstd = torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32))
    y = (x - mean[:, None]) * rstd[:, None]
    if gamma is not None:
        y = y * gamma.float()
    if beta is not None:
        y = y + beta.float()
    return y, mean, rstd


def chan_f32(x, gamma, beta, eps, bad_level=None, fault=None):
    """f32 restatement of gemm256.hip EP_LN_FWD: a two-pass (mean, M2) per 8 columns, then pairwise
    equal-count merges of neighbours (levels 0 .. log2(D / 8) - 1; at D = 512: three across lanes, two
    across wave columns, one across the tiles).  fault at bad_level: 'count' halves that level's n / 2,
    'drop' leaves its d^2 n / 2 term out."""
    x = x.float()
    R, D = x.shape
    v = x.view(R, D // 8, 8)
    m = torch.zeros(R, D // 8, dtype=torch.float32)
    for j in range(8):
        m = m + v[:, :, j]
    m = m * 0.125
    M2 = torch.zeros_like(m)
    for j in range(8):
        d = v[:, :, j] - m
        M2 = M2 + d * d
    half_n, level = 4.0, 0
    while m.shape[1] > 1:
        a, b = m[:, 0::2], m[:, 1::2]
        d = a - b
        h = half_n
        if level == bad_level and fault == 'count':
            h = half_n / 2
        term = d * d * h
        if level == bad_level and fault == 'drop':
            term = torch.zeros_like(term)
        M2 = (M2[:, 0::2] + M2[:, 1::2]) + term
        m = 0.5 * (a + b)
        half_n *= 2
        level += 1
    mean = m[:, 0]
    rstd = torch.rsqrt(M2[:, 0] * (torch.tensor(1.0, dtype=torch.float32) / D) + torch.tensor(eps, dtype=torch.float32))
    y = (x - mean[:, None]) * rstd[:, None]
    if gamma is not None:
        y = y * gamma.float()
    if beta is not None:
        y = y + beta.float()
    return y, mean, rstd
