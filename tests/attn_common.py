"""Shared helpers of the attention tests (a plain module, imported by test_gpu_ops.py,
test_gpu_attn_plan.py and test_attn_compare_cpu.py): the sequence gather, the softmax-attention
reference in any float type, the CPB bin table, a float64 reference of every output of the forward
and backward C ABI, a torch emulation of a bf16 attention pipeline (the yardstick for the tolerance),
and the block-scaled comparison."""
import torch

dev = 'cuda'


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _gather_rows(n_inner, s_outer, s_inner, s_pos, nseq, L, device=dev):
    s = torch.arange(nseq)[:, None]
    i = torch.arange(L)[None, :]
    return ((s // n_inner) * s_outer + (s % n_inner) * s_inner + i * s_pos).to(device)


def _heads(t, rows, H, D):
    """[M, >= H*D] canonical rows -> [nseq, H, L, D]"""
    nseq, L = rows.shape
    return t[rows.reshape(-1)][:, :H * D].reshape(nseq, L, H, D).permute(0, 2, 1, 3)


def _scatter(x, rows, M):
    """[nseq, H, L, D] -> [M, H*D] canonical rows (zero elsewhere)"""
    nseq, H, L, D = x.shape
    out = torch.zeros(M, H * D, device=x.device, dtype=x.dtype)
    return out.index_copy(0, rows.reshape(-1), x.permute(0, 2, 1, 3).reshape(nseq * L, H * D))


def _scatter_lse(lse, rows, M):
    """[nseq, H, L] -> [H, M], the kernels' layout"""
    nseq, H, L = lse.shape
    out = torch.zeros(H, M, device=lse.device, dtype=lse.dtype)
    return out.index_copy(1, rows.reshape(-1), lse.permute(1, 0, 2).reshape(H, nseq * L))


def _attn_ref(q, k, v, rows, H, D, scale, bias=None, kmask=None, want_lse=False, keep=None):
    """softmax(scale q.k^T + bias + mask) v in the dtype of q, k, v, on the canonical rows [M, H*D].
    bias: [H, L, L] (u[:, bins] of _cpb_table, any gh x gw grid); kmask [nseq, L] 1 = keep; keep
    [nseq, H, L, L]: the dropout multiplier of the probabilities (0 or 1 / (1 - p)).
    want_lse: also the LSE in the kernels' units and layout -- attn.hip stores the NATURAL-log
    ln(sum_k exp(scale q.k + bias + mask)) of every query (before dropout) as f32 at
    lse[h * M + row(s, i)], i.e. [H, M] indexed by the canonical token row."""
    nseq, L = rows.shape
    s = torch.einsum('shid,shjd->shij', _heads(q, rows, H, D), _heads(k, rows, H, D)) * scale
    if bias is not None:
        s = s + bias
    if kmask is not None:
        s = s.masked_fill(~kmask[:, None, None, :].bool(), float('-inf'))
    a = s.softmax(-1)
    if keep is not None:
        a = a * keep
    out = _scatter(torch.einsum('shij,shjd->shid', a, _heads(v, rows, H, D)), rows, q.shape[0])
    if want_lse:
        return out, _scatter_lse(torch.logsumexp(s, -1), rows, q.shape[0])
    return out


def _cpb_bins(gh, gw, device=dev):
    """bin(q, k) = (hq - hk + gh - 1)(2 gw - 1) + (wq - wk + gw - 1), [L, L], L = gh * gw row-major"""
    pos = torch.stack(torch.meshgrid(torch.arange(gh), torch.arange(gw), indexing='ij')).reshape(2, -1).t()
    rel_ = pos[:, None, :] - pos[None, :, :]
    return ((rel_[..., 0] + gh - 1) * (2 * gw - 1) + (rel_[..., 1] + gw - 1)).to(device)


def _cpb_table(H, gh, gw, device=dev):
    nb = (2 * gh - 1) * (2 * gw - 1)
    u = torch.randn(H, nb, device=device) * 0.5
    return u, _cpb_bins(gh, gw, device)


# --------------------------------------------------------------- float64 reference, all outputs
def attn_ref64(q, k, v, do, rows, H, D, scale, u=None, bins=None, kmask=None, keep=None):
    """float64 reference built from the exact bf16 inputs: dict of o, dq, dk, dv [M, H*D], lse [H, M]
    (natural log, see _attn_ref) and du [H, nbins], the gradient of the deduplicated bias table;
    gradients by autograd in float64."""
    qd, kd, vd = (t[:, :H * D].double().clone().requires_grad_(True) for t in (q, k, v))
    ud = u.double().clone().requires_grad_(True) if u is not None else None
    o, lse = _attn_ref(qd, kd, vd, rows, H, D, scale, ud[:, bins] if u is not None else None, kmask,
                       want_lse=True, keep=keep.double() if keep is not None else None)
    o.backward(do.double())
    return dict(o=o.detach(), lse=lse.detach(), dq=qd.grad, dk=kd.grad, dv=vd.grad,
                du=ud.grad if u is not None else None)


# ------------------------------------------------------------------- bf16 pipeline emulation
def _bf(x):
    return x.bfloat16().float()


def attn_emul_bf16(q, k, v, do, rows, H, D, scale, u=None, bins=None, kmask=None, keep=None, smask=None):
    """A plain torch emulation of a bf16 flash-attention pipeline on the same inputs, the yardstick
    the kernels are held to: f32 scores; the unnormalised P = exp(s - max) rounded to bf16 before
    P.V, the row sum taken over those bf16 values (what the C-init forward sums), O rounded to bf16;
    in the backward delta = rowsum(dO * O) from the bf16 O, P = exp(s - lse) and dS = P (dP - delta)
    in f32, both rounded to bf16 before the dV / dQ / dK products, whose results are rounded to
    bf16; dU bins the f32 dS.  smask [nseq, H, L, L] (tests of the comparison only): an extra
    additive score mask.  Same dict as attn_ref64."""
    M = q.shape[0]
    qf, kf, vf, dof = (_heads(t.float(), rows, H, D) for t in (q, k, v, do))
    s = torch.einsum('shid,shjd->shij', qf, kf) * scale
    if u is not None:
        s = s + u.float()[:, bins]
    if kmask is not None:
        s = s.masked_fill(~kmask[:, None, None, :].bool(), float('-inf'))
    if smask is not None:
        s = s + smask
    m = s.amax(-1, keepdim=True)
    e = torch.exp(s - m)
    pb = _bf(e)
    l = pb.sum(-1, keepdim=True)
    lse = m + torch.log(l)
    pv = pb if keep is None else _bf(e * keep)
    o = _bf(torch.einsum('shij,shjd->shid', pv, vf) / l)
    delta = (dof * o).sum(-1, keepdim=True)
    p = torch.exp(s - lse)
    dp = torch.einsum('shid,shjd->shij', dof, vf)
    if keep is not None:
        dp = dp * keep
    ds = p * (dp - delta)
    dsb = _bf(ds * scale)
    dv = _bf(torch.einsum('shij,shid->shjd', _bf(p if keep is None else p * keep), dof))
    dq = _bf(torch.einsum('shij,shjd->shid', dsb, kf))
    dk = _bf(torch.einsum('shij,shid->shjd', dsb, qf))
    du = None
    if u is not None:
        L = rows.shape[1]
        du = torch.zeros(H, u.shape[1], device=q.device).index_add_(1, bins.reshape(-1), ds.sum(0).reshape(H, L * L))
    return dict(o=_scatter(o, rows, M), lse=_scatter_lse(lse.squeeze(-1), rows, M), dq=_scatter(dq, rows, M),
                dk=_scatter(dk, rows, M), dv=_scatter(dv, rows, M), du=du)


# ------------------------------------------------------------------------------- comparison
FLOOR = 2.0 ** -8          # one bf16 ulp of the block maximum
FACTOR = 3.0               # accumulation order, exp2 against exp, the lazy rescale
LSE_CAP = 2e-3             # the project's figure for the C-init forward (test_attention_fwd_cinit), natural log
# LSE floor: |lse| < 16 in every case here (scores of a few units plus ln L), so 2^-16 is 16 f32 ulps
# of the stored value -- the score's f32 accumulation, one v_exp / v_log and the ln 2 product
LSE_FLOOR = 2.0 ** -16
FROB = {'o': 8e-3, 'dq': 2e-2, 'dk': 2e-2, 'dv': 2e-2, 'du': 2e-2}   # the suite's Frobenius bounds


def block_err(got, ref, rows, H, D):
    """worst (sequence, head) block of max|got - ref| / max|ref|, both over the block"""
    g, r = (_heads(t.double(), rows, H, D).reshape(rows.shape[0], H, -1) for t in (got, ref))
    return ((g - r).abs().amax(-1) / r.abs().amax(-1).clamp_min(1e-300)).max().item()


def row_err(got, ref):
    """dU: the block is a head's row of bins"""
    g, r = got.double(), ref.double()
    return ((g - r).abs().amax(-1) / r.abs().amax(-1).clamp_min(1e-300)).max().item()


def lse_err(got, ref, rows):
    """absolute error, worst (head, sequence)"""
    return (got.double() - ref.double())[:, rows.reshape(-1)].abs().max().item()


def _err(name, got, ref, rows, H, D):
    if name == 'lse':
        return lse_err(got, ref, rows)
    if name == 'du':
        return row_err(got, ref)
    return block_err(got, ref, rows, H, D)


def attn_compare(got, ref, emul, rows, H, D, label='', log=print):
    """Every output of `got` (o, lse, dq, dk, dv, du; missing / None ones are skipped) against the
    float64 `ref`, with the emulation's own error E_emul under the same metric as the yardstick:
        err <= max(3 E_emul, 2^-8)                      o, dq, dk, dv, du (block-scaled maximum)
        err <= min(max(3 E_emul, 2^-16), 2e-3)          lse (absolute)
    plus finiteness and the suite's Frobenius bounds.  Returns {name: dict(err, e_emul, tol, frob,
    ok, frob_ok)}; prints one line per output."""
    res = {}
    for name in ('o', 'lse', 'dq', 'dk', 'dv', 'du'):
        if got.get(name) is None:
            continue
        g = got[name]
        finite = bool(torch.isfinite(g.float()[:, rows.reshape(-1)] if name == 'lse' else g.float()).all())
        err = _err(name, g, ref[name], rows, H, D)
        e_emul = _err(name, emul[name], ref[name], rows, H, D)
        if name == 'lse':
            tol, frob, frob_ok = min(max(FACTOR * e_emul, LSE_FLOOR), LSE_CAP), float('nan'), True
        else:
            tol = max(FACTOR * e_emul, FLOOR)
            frob = rel(g, ref[name])
            frob_ok = frob < FROB[name]
        ok = finite and err <= tol
        res[name] = dict(err=err, e_emul=e_emul, tol=tol, frob=frob, ok=ok, frob_ok=frob_ok, finite=finite)
        log(f'{label:30s} {name:3s} err {err:.3e}  E_emul {e_emul:.3e}  tol {tol:.3e}  frob {frob:.3e}'
            f'{"" if ok and frob_ok else "   <-- FAIL"}')
    return res


def attn_check(got, ref, emul, rows, H, D, label=''):
    res = attn_compare(got, ref, emul, rows, H, D, label)
    bad = {n: r for n, r in res.items() if not (r['ok'] and r['frob_ok'])}
    assert not bad, f'{label}: {bad}'
    return res
