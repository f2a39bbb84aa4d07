"""Shared pieces of tests/test_gpu_grad_audit.py: float64 references on the CPU oracle, the bounds
of the audit and the comparison / sink-semantics helpers.  Nothing here touches the GPU by itself."""
import contextlib

import torch

from oracle import ctclip_oracle as O

# the project's bounds for each kind of quantity (relative Frobenius error against float64)
OUT_BF16 = 4e-3      # f32 output computed from 16-bit operands
DX = 1e-2            # input gradient
DW = 3e-2            # parameter gradient (tests/test_gpu_ln1_fold.py::test_layer_fold_vs_unfolded)
F32 = 1e-5           # anything computed wholly in f32
MODEL_GRAD = 5e-2    # whole-model parameter gradient (test_backward_grads, GRAD_TOL of the chunked step)
SINK = 1e-6          # .grad arithmetic: same deterministic kernels, only the f32 add differs


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def bf16r(t):
    """t rounded to bf16-representable f32 values."""
    return t.bfloat16().float()


def perturb(mod, seed, scale=0.02):
    """Move every parameter off its initial value (scales of 1 and biases of 0 hide missing terms)."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in mod.parameters():
            if p.numel():
                p.add_((scale * torch.randn(p.shape, generator=g)).to(p.device))
    return mod


def spread_scales(tr, seed, scale=0.25):
    """Move every layer's q_scale / k_scale well apart: d sim / d q_scale[d] * q_scale[d] equals
    d sim / d k_scale[d] * k_scale[d], so with both near 1 an exchange of the two gradients would
    sit inside the parameter-gradient bound."""
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for _, attn, _, _ in tr.layers:
            for p in (attn.q_scale, attn.k_scale):
                p.add_((scale * torch.randn(p.shape, generator=g)).to(p.device))
    return tr


def module_sd(mod, prefix=''):
    """float64 CPU oracle state dict of a module: every parameter a leaf that records its gradient."""
    sd = {}
    for k, v in mod.state_dict().items():
        v = v.detach().cpu().clone()
        sd[prefix + k] = v.double() if v.is_floating_point() else v
    for k, p in mod.named_parameters():
        if p.numel():
            sd[prefix + k].requires_grad_(True)
    return sd


def leaf(t):
    return t.detach().double().cpu().clone().requires_grad_(True)


def cpb_bins(h, w):
    """[h*w, h*w] index of each (i, j) pair's relative offset in the deduplicated CPB table."""
    pos = torch.stack(torch.meshgrid(torch.arange(h), torch.arange(w), indexing='ij')).reshape(2, -1).t()
    r = pos[:, None, :] - pos[None, :, :]
    return (r[..., 0] + h - 1) * (2 * w - 1) + (r[..., 1] + w - 1)


def to_seq(x, geo):
    """Canonical rows (b, t, h, w) [M, D] -> the (n, L, D) view the reference's transformer sees."""
    hw, D = geo.Hg * geo.Wg, x.shape[-1]
    if geo.mode == 0:
        return x.reshape(geo.B * geo.T, hw, D)
    return x.reshape(geo.B, geo.T, hw, D).permute(0, 2, 1, 3).reshape(geo.B * hw, geo.T, D)


def from_seq(y, geo):
    hw, D = geo.Hg * geo.Wg, y.shape[-1]
    if geo.mode == 0:
        return y.reshape(geo.M, D)
    return y.reshape(geo.B, hw, geo.T, D).permute(0, 2, 1, 3).reshape(geo.M, D)


def ref_transformer(sd, p, x, geo, depth, dense_bias=None):
    """oracle transformer_forward on canonical rows x [M, D] (float64) -> canonical rows."""
    y = O.transformer_forward(sd, p, to_seq(x, geo), depth, geo.heads, geo.dim_head,
                              (geo.B, geo.T, geo.Hg, geo.Wg), dense_bias)
    return from_seq(y, geo)


class Rows:
    """The measured (label, error, bound) rows of one test: printed, then asserted together."""

    def __init__(self, tag):
        self.tag, self.rows = tag, []

    def add(self, label, err, bound):
        self.rows.append((label, float(err), bound))

    def params(self, named, sd, prefix, bound, sibling_zero=()):
        """Every parameter of ``named`` against the gradient the float64 reference left in ``sd``;
        ``sibling_zero`` {name: sibling}: gradients that are zero in exact arithmetic (softmax shift
        invariance), bounded relative to the sibling's reference gradient instead."""
        for n, p in named:
            if not p.numel():
                continue
            r = sd[prefix + n].grad
            if n in sibling_zero:      # zero in exact arithmetic: measured against its sibling's scale
                sn = sd[prefix + sibling_zero[n]].grad.norm().item()
                assert r.norm().item() < 1e-12 * sn, (n, r.norm().item(), sn)
                e = float('inf') if p.grad is None else p.grad.double().norm().item() / sn
                self.add(f'd {n} / |d {sibling_zero[n]}|', e, bound)
            elif r is None:
                z = p.grad is None or not bool(p.grad.count_nonzero().item())
                self.add(f'd {n} (no gradient in the reference)', 0.0 if z else float('inf'), 0.0)
            elif p.grad is None:
                self.add(f'd {n} (MISSING)', float('inf'), bound)
            else:
                self.add(f'd {n}', rel(p.grad, r), bound)

    def check(self):
        for label, e, b in self.rows:
            print(f'AUDIT {self.tag} | {label} | {e:.3e} | {b:.0e}')
        bad = [r for r in self.rows if not r[1] <= r[2]]
        assert not bad, (self.tag, bad)


def grads_of(params):
    return [None if p.grad is None else p.grad.detach().clone() for p in params]


def sink_checks(tag, run, params, K, sync):
    """Part C of the audit on one forward + backward ``run()`` that leaves .grad of ``params`` alone
    otherwise: (i) a backward into pre-filled .grad adds exactly the gradient of a run from None,
    (ii) two backwards without zeroing give twice it, (iii) no deferred reduction is left pending."""
    params = [p for p in params if p.numel()]

    def clear():
        for p in params:
            p.grad = None
    clear()
    run()
    sync()
    assert not K._DEFERRED, 'a deferred reduction is still queued after the backward'
    g1 = grads_of(params)
    K.flush_reductions()
    sync()
    for a, p in zip(g1, params):                       # (iii): bit for bit
        assert (a is None) == (p.grad is None) and (a is None or torch.equal(a, p.grad)), tag
    live = [(p, g) for p, g in zip(params, g1) if g is not None]
    assert live
    rows = Rows(tag)
    # (i) a random base of each gradient's own magnitude (the f32 add then rounds at ~6e-8 of it)
    gen = torch.Generator().manual_seed(5)
    clear()
    bases = []
    for p, g in live:
        s = (g.double().norm() / max(g.numel(), 1) ** 0.5).item()
        b = (torch.randn(g.shape, generator=gen) * s).to(g.device)
        p.grad = b.clone()
        bases.append(b)
    run()
    sync()
    for i, ((p, g), b) in enumerate(zip(live, bases)):
        rows.add(f'(i) grad {i} {tuple(g.shape)} - base', rel(p.grad.double() - b.double(), g), SINK)
    # (ii)
    clear()
    run()
    run()
    sync()
    for i, (p, g) in enumerate(live):
        rows.add(f'(ii) grad {i} {tuple(g.shape)} two backwards', rel(p.grad, 2 * g.double()), SINK)
    clear()
    rows.check()


@contextlib.contextmanager
def vit_variant(name):
    """The forward / backward variants of ViTLayerFn, every switch restored on the way out."""
    from ctclip_mi355x import functional as Fn, kernels as K, precise
    f16, fold = Fn.vit_f16(), Fn._LN1_FOLD
    try:
        with contextlib.ExitStack() as st:
            if name == 'bf16':
                Fn.set_vit_f16(False)
            elif name == 'unfold':
                Fn._LN1_FOLD = False
            elif name == 'guard':
                st.enter_context(K.ln_guard())
            elif name in ('f32', 'split'):
                st.enter_context(precise.vit_precision_scope(name))
            else:
                assert name in ('default', 'heads16'), name
            yield
    finally:
        Fn.set_vit_f16(f16)
        Fn._LN1_FOLD = fold
