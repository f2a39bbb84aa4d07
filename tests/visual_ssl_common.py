"""Float64 restatements of the three kernels of csrc/ssl.hip (the SimSiam visual self-supervision head,
DESIGN.md §33) and the per-element error bounds the tests hold them to.  Written from the formulas of the
kernels' contract (include/ctclip_hip.h) and torch's ``BatchNorm1d``; CPU tensors, float64.

Bounds, u = 2^-24 (f32 unit roundoff), to first order:

  y = X W^T (+ bias): an ascending fma chain of K terms is within K u (|X| |W|^T) of the exact sum; the tests
      allow bound_y = 4 K u (|X| |W|^T) + u |y| (margin 4; the bias add is one more rounding).
  centred value c = y - mean: the mean of a group is a sum of the same y, so |dc| <= 2 max_r bound_y =: bc
      (with the running statistics the mean is exact and bound_y alone would do; the same bc is used).
  rstd = (var + eps)^-1/2, var = mean c^2: d var <= 2 bc mean|c|, d rstd <= rstd^3 bc mean|c| <= rstd^2 bc
      (mean |xhat| <= 1); allowed rstd^2 bc + 8 u rstd.
  xhat = c rstd: |d xhat| <= bc rstd + |c| d rstd <= bc rstd (1 + xhat^2); allowed that + 8 u |xhat|.
  out = [relu](gamma xhat + beta): |gamma| bound_xhat + 8 u (|gamma xhat| + |beta|); relu is 1-Lipschitz.
The f32 accumulation of the statistics themselves (R <= 128 terms, relative error <= R u) is below the bc
term at every shape used: bc carries the factor 4 K >= 160.  eps = 1e-5 caps rstd at 316.

Backward, per group, dxhat = dout mask gamma, dy = rstd / R (R dxhat - s1 - xhat s2), s1 = sum dxhat,
s2 = sum dxhat xhat.  ``bn_bwd_bounds`` propagates given input perturbations (d dxhat, d xhat, d rstd) through
that expression to first order and adds the rounding of the sums, 4 (R + 4) u times the sum of the absolute
terms.  A ReLU mask can differ from the float64 one only where the pre-activation is within its own bound of
zero: there d dxhat = |dout gamma|.
"""
import math

import torch

U = 2.0 ** -24
SHAPES = [(1, 2, 40, 72), (2, 3, 516, 72), (2, 8, 512, 4), (2, 64, 64, 130)]      # (G, R, K, N)
FLAGS = [(a, r, b) for a in (True, False) for r in (True, False) for b in (True, False)]   # affine, relu, bias
EPS, MOM = 1e-5, 0.1


def make_inputs(G, R, K, N, affine, bias, seed=0, dtype=torch.float32):
    """N(0, 1) rows, W / sqrt(K) so y is O(1); gains around 1, running statistics off their defaults."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * G + 131 * R + 17 * K + N)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float32)
    d = dict(X=rn(G * R, K), W=rn(N, K) / math.sqrt(K), bias=0.5 * rn(N) if bias else None,
             gamma=1.0 + 0.3 * rn(N) if affine else None, beta=0.2 * rn(N) if affine else None,
             running_mean=0.1 * rn(N), running_var=1.0 + 0.2 * torch.rand(N, generator=g))
    return {k: (v if v is None else v.to(dtype)) for k, v in d.items()}


def linear_bn_ref(inp, G, relu, use_running=False, eps=EPS, momentum=MOM):
    """The float64 forward: dict of y, pre (pre-activation), out, xhat [G R, N], rstd [G, N] and the running
    statistics after the call."""
    f = lambda t: None if t is None else t.double()
    X, W, bias, gamma, beta = (f(inp[k]) for k in ('X', 'W', 'bias', 'gamma', 'beta'))
    rm, rv = f(inp['running_mean']).clone(), f(inp['running_var']).clone()
    M, N = X.shape[0], W.shape[0]
    R = M // G
    y = X @ W.t()
    if bias is not None:
        y = y + bias
    yg = y.view(G, R, N)
    if use_running:
        mean, var = rm.expand(G, N), rv.expand(G, N)
    else:
        mean = yg.mean(1)
        var = ((yg - mean[:, None]) ** 2).mean(1)             # biased
        for g in range(G):                                    # G successive BatchNorm1d calls
            rm = (1 - momentum) * rm + momentum * mean[g]
            rv = (1 - momentum) * rv + momentum * var[g] * R / (R - 1)
    rstd = (var + eps).rsqrt()
    xhat = ((yg - mean[:, None]) * rstd[:, None]).reshape(M, N)
    pre = xhat * gamma + beta if gamma is not None else xhat
    out = pre.clamp_min(0) if relu else pre
    return dict(y=y, pre=pre, out=out, xhat=xhat, rstd=rstd, running_mean=rm, running_var=rv)


def linear_bn_bounds(inp, ref, G):
    """Per-element bounds of out, xhat [G R, N] and rstd [G, N] (module docstring)."""
    X, W = inp['X'].double(), inp['W'].double()
    M, K = X.shape
    N = W.shape[0]
    by = 4 * K * U * (X.abs() @ W.abs().t()) + U * ref['y'].abs()
    bc = 2 * by.view(G, M // G, N).amax(1)                                     # [G, N]
    rstd, xhat = ref['rstd'], ref['xhat']
    b_rstd = rstd ** 2 * bc + 8 * U * rstd
    b_xhat = ((bc * rstd)[:, None] * (1 + xhat.view(G, -1, N) ** 2)).reshape(M, N) + 8 * U * xhat.abs()
    if inp['gamma'] is not None:
        ga, be = inp['gamma'].double(), inp['beta'].double()
        b_out = ga.abs() * b_xhat + 8 * U * ((ga * xhat).abs() + be.abs())
    else:
        b_out = b_xhat + 8 * U * xhat.abs()
    return dict(out=b_out, xhat=b_xhat, rstd=b_rstd)


def bn_bwd_ref(dout, out, xhat, rstd, gamma, relu, use_running=False):
    """The float64 BatchNorm (+ ReLU) backward on the given (float64) inputs: dy, dgamma, dbeta, dbias."""
    G, N = rstd.shape
    M = dout.shape[0]
    R = M // G
    d = dout * (out > 0) if relu else dout
    dxh = d * gamma if gamma is not None else d
    dg, xg = dxh.view(G, R, N), xhat.view(G, R, N)
    if use_running:
        dy = dg * rstd[:, None]
    else:
        s1, s2 = dg.sum(1, keepdim=True), (dg * xg).sum(1, keepdim=True)
        dy = rstd[:, None] / R * (R * dg - s1 - xg * s2)
    dy = dy.reshape(M, N)
    return dict(dy=dy, dgamma=(d * xhat).sum(0), dbeta=d.sum(0), dbias=dy.sum(0))


def bn_bwd_bounds(dout, out, xhat, rstd, gamma, relu, use_running=False, d_d=None, d_xhat=None, d_rstd=None):
    """Bounds of bn_bwd_ref's outputs: the rounding of the f32 evaluation plus, to first order, the effect of
    input perturbations d_d (of dout mask), d_xhat, d_rstd (zero when not given)."""
    G, N = rstd.shape
    M = dout.shape[0]
    R = M // G
    zero = torch.zeros_like(dout)
    d_d = zero if d_d is None else d_d
    d_xhat = zero if d_xhat is None else d_xhat
    d_rstd = torch.zeros_like(rstd) if d_rstd is None else d_rstd
    ga = gamma.abs() if gamma is not None else torch.ones(N, dtype=dout.dtype)
    d = dout * (out > 0) if relu else dout
    dxh = (d * ga).abs().view(G, R, N)
    ddx = (d_d * ga).view(G, R, N)
    xg, bx = xhat.abs().view(G, R, N), d_xhat.view(G, R, N)
    ref = bn_bwd_ref(dout, out, xhat, rstd, gamma, relu, use_running)
    dyr = ref['dy'].abs().view(G, R, N)
    rs = rstd[:, None]
    if use_running:
        b_dy = rs * ddx + d_rstd[:, None] * dxh + 8 * U * dyr
    else:
        s1a, s2a = dxh.sum(1, keepdim=True), (dxh * xg).sum(1, keepdim=True)
        terms = R * dxh + s1a + xg * s2a
        prop = R * ddx + ddx.sum(1, keepdim=True) + bx * s2a + xg * (ddx * xg + dxh * bx).sum(1, keepdim=True)
        b_dy = (d_rstd / rstd)[:, None] * dyr + rs / R * prop + 4 * (R + 4) * U * rs / R * terms
    b_dy = b_dy.reshape(M, N)
    rnd = 4 * (M + 2) * U
    da = d.abs()
    return dict(dy=b_dy,
                dgamma=(d_d * xhat.abs() + da * d_xhat).sum(0) + rnd * (da * xhat.abs()).sum(0),
                dbeta=d_d.sum(0) + rnd * da.sum(0),
                dbias=b_dy.sum(0) + rnd * ref['dy'].abs().sum(0))


def simsiam_ref(p1, p2, z1, z2):
    """loss (scalar) = mean_b (2 - 2 cos(p1_b, z2_b)) + (2 - 2 cos(p2_b, z1_b)), cos through x / max(|x|, 1e-12)."""
    unit = lambda x: x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return ((2 - 2 * (unit(p1) * unit(z2)).sum(-1)) + (2 - 2 * (unit(p2) * unit(z1)).sum(-1))).mean()


def simsiam_ref_grads(p1, p2, z1, z2):
    """float64 (loss, dp1, dp2) by autograd; the targets are constants."""
    a, b = p1.double().clone().requires_grad_(True), p2.double().clone().requires_grad_(True)
    loss = simsiam_ref(a, b, z1.double(), z2.double())
    loss.backward()
    return loss.detach(), a.grad, b.grad


def head_ref64(head, views):
    """The loss of a float64 copy of ``head`` (loaded from its state_dict) on ``views`` [2, B, dim], in the
    head's mode; the copy's buffers afterwards are what the head's must be."""
    from ctclip_mi355x.visual_ssl import VisualSSLHead
    bn = head.projector[1]
    copy = VisualSSLHead(head.dim, head.projection_size, head.projection_hidden_size, momentum=bn.momentum,
                         eps=bn.eps).double()
    copy.load_state_dict({k: v.detach().cpu() for k, v in head.state_dict().items()})
    copy.train(head.training)
    return copy(views.detach().double().cpu()), copy


def worst(got, ref, bound):
    """max over elements of |got - ref| / bound (float64, CPU)."""
    return ((got.double().cpu() - ref).abs() / bound).max().item()
