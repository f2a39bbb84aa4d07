"""Linear-probe evaluation: how linearly separable are the pathologies in the FROZEN image latents?

``LinearProbe`` is a multi-label logistic regression (one logit per pathology) over the [N, Dl] f32 latents
of ``zero_shot.image_latents``, fitted by full-batch Adam / AdamW.  On the device each step is two queued
calls -- ``K.probe_step`` (csrc/probe.hip: loss, dW and db in one pass over the latents, exact f32 on the
matrix pipe, bit-reproducible) and ``K.adam`` over a two-tensor flat arena -- with no host synchronisation
inside the loop.  On CPU tensors the same class runs ``step_reference``, a torch restatement of the step in
the operands' dtype (float64 included): what the GPU tests compare the kernel against.

``LinearProbeEvaluator`` reports the fitted probe with the functions of ``evaluate.py`` that score the
zero-shot classifier, under ``ZeroShotEvaluator.evaluate``'s keys, so both sit in one table.
The towers are never touched: they run in eval mode under ``no_grad`` through ``zero_shot.image_latents``.
"""
from __future__ import annotations

import torch
from torch import nn

from . import evaluate as E
from . import kernels as K
from . import zero_shot
from .ct_clip import require_cls_latents

UNLABELLED = 255          # a label entry that is excluded from loss, gradient and count


class NonFiniteLossError(ValueError):
    """``LinearProbe.fit`` ended on a loss that is not finite (non-finite latents, or a diverged fit)."""


def labels_u8(labels, device=None):
    """[N, P] labels as the step's uint8: 0 / 1 (floats are rounded), 255 and NaN = not labelled."""
    y = torch.as_tensor(labels)
    if device is not None:
        y = y.to(device)
    if y.dtype == torch.uint8:
        return y.contiguous()
    if y.is_floating_point():
        un = torch.isnan(y) | (y == UNLABELLED)
        y = torch.round(torch.nan_to_num(y))
    else:
        un = y == UNLABELLED
    out = (y != 0).to(torch.uint8)
    out[un] = UNLABELLED
    return out.contiguous()


def step_reference(X, W, b, Y, idx=None, pos_weight=None):
    """The arithmetic of ``ctclip_probe_step`` (include/ctclip_hip.h) in torch, in X's dtype: a dict of loss
    [1], dW [P, D], db [P], Z [M, P] and count (int64 [1]) for the rows ``X[idx]`` (all rows when None).
    Y: uint8 [N, P], 255 = not counted.  With no 255 it is ``F.binary_cross_entropy_with_logits(Z, Y,
    pos_weight=pos_weight, reduction='mean')`` and its gradient; count == 0 gives loss 0 and zero gradients."""
    dt = X.dtype
    if idx is not None:
        X, Y = X[idx.long()], Y[idx.long()]
    Z = X @ W.t() + b
    counted = Y != UNLABELLED
    y = (counted & (Y != 0)).to(dt)
    cnt = counted.sum()
    L = 1 + (pos_weight.to(dt) - 1) * y if pos_weight is not None else torch.ones_like(y)
    ell = (1 - y) * Z + L * (torch.clamp(-Z, min=0) + torch.log1p(torch.exp(-Z.abs())))
    den = torch.clamp(cnt, min=1).to(dt)
    zero = torch.zeros((), dtype=dt, device=X.device)
    loss = torch.where(counted, ell, zero).sum() / den
    r = torch.where(counted, (1 - y) - L * torch.sigmoid(-Z), zero) / den
    return dict(loss=loss.reshape(1), dW=r.t() @ X, db=r.sum(0), Z=Z, count=cnt.reshape(1))


def balanced_pos_weight(Y, idx=None, dtype=torch.float32):
    """n_neg / n_pos per label over the counted rows (computed where Y lives, nothing read back); a label
    with no positive or no negative gets 1."""
    if idx is not None:
        Y = Y[idx.long()]
    pos = (Y == 1).sum(0).to(torch.float64)
    neg = (Y == 0).sum(0).to(torch.float64)
    ok = (pos > 0) & (neg > 0)
    return torch.where(ok, neg / torch.clamp(pos, min=1), torch.ones_like(pos)).to(dtype).contiguous()


class LinearProbe(nn.Module):
    """``weight`` [P, D] and ``bias`` [P], zero-initialised; ``forward`` gives the logits."""

    def __init__(self, dim, n_labels, dtype=torch.float32, device=None):
        super().__init__()
        self.weight = nn.Parameter(torch.zeros(n_labels, dim, dtype=dtype, device=device))
        self.bias = nn.Parameter(torch.zeros(n_labels, dtype=dtype, device=device))

    def _operands(self, latents):
        X = latents.detach()
        if X.dim() != 2 or X.shape[1] != self.weight.shape[1]:
            raise ValueError(f'LinearProbe: latents [N, {self.weight.shape[1]}], got {tuple(X.shape)}')
        if X.device != self.weight.device or X.dtype != self.weight.dtype:
            raise ValueError(f'LinearProbe: latents are {X.dtype} on {X.device}, the probe is {self.weight.dtype} on '
                             f'{self.weight.device}')
        return X

    def forward(self, latents):
        X = self._operands(latents)
        W, b = self.weight.detach(), self.bias.detach()
        if X.is_cuda:
            return K.probe_step(X, W, b, None, want=('Z',))['Z']
        return X @ W.t() + b

    def predict_proba(self, latents):
        return torch.sigmoid(self.forward(latents))

    def fit(self, latents, labels, *, steps=500, lr=1e-2, wd=0.0, betas=(0.9, 0.999), eps=1e-8, pos_weight=None,
            rows=None):
        """Full-batch Adam (``wd != 0``: AdamW, decay on ``weight`` only -- the trainer's ndim >= 2 rule) on the
        mean BCE-with-logits of the counted label entries.  ``labels`` [N, P]: 0 / 1, 255 (or NaN) = not
        labelled.  ``pos_weight``: None, a [P] tensor, or 'balanced' (``balanced_pos_weight``).  ``rows``: row
        indices the fit runs over (a subset, a fold, a resample: repeats allowed).  Continues from the current
        ``weight`` / ``bias`` with fresh moments.  Returns the per-step loss [steps] (the loss BEFORE each update), kept on the
        latents' device; one host read at the end raises ValueError if the last one is not finite."""
        X = self._operands(latents)
        P, D = self.weight.shape
        Y = labels_u8(labels, X.device)
        if tuple(Y.shape) != (X.shape[0], P):
            raise ValueError(f'LinearProbe.fit: labels {tuple(Y.shape)} do not match {(X.shape[0], P)}')
        steps = int(steps)
        if steps < 1:
            raise ValueError(f'LinearProbe.fit: steps >= 1, got {steps}')
        idx = None if rows is None else torch.as_tensor(rows).to(device=X.device, dtype=torch.int32).contiguous()
        if idx is not None and (idx.dim() != 1 or idx.numel() < 1):
            raise ValueError(f'LinearProbe.fit: rows is a non-empty 1-d index list, got {tuple(idx.shape)}')
        if isinstance(pos_weight, str):
            if pos_weight != 'balanced':
                raise ValueError(f"LinearProbe.fit: pos_weight is None, a [P] tensor or 'balanced', got {pos_weight!r}")
            pw = balanced_pos_weight(Y, idx, X.dtype)
        elif pos_weight is not None:
            pw = torch.as_tensor(pos_weight).to(device=X.device, dtype=X.dtype).contiguous()
        else:
            pw = None
        losses = torch.zeros(steps, dtype=X.dtype, device=X.device)
        if X.is_cuda:
            self._fit_device(X, Y, idx, pw, losses, steps, lr, wd, betas, eps)
        else:
            self._fit_reference(X, Y, idx, pw, losses, steps, lr, wd, betas, eps)
        last = float(losses[-1])                       # the one host read
        if last != last or last in (float('inf'), float('-inf')):
            raise NonFiniteLossError(f'LinearProbe.fit: the loss is {last} after {steps} steps (lr {lr})')
        return losses

    def _fit_device(self, X, Y, idx, pw, losses, steps, lr, wd, betas, eps):
        P, D = self.weight.shape
        n = P * D
        # the two-tensor flat arena: [weight | bias], with its gradient and moments in the same layout
        flat = torch.cat([self.weight.detach().reshape(-1), self.bias.detach()]).contiguous()
        g, m, v = torch.zeros_like(flat), torch.zeros_like(flat), torch.zeros_like(flat)
        W, b = flat[:n].view(P, D), flat[n:]
        out = dict(dW=g[:n].view(P, D), db=g[n:])
        hyp = dict(lr=float(lr), b1=float(betas[0]), b2=float(betas[1]), eps=float(eps))
        # the towers' weights do not change here: K.adam's weights epoch (derived-weight caches) is put back
        epoch = K.weights_epoch()
        for s in range(steps):
            out['loss'] = losses[s:s + 1]
            K.probe_step(X, W, b, Y, idx=idx, pos_weight=pw, want=('loss', 'dW', 'db'), out=out)
            if wd == 0:
                K.adam(flat, g, m, v, wd=0.0, step=s + 1, **hyp)
            else:
                K.adam(flat[:n], g[:n], m[:n], v[:n], wd=float(wd), step=s + 1, **hyp)
                K.adam(flat[n:], g[n:], m[n:], v[n:], wd=0.0, step=s + 1, **hyp)
        K._WEIGHTS_EPOCH[0] = epoch
        with torch.no_grad():
            self.weight.copy_(W)
            self.bias.copy_(b)

    def _fit_reference(self, X, Y, idx, pw, losses, steps, lr, wd, betas, eps):
        W, b = self.weight, self.bias
        kw = dict(lr=lr, betas=tuple(betas), eps=eps)
        opt = (torch.optim.Adam([W, b], **kw) if wd == 0 else
               torch.optim.AdamW([dict(params=[W], weight_decay=wd), dict(params=[b], weight_decay=0.0)], **kw))
        for s in range(steps):
            with torch.no_grad():
                res = step_reference(X, W, b, Y, idx, pw)
            losses[s] = res['loss'][0]
            W.grad, b.grad = res['dW'], res['db']
            opt.step()
        W.grad = b.grad = None


class LinearProbeEvaluator:
    """Fit and score a ``LinearProbe`` on a model's frozen image latents.  ``evaluate`` returns
    ``ZeroShotEvaluator.evaluate``'s dict, computed by the same functions of ``evaluate.py``."""

    def __init__(self, model, pathologies=zero_shot.PATHOLOGIES, normalize=True):
        require_cls_latents(model, 'LinearProbeEvaluator')
        self.model = model
        self.pathologies = tuple(pathologies)
        self.normalize = normalize
        self.probe = None

    def encode(self, volumes, batch_size=8):
        """[N, Dl] f32 latents of ``volumes`` (an (N, 1, D, H, W) tensor or an iterable of such batches)
        through ``zero_shot.image_latents`` -- eval mode, no_grad -- l2-normalised per row unless
        ``normalize=False`` (the contrastive loss compares the normalised latents)."""
        batches = [volumes] if isinstance(volumes, torch.Tensor) else volumes
        lat = [zero_shot.image_latents(self.model, vb[i:i + batch_size])
               for vb in batches for i in range(0, vb.shape[0], batch_size)]
        lat = torch.cat(lat).float()
        return nn.functional.normalize(lat, dim=-1).contiguous() if self.normalize else lat.contiguous()

    def _latents(self, x, batch_size):
        if isinstance(x, torch.Tensor) and x.dim() == 2:
            return x
        return self.encode(x, batch_size=batch_size)

    def fit(self, train, train_labels, batch_size=8, **fit_kw):
        """``train``: latents [N, Dl] (as ``encode`` gives them) or volumes.  Fits a fresh probe; returns the
        per-step loss of ``LinearProbe.fit``."""
        lat = self._latents(train, batch_size)
        self.probe = LinearProbe(lat.shape[1], len(self.pathologies), dtype=lat.dtype, device=lat.device)
        return self.probe.fit(lat, train_labels, **fit_kw)

    def evaluate(self, volumes, labels, n_boot=0, curves=False, batch_size=8):
        """``volumes``: latents [N, Dl] or volumes; labels [N, P] of 0 / 1.  The dict of
        ``ZeroShotEvaluator.evaluate``: probs, auroc, ci, f1_micro, flat_accuracy, and with ``curves=True``
        curves (and curves_ci with n_boot > 0)."""
        if self.probe is None:
            raise RuntimeError('LinearProbeEvaluator.evaluate: fit() first')
        probe = self.probe

        class _Scores:                                  # the classifier ZeroShotEvaluator scores: predict -> (probs, _)
            @staticmethod
            def predict(lat, batch_size=None):
                return probe.predict_proba(lat), None
        return E.ZeroShotEvaluator(_Scores).evaluate(self._latents(volumes, batch_size), labels, n_boot=n_boot,
                                                     curves=curves)


__all__ = ['LinearProbe', 'LinearProbeEvaluator', 'NonFiniteLossError', 'step_reference', 'balanced_pos_weight', 'labels_u8', 'UNLABELLED']
