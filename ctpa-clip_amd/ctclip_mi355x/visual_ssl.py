"""SimSiam visual self-supervision head for CT volumes (Chen & He 2021).

The reference's ``use_visual_ssl`` (ct_clip/ct_clip.py:526-545, visual_ssl.py) wraps the image tower in a 2-D
SimSiam: it sends ``randn(2, C, S, S)`` through the tower, augments with torchvision's colour-image pipeline and
sizes its first projector layer by the flattened tower output.  None of that runs on a 3-D CT tower, so this is
a restatement: the SimSiam projector / predictor / loss on the RAW IMAGE LATENTS of two views, which the
multiview forward (``CTCLIP.forward(aug_image=...)``) already computes.

    head = VisualSSLHead(dim_latent)
    model = CTCLIP(..., visual_ssl=head, image_ssl_loss_weight=0.05)

``projector`` and ``predictor`` are plain ``nn.Sequential``s of ``nn.Linear`` / ``nn.BatchNorm1d`` / ``nn.ReLU``
in the SimSiam layout, so the ``state_dict`` keys are torch's (``projector.0.weight``,
``projector.1.running_mean``, ...) and a float64 torch copy loads them.  On device tensors ``forward`` does not
call the Sequentials: each Linear + BatchNorm1d (+ ReLU) is one launch of ``functional.LinearBNFn`` with the
two views as two BatchNorm groups, the predictor's last Linear is ``functional.LinearBiasFn`` and the loss is
``functional.SimSiamLossFn`` (csrc/ssl.hip).  CPU tensors run the Sequentials view by view: the restatement
the CPU tests compare against.

Two differences from the reference's SimSiam, with the same numbers: the target projections are the online
ones detached (its "target encoder" IS the online encoder, evaluated a second time under no_grad), so the
BatchNorm running statistics are updated once per view and forward, not twice.
"""
from __future__ import annotations

import torch
from torch import nn

from . import functional as Fn

MAX_ROWS = 128      # rows of one fused Linear + BatchNorm launch (both views): kernels.ssl_linear_bn


class VisualSSLHead(nn.Module):
    def __init__(self, dim, projection_size=256, projection_hidden_size=4096, momentum=0.1, eps=1e-5):
        super().__init__()
        d, h, p = int(dim), int(projection_hidden_size), int(projection_size)
        if min(d, h, p) < 1:
            raise ValueError(f'VisualSSLHead: widths must be positive, got dim={dim}, hidden={h}, projection={p}')
        self.dim, self.projection_size, self.projection_hidden_size = d, p, h

        def bn(n, affine=True):
            return nn.BatchNorm1d(n, eps=eps, momentum=momentum, affine=affine)

        self.projector = nn.Sequential(nn.Linear(d, h, bias=False), bn(h), nn.ReLU(),
                                       nn.Linear(h, h, bias=False), bn(h), nn.ReLU(),
                                       nn.Linear(h, p, bias=False), bn(p, affine=False))
        self.predictor = nn.Sequential(nn.Linear(p, h), bn(h), nn.ReLU(), nn.Linear(h, p))

    def _fused(self, x, lin, norm, relu):
        """One Linear + BatchNorm1d (+ ReLU) launch over both views (two BatchNorm groups)."""
        y = Fn.LinearBNFn.apply(x, lin.weight, lin.bias, norm.weight, norm.bias, norm.running_mean,
                                norm.running_var, 2, relu, norm.eps, norm.momentum, not self.training)
        if self.training:
            norm.num_batches_tracked += 2       # as the two BatchNorm1d calls it stands for
        return y

    def forward(self, views):
        """``views`` [2, B, dim]: the raw image latents of two views of the same B volumes.  Returns the scalar
        SimSiam loss mean_b (2 - 2 cos(p1_b, z2_b)) + (2 - 2 cos(p2_b, z1_b)), z = projector(view),
        p = predictor(z), the targets z detached."""
        if views.dim() != 3 or views.shape[0] != 2 or views.shape[2] != self.dim:
            raise ValueError(f'VisualSSLHead: views must be [2, B, {self.dim}], got {tuple(views.shape)}')
        B = views.shape[1]
        if self.training and B < 2:
            raise ValueError('VisualSSLHead: training needs more than one volume per view (BatchNorm1d has no '
                             'batch statistics at B = 1)')
        if not views.is_cuda:
            z = [self.projector(views[g]) for g in range(2)]
            p = [self.predictor(z[g]) for g in range(2)]
            return (simsiam_loss_rows(p[0], z[1].detach()) + simsiam_loss_rows(p[1], z[0].detach())).mean()
        if 2 * B > MAX_ROWS:
            raise ValueError(f'VisualSSLHead: at most {MAX_ROWS // 2} volumes per view on the device, got {B}')
        if views.dtype != torch.float32:
            raise ValueError(f'VisualSSLHead: f32 latents on the device, got {views.dtype}')
        pj, pd = self.projector, self.predictor
        x = views.reshape(2 * B, self.dim)
        x = self._fused(x, pj[0], pj[1], True)
        x = self._fused(x, pj[3], pj[4], True)
        z = self._fused(x, pj[6], pj[7], False)
        q = self._fused(z, pd[0], pd[1], True)
        p = Fn.LinearBiasFn.apply(q, pd[3].weight, pd[3].bias)
        return Fn.SimSiamLossFn.apply(p[:B], p[B:], z[:B], z[B:])


def simsiam_loss_rows(p, z):
    """2 - 2 cos(p_b, z_b) per row, cos through ``F.normalize`` (eps 1e-12)."""
    return 2 - 2 * (nn.functional.normalize(p, dim=-1) * nn.functional.normalize(z, dim=-1)).sum(dim=-1)
