"""Retrieval evaluation on the HIP path: given a report, how high does its own volume rank among all
volumes, and the other way round -- the report-to-volume Recall@5/10/50/100 CT-CLIP's evaluation
reports beside the zero-shot AUROC.

The latents come from the forwards ``zero_shot.ZeroShotClassifier`` uses (eval mode, no grad); the
ranking runs in two HIP kernels (csrc/retrieval.hip) that never write the N x M score matrix:
``kernels.retrieval_ranks`` (the 0-based place of each query's positive in a stable descending sort
of its scores) and ``kernels.retrieval_topk``.  Ties are the normal case (radiology reports repeat
verbatim): among equal scores the lower gallery index ranks first, in both kernels.

The metric functions below are plain torch on the rank vector and work on any device.
"""
from __future__ import annotations

import types

import torch

from . import kernels as K
from . import zero_shot as Z
from .ct_clip import require_cls_latents
from .evaluate import bootstrap_indices, compute_cis

DEFAULT_KS = (1, 5, 10, 50, 100)


def _ranks(ranks):
    r = torch.as_tensor(ranks)
    if r.dim() != 1 or r.numel() == 0 or r.is_floating_point():
        raise ValueError(f'retrieval: ranks must be a non-empty integer vector, got {tuple(r.shape)} {r.dtype}')
    return r.long()


def recall_at_k(ranks, ks=DEFAULT_KS):
    """Recall@K [len(ks)] f64 (a host tensor): the share of queries whose positive has 0-based rank < K."""
    r = _ranks(ranks)
    kk = torch.as_tensor(list(ks), dtype=torch.long, device=r.device)
    # an integer count on the ranks' device, one IEEE division on the host (a device may divide by a
    # scalar through its reciprocal): a host tensor, the same bits wherever the ranks live
    return (r[None, :] < kk[:, None]).sum(1).cpu().double() / r.numel()


def median_rank(ranks):
    """Median of the 1-based ranks (the mean of the two middle ones for an even count), a float."""
    r = torch.sort(_ranks(ranks) + 1).values
    n = r.numel()
    return (int(r[(n - 1) // 2]) + int(r[n // 2])) / 2


def mean_reciprocal_rank(ranks):
    """Mean of 1 / (1-based rank), a float (summed on the host: one answer whatever the device)."""
    r = _ranks(ranks).cpu()
    return float((1.0 / (r + 1).double()).sum()) / r.numel()


def bootstrap_recall(ranks, ks=DEFAULT_KS, n_samples=1000):
    """[n_samples, len(ks)] f64 (host): Recall@K of ``evaluate.bootstrap_indices``' resamples of the QUERIES
    (the gallery, and so every query's rank, stays fixed); ``evaluate.compute_cis`` takes the table."""
    r = _ranks(ranks)
    rows = torch.from_numpy(bootstrap_indices(r.numel(), n_samples)).long().to(r.device)
    kk = torch.as_tensor(list(ks), dtype=torch.long, device=r.device)
    return (r[rows][:, None, :] < kk[None, :, None]).sum(2).cpu().double() / r.numel()


def _direction(ranks, ks, n_boot):
    valid = ranks[ranks >= 0]
    return dict(ranks=ranks, recall=recall_at_k(valid, ks), median_rank=median_rank(valid),
                mrr=mean_reciprocal_rank(valid),
                ci=compute_cis(bootstrap_recall(valid, ks, n_boot)) if n_boot else None)


def _batches(n, batch_size):
    if batch_size < 1:
        raise ValueError(f'retrieval: batch_size {batch_size}')
    return range(0, n, batch_size)


class RetrievalEvaluator:
    """Report <-> volume retrieval metrics of a ``ctclip_mi355x.CTCLIP``."""

    def __init__(self, model):
        require_cls_latents(model, 'RetrievalEvaluator')
        self.model = model

    def text_latents(self, text, batch_size=8):
        """Raw text latents [R, Dl] of ``text`` (``.input_ids`` / ``.attention_mask`` of R rows)."""
        ids, mask = text.input_ids, text.attention_mask
        return torch.cat([Z.text_latents(self.model, types.SimpleNamespace(input_ids=ids[i:i + batch_size],
                                                                           attention_mask=mask[i:i + batch_size]))
                          for i in _batches(ids.shape[0], batch_size)])

    def image_latents(self, volumes, batch_size=8):
        """Raw image latents [V, Dl]; volumes: a (V, 1, D, H, W) tensor or an iterable of such batches."""
        if isinstance(volumes, torch.Tensor):
            volumes = [volumes]
        return torch.cat([Z.image_latents(self.model, v[i:i + batch_size]) for v in volumes
                          for i in _batches(v.shape[0], batch_size)])

    def evaluate(self, volumes, text, pair=None, ks=DEFAULT_KS, n_boot=0, topk=0, batch_size=8):
        """``pair`` [R]: the volume of each report (several reports may share one); None: report i
        belongs to volume i (needs R == V).  Returns a dict:

        ``text_latents`` [R, Dl], ``image_latents`` [V, Dl]: the raw latents that were ranked;
        ``report_to_volume``, ``volume_to_report``: each a dict of ``ranks`` (int32, 0-based),
        ``recall`` ([len(ks)] f64), ``median_rank`` (1-based), ``mrr``, ``ci`` (None, or with
        n_boot > 0 ``compute_cis``' [3, len(ks)] mean / lower / upper table over n_boot resamples of
        the queries) and, with topk > 0, ``score`` / ``idx`` [queries, topk]: the best gallery rows.

        report_to_volume: ranks [R], the place of the report's own volume among the V volumes.
        volume_to_report: ranks [V], the place of the volume's BEST-RANKED own report among the R
        reports (with one report per volume simply that report's); a volume without any report has
        rank -1 and is left out of the metrics."""
        t = self.text_latents(text, batch_size)
        v = self.image_latents(volumes, batch_size)
        R, V = t.shape[0], v.shape[0]
        if pair is None:
            if R != V:
                raise ValueError(f'RetrievalEvaluator: pair=None pairs report i with volume i, but there are {R} '
                                 f'reports and {V} volumes')
            r2v = K.retrieval_ranks(t, v)
            v2r = K.retrieval_ranks(v, t)
        else:
            pair = torch.as_tensor(pair).to(t.device)
            r2v = K.retrieval_ranks(t, v, pair)
            # one query per report: its volume against all reports.  The volume's best-ranked own report
            # has none of its other reports above it, so its place there is the volume's rank
            per_report = K.retrieval_ranks(v[pair.long()], t)
            v2r = torch.full((V,), R, device=t.device, dtype=torch.int32)
            v2r = v2r.scatter_reduce(0, pair.long(), per_report, 'amin')
            v2r = torch.where(v2r == R, torch.full_like(v2r, -1), v2r)
        res = dict(text_latents=t, image_latents=v, report_to_volume=_direction(r2v, ks, n_boot),
                   volume_to_report=_direction(v2r, ks, n_boot))
        if topk:
            for name, q, g in (('report_to_volume', t, v), ('volume_to_report', v, t)):
                res[name]['score'], res[name]['idx'] = K.retrieval_topk(q, g, topk)
        return res


__all__ = ['recall_at_k', 'median_rank', 'mean_reciprocal_rank', 'bootstrap_recall', 'RetrievalEvaluator',
           'DEFAULT_KS']
