"""Retrieval evaluation on the HIP path: given a report, how high does its own volume rank among all
volumes, and the other way round -- the report-to-volume Recall@5/10/50/100 CT-CLIP's evaluation
reports beside the zero-shot AUROC.

The latents come from the forwards ``zero_shot.ZeroShotClassifier`` uses (eval mode, no grad); the
ranking runs in two HIP kernels (csrc/retrieval.hip) that never write the N x M score matrix:
``kernels.retrieval_ranks`` (the 0-based place of each query's positive in a stable descending sort
of its scores) and ``kernels.retrieval_topk``.  Ties are the normal case (radiology reports repeat
verbatim): among equal scores the lower gallery index ranks first, in both kernels.

The metric functions below are plain torch on the rank vector and work on any device.

Volume-to-volume ("case") retrieval, the third part of CT-CLIP's evaluation, is ``CaseRetrievalEvaluator``:
volumes are ranked against volumes and scored by their pathology labels (MAP@K, precision@K, mean Jaccard@K)
in one fused pass, ``kernels.case_retrieval`` (csrc/case_retrieval.hip), which can leave gallery rows out per
query (the query itself, other reconstructions of its scan, other scans of its patient).
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


def _image_latents(model, volumes, batch_size):
    if isinstance(volumes, torch.Tensor):
        volumes = [volumes]
    return torch.cat([Z.image_latents(model, v[i:i + batch_size]) for v in volumes
                      for i in _batches(v.shape[0], batch_size)])


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
        return _image_latents(self.model, volumes, batch_size)

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


# ------------------------------------------------------------------------------------ case retrieval
DEFAULT_CASE_KS = (1, 5, 10, 50)


def pack_labels(labels):
    """[N, C] labels of 0 / 1 (any integer, bool or float dtype, C <= 64) -> [N] int64 bitmasks, bit c = label
    c present: what ``kernels.case_retrieval`` takes.  Any other value raises ValueError (one host read for
    a device tensor)."""
    y = torch.as_tensor(labels)
    if y.dim() != 2 or y.shape[1] > 64 or y.is_complex():
        raise ValueError(f'pack_labels: labels must be [N, C] with C <= 64, got {tuple(y.shape)} {y.dtype}')
    if y.numel() and not bool(((y == 0) | (y == 1)).all()):
        raise ValueError('pack_labels: labels must be 0 or 1')
    # distinct bits never carry, so the sum is the OR; bit 63 lands in the sign, as in the kernel's word
    shifts = torch.arange(y.shape[1], device=y.device, dtype=torch.int64)
    return ((y != 0).long() << shifts[None, :]).sum(1)


def _table(x, name, floating):
    t = torch.as_tensor(x)
    if t.dim() != 2 or t.shape[0] == 0 or t.is_floating_point() != floating:
        raise ValueError(f'{name} must be a non-empty [N, len(ks)] {"float64" if floating else "integer"} table, '
                         f'got {tuple(t.shape)} {t.dtype}')
    return t


def _places(filled, ks, n):
    """[N, len(ks)] int64 on the host: min(K_a, filled_i), the places a query's list has up to K_a."""
    f = torch.as_tensor(filled)
    if f.dim() != 1 or f.shape[0] != n or f.is_floating_point():
        raise ValueError(f'filled must be {n} integer counts, got {tuple(f.shape)} {f.dtype}')
    return torch.minimum(f.long().cpu()[:, None], torch.as_tensor(list(ks), dtype=torch.long)[None, :])


def map_at_k(ap):
    """(MAP@K [len(ks)] f64 on the host, n_scored): the mean of ``ap`` [N, len(ks)] over the queries that
    have an AP -- rows of -1 (no relevant visible gallery row) are left out, n_scored counts the rest.  The
    f64 values are summed on the host (one answer whatever the device) and divided once; NaN if n_scored
    is 0."""
    a = _table(ap, 'map_at_k: ap', True).detach().cpu().double()
    keep = a[:, 0] != -1.0 if a.shape[1] else torch.zeros(a.shape[0], dtype=torch.bool)
    n = int(keep.sum())
    return a[keep].sum(0) / n if n else torch.full((a.shape[1],), float('nan'), dtype=torch.float64), n


def precision_at_k(hits, filled, ks):
    """Precision@K [len(ks)] f64 on the host: the relevant share of all places the lists have up to K,
    sum_i hits[i, a] / sum_i min(K_a, filled_i) -- two integer counts and one division.  With every list full
    that is the mean of hits / K; a query whose list is shorter than K (a small gallery, a large group) is
    not charged for places it cannot fill.  NaN if no list has a place."""
    h = _table(hits, 'precision_at_k: hits', False)
    den = _places(filled, ks, h.shape[0]).sum(0)
    return h.long().sum(0).cpu().double() / den.double()


def mean_jaccard_at_k(gain, filled, ks):
    """Mean Jaccard@K [len(ks)] f64 on the host: the mean graded relevance of all places the lists have up
    to K, sum_i gain[i, a] / sum_i min(K_a, filled_i); the f64 gains are summed on the host, divided once."""
    g = _table(gain, 'mean_jaccard_at_k: gain', True).detach().cpu().double()
    return g.sum(0) / _places(filled, ks, g.shape[0]).sum(0).double()


def bootstrap_case(per_query, n_samples=1000, places=None):
    """[n_samples, len(ks)] f64 (host): a per-query table [N, len(ks)] under ``evaluate.bootstrap_indices``'
    resamples of the QUERIES (the gallery, and so every query's list, stays fixed); ``evaluate.compute_cis``
    takes the result.  ``places=None``: ``per_query`` is ``ap`` and a row is the mean over its drawn queries
    that have an AP (-1 rows left out; NaN if none is drawn) -- ``map_at_k`` of the resample.  With
    ``places`` [N, len(ks)] (min(K, filled)): ``per_query`` is ``hits`` or ``gain`` and a row is the drawn sum
    over the drawn places -- ``precision_at_k`` / ``mean_jaccard_at_k`` of the resample."""
    v = torch.as_tensor(per_query)
    if v.dim() != 2 or v.shape[0] == 0:
        raise ValueError(f'bootstrap_case: per_query must be a non-empty [N, len(ks)] table, got {tuple(v.shape)}')
    v = v.detach().cpu().double()
    rows = torch.from_numpy(bootstrap_indices(v.shape[0], n_samples)).long()
    if places is None:
        keep = (v != -1.0).double()
        return (v * keep)[rows].sum(1) / keep[rows].sum(1)
    den = torch.as_tensor(places).cpu().double()
    if den.shape != v.shape:
        raise ValueError(f'bootstrap_case: places {tuple(den.shape)} for a table {tuple(v.shape)}')
    return v[rows].sum(1) / den[rows].sum(1)


class CaseRetrievalEvaluator:
    """Volume-to-volume retrieval of a ``ctclip_mi355x.CTCLIP`` scored by pathology labels: MAP@K,
    precision@K and mean Jaccard@K, the retrieval table of CT-CLIP's evaluation.

    Not provided, and refused by name where a caller can ask: token-wise (``use_all_token_embeds``) case
    retrieval, nDCG, K above 128.  The gallery is not sharded over ranks: each rank evaluates what it is
    passed."""

    def __init__(self, model):
        require_cls_latents(model, 'CaseRetrievalEvaluator')
        self.model = model

    def image_latents(self, volumes, batch_size=8):
        """Raw image latents [V, Dl]; volumes: a (V, 1, D, H, W) tensor or an iterable of such batches."""
        return _image_latents(self.model, volumes, batch_size)

    @staticmethod
    def _labels(labels, n, device, who):
        y = torch.as_tensor(labels)
        y = pack_labels(y) if y.dim() == 2 else y
        if y.dim() != 1 or y.shape[0] != n or y.dtype != torch.int64:
            raise ValueError(f'CaseRetrievalEvaluator: {who} must be [{n}, C] 0 / 1 labels or {n} int64 bitmasks, '
                             f'got {tuple(y.shape)} {y.dtype}')
        return y.to(device).contiguous()

    @staticmethod
    def _groups(groups, n, device, who):
        r = torch.as_tensor(groups)
        if r.dim() != 1 or r.shape[0] != n or r.is_floating_point():
            raise ValueError(f'CaseRetrievalEvaluator: {who} must be {n} integer group ids, got {tuple(r.shape)} '
                             f'{r.dtype}')
        return r.to(device=device, dtype=torch.int32).contiguous()

    def evaluate(self, volumes, labels, groups=None, gallery_volumes=None, gallery_labels=None, gallery_groups=None,
                 ks=DEFAULT_CASE_KS, rel='any', n_boot=0, batch_size=8, exclude_self=True):
        """Rank ``gallery_volumes`` for every one of ``volumes`` and score the lists by the labels.

        ``labels`` [N, C] 0 / 1 (C <= 64) or [N] int64 bitmasks (``pack_labels``).  ``groups`` [N] integer ids:
        a query never sees a gallery row of its own group (the scan's other reconstructions, the patient's
        other scans); a negative id excludes nothing.  Without ``gallery_volumes`` the queries are the
        gallery (``gallery_labels`` / ``gallery_groups`` must be None then), and with ``groups=None`` and
        ``exclude_self`` every volume is its own group, so a query skips itself.  With a separate gallery
        pass ``gallery_labels``, and ``groups`` / ``gallery_groups`` together or not at all.

        ``rel``: 'any' (a shared label, or both without any) or 'exact' (equal label sets) decides what counts
        as relevant for MAP and precision; the graded measure is always the Jaccard index of the two sets.

        Returns a dict: ``image_latents`` [N, Dl] (and ``gallery_latents`` [M, Dl] with a separate gallery);
        the kernel's ``idx``, ``score``, ``filled``, ``nrel``, ``hits``, ``ap``, ``gain`` (on the device);
        ``ks``; ``map``, ``precision``, ``mean_jaccard`` ([len(ks)] f64 on the host); ``n_scored``, the queries
        with an AP (those without a relevant visible gallery row are left out of ``map``); ``ci``: None, or
        with n_boot > 0 a dict of ``compute_cis``' [3, len(ks)] mean / lower / upper tables for ``map``,
        ``precision`` and ``mean_jaccard`` over n_boot resamples of the queries."""
        own = gallery_volumes is None
        if own and (gallery_labels is not None or gallery_groups is not None):
            raise ValueError('CaseRetrievalEvaluator: gallery_labels / gallery_groups without gallery_volumes (the '
                             'queries are the gallery then, with their own labels and groups)')
        if not own and gallery_labels is None:
            raise ValueError('CaseRetrievalEvaluator: gallery_volumes needs gallery_labels')
        if not own and (groups is None) != (gallery_groups is None):
            raise ValueError('CaseRetrievalEvaluator: groups and gallery_groups come together')
        q = self.image_latents(volumes, batch_size).contiguous()
        N, dev = q.shape[0], q.device
        qlab = self._labels(labels, N, dev, 'labels')
        if own:
            g, glab = q, qlab
            if groups is not None:
                qgrp = self._groups(groups, N, dev, 'groups')
            else:
                qgrp = torch.arange(N, device=dev, dtype=torch.int32) if exclude_self else None
            ggrp = qgrp
        else:
            g = self.image_latents(gallery_volumes, batch_size).contiguous()
            glab = self._labels(gallery_labels, g.shape[0], dev, 'gallery_labels')
            qgrp = None if groups is None else self._groups(groups, N, dev, 'groups')
            ggrp = None if groups is None else self._groups(gallery_groups, g.shape[0], dev, 'gallery_groups')
        r = K.case_retrieval(q, g, qlab, glab, qgrp, ggrp, ks=ks, rel=rel)
        res = dict(image_latents=q, idx=r.idx, score=r.score, filled=r.filled, nrel=r.nrel, hits=r.hits, ap=r.ap,
                   gain=r.gain, ks=r.ks)
        if not own:
            res['gallery_latents'] = g
        res['map'], res['n_scored'] = map_at_k(r.ap)
        res['precision'] = precision_at_k(r.hits, r.filled, r.ks)
        res['mean_jaccard'] = mean_jaccard_at_k(r.gain, r.filled, r.ks)
        res['ci'] = None
        if n_boot:
            places = _places(r.filled, r.ks, N)
            res['ci'] = dict(map=compute_cis(bootstrap_case(r.ap, n_boot)),
                             precision=compute_cis(bootstrap_case(r.hits, n_boot, places)),
                             mean_jaccard=compute_cis(bootstrap_case(r.gain, n_boot, places)))
        return res


__all__ = ['recall_at_k', 'median_rank', 'mean_reciprocal_rank', 'bootstrap_recall', 'RetrievalEvaluator',
           'DEFAULT_KS', 'pack_labels', 'map_at_k', 'precision_at_k', 'mean_jaccard_at_k', 'bootstrap_case',
           'CaseRetrievalEvaluator', 'DEFAULT_CASE_KS']
