"""Evaluation of a ``CTCLIP(use_all_token_embeds=True)`` model: zero-shot classification and report <->
volume retrieval on the token-wise (FILIP) scores the model was trained on.

Such a model has no pooled latent pair, so ``zero_shot.ZeroShotClassifier`` and
``retrieval.RetrievalEvaluator`` refuse it (``ct_clip.require_cls_latents``).  Here a report and a volume are
scored as the fine-grained loss scores them: with ``S`` the temperature-scaled similarity of every
kept report token with every spatial image token,

    A[x, y] = mean over the kept tokens t of max_i S        (text -> image)
    C[x, y] = mean over the image tokens i of max_t S       (image -> text)

``kernels.filip_scores`` (csrc/filip_eval.hip) forms both from one exact-f32 product, forward only, for an
unpaired rectangle of reports x volumes, and its entries do not depend on how the rectangle is cut into
calls: the evaluators below score in blocks and get the bits of one call over everything.
``direction``: ``'t2i'`` scores with A, ``'i2t'`` with C, ``'mean'`` with (A + C) / 2.
"""
from __future__ import annotations

import types

import torch

from . import dist_sync
from . import functional as Fn
from . import kernels as K
from .retrieval import DEFAULT_KS, _batches, _direction
from .zero_shot import INFERENCE_TEMPLATE, PATHOLOGIES, _eval, prompts

DIRECTIONS = ('t2i', 'i2t', 'mean')


def require_token_latents(model, who):
    """The token evaluators score projected tokens: a model without ``use_all_token_embeds`` (whose heads
    project one pooled latent) is refused by name, and so is more than one rank (as the loss is)."""
    if not getattr(model, 'use_all_token_embeds', False):
        raise NotImplementedError(f'{who} without CTCLIP(use_all_token_embeds=True): the model projects one pooled '
                                  'latent per report and volume (use zero_shot / retrieval)')
    if dist_sync.world_rank()[0] > 1:
        raise NotImplementedError(f'{who} under torch.distributed with world size > 1 (the token latents are not '
                                  'gathered)')


def _check_direction(direction, who):
    if direction not in DIRECTIONS:
        raise ValueError(f'{who}: direction is one of {DIRECTIONS}, got {direction!r}')
    return direction


def _pick(out, direction):
    """The score matrix of ``direction`` from ``kernels.filip_scores``' dict."""
    if direction == 't2i':
        return out['A']
    if direction == 'i2t':
        return out['C']
    return (out['A'] + out['C']) / 2


# the eval-mode, no-grad forwards of CTCLIP._forward_filip
def token_latents_text(model, text):
    """Raw projected text token latents [rows, T, Dl] of ``text`` (``.input_ids`` / ``.attention_mask``):
    BERT, to_text_latent on every token."""
    require_token_latents(model, 'token_eval.token_latents_text')
    with torch.no_grad(), _eval(model):
        enc = model.text_transformer(text.input_ids, attention_mask=text.attention_mask)[0]
        B, T, dt = enc.shape
        W = model.to_text_latent.weight
        return Fn.TextProjFn.apply(enc.reshape(B * T, dt).contiguous(), W).view(B, T, W.shape[0])


def token_latents_image(model, volumes):
    """Raw projected image token latents [N, h w, Dl]: image tower + VQ + mean over t, the pooled volume
    viewed [N, h w, d], to_visual_latent on every token."""
    require_token_latents(model, 'token_eval.token_latents_image')
    with torch.no_grad(), _eval(model):
        pooled, _ = model.visual_transformer.encode_pooled(volumes)
        W = model.to_visual_latent.weight
        B, d = pooled.shape[0], W.shape[1]
        tokens = pooled.view(B, -1, d)
        I = tokens.shape[1]
        return Fn.TextProjFn.apply(tokens.reshape(B * I, d).contiguous(), W).view(B, I, W.shape[0])


def _key_mask(text):
    return (text.attention_mask != 0).to(torch.uint8).contiguous()


class TokenZeroShotClassifier:
    """``zero_shot.ZeroShotClassifier``'s interface on the token-wise scores: ``predict(volumes) ->
    (probs [N, P], scores [N, P, 2])``, ``scores[n, j]`` the (present, not present) prompt pair of pathology j
    against volume n under ``direction``, ``probs`` the pair's softmax, entry 0 (``kernels.zero_shot``'s rule).
    ``ground(volumes)`` says where each prompt word points in the volume.  Works with
    ``evaluate.ZeroShotEvaluator`` and ``CTClipTrainer.validate`` as the CLS classifier does."""

    def __init__(self, model, pathologies=PATHOLOGIES, tokenizer=None, max_length=512, template=INFERENCE_TEMPLATE,
                 direction='mean'):
        require_token_latents(model, 'TokenZeroShotClassifier')
        self.model = model
        self.pathologies = tuple(pathologies)
        self.max_length = max_length
        self.template = tuple(template)
        self.direction = _check_direction(direction, 'TokenZeroShotClassifier')
        self._t_raw = None
        if tokenizer is not None:
            dev = next(model.parameters()).device
            self.set_prompts(tokenizer(prompts(self.pathologies, self.template), return_tensors='pt',
                                       padding='max_length', truncation=True, max_length=max_length).to(dev))

    def set_prompts(self, text):
        ids = text.input_ids
        if ids.shape[0] != 2 * len(self.pathologies):
            raise ValueError(f'expected {2 * len(self.pathologies)} prompt rows (a present / not present pair '
                             f'per pathology), got {ids.shape[0]}')
        mask = _key_mask(text)
        if not bool(mask.any(1).all()):
            raise ValueError('TokenZeroShotClassifier: a prompt without a kept token (an all-zero attention_mask row)')
        self._text = text
        self._mask = mask
        self._t_raw = token_latents_text(self.model, text)
        return self

    def refresh(self):
        """Encode the prompts again with the model's current weights (``CTClipTrainer.validate`` calls this)."""
        self._require_prompts()
        return self.set_prompts(self._text)

    def _require_prompts(self):
        if self._t_raw is None:
            raise RuntimeError('TokenZeroShotClassifier: no prompts (pass tokenizer= or call set_prompts)')

    def image_latents(self, volumes):
        """Raw projected image token latents [N, h w, Dl]."""
        return token_latents_image(self.model, volumes)

    def _score(self, volumes, want_idx):
        log_temp = self.model.temperature.detach().reshape(1)
        return K.filip_scores(self._t_raw, self.image_latents(volumes), self._mask, log_temp, want_idx=want_idx)

    def predict(self, volumes, batch_size=8):
        self._require_prompts()
        P = len(self.pathologies)
        probs, scores = [], []
        for i in _batches(volumes.shape[0], batch_size):
            s = _pick(self._score(volumes[i:i + batch_size], False), self.direction)      # [2P, n]
            s = s.t().reshape(-1, P, 2).contiguous()
            # kernels.zero_shot's rule: the pair's softmax with the maximum subtracted, entry 0
            e = (s - s.amax(2, keepdim=True)).exp()
            probs.append(e[..., 0] / (e[..., 0] + e[..., 1]))
            scores.append(s)
        return torch.cat(probs), torch.cat(scores)

    def ground(self, volumes, batch_size=8):
        """Where each prompt word points: dict(``idx`` int32 [N, P, 2, T], the image token (row-major in the
        (h, w) ``grid``) that scores highest with each prompt token, the lowest index on ties, -1 at padding;
        ``score`` f32 [N, P, 2, T], that score, 0 at padding; ``grid`` = (h, w))."""
        self._require_prompts()
        P, T = len(self.pathologies), self._t_raw.shape[1]
        idx, val = [], []
        for i in _batches(volumes.shape[0], batch_size):
            out = self._score(volumes[i:i + batch_size], True)
            idx.append(out['idx_t2i'].permute(1, 0, 2).reshape(-1, P, 2, T))
            val.append(out['val_t2i'].permute(1, 0, 2).reshape(-1, P, 2, T))
        return dict(idx=torch.cat(idx), score=torch.cat(val), grid=tuple(self.model.visual_transformer.patch_height_width))


class TokenRetrievalEvaluator:
    """``retrieval.RetrievalEvaluator`` on the token-wise scores of a ``use_all_token_embeds`` model."""

    def __init__(self, model, direction='mean'):
        require_token_latents(model, 'TokenRetrievalEvaluator')
        self.model = model
        self.direction = _check_direction(direction, 'TokenRetrievalEvaluator')

    def text_latents(self, text, batch_size=8):
        """Raw text token latents [R, T, Dl] of ``text`` (``.input_ids`` / ``.attention_mask`` of R rows)."""
        ids, mask = text.input_ids, text.attention_mask
        return torch.cat([token_latents_text(self.model, types.SimpleNamespace(input_ids=ids[i:i + batch_size],
                                                                               attention_mask=mask[i:i + batch_size]))
                          for i in _batches(ids.shape[0], batch_size)])

    def image_latents(self, volumes, batch_size=8):
        """Raw image token latents [V, h w, Dl]; volumes: a (V, 1, D, H, W) tensor or an iterable of batches."""
        if isinstance(volumes, torch.Tensor):
            volumes = [volumes]
        return torch.cat([token_latents_image(self.model, v[i:i + batch_size]) for v in volumes
                          for i in _batches(v.shape[0], batch_size)])

    def scores(self, t, v, mask, report_block=64, volume_block=64):
        """The score matrix [R, V] of ``direction``, in ``report_block`` x ``volume_block`` kernel calls (the
        same bits whatever the blocks)."""
        if report_block < 1 or volume_block < 1 or max(report_block, volume_block) > K.FILIP_SCORES_MAX_ROWS:
            raise ValueError(f'TokenRetrievalEvaluator: blocks of 1 .. {K.FILIP_SCORES_MAX_ROWS} rows, got '
                             f'{report_block} x {volume_block}')
        log_temp = self.model.temperature.detach().reshape(1)
        R, V = t.shape[0], v.shape[0]
        S = torch.empty(R, V, device=t.device, dtype=torch.float32)
        for r0 in range(0, R, report_block):
            for v0 in range(0, V, volume_block):
                out = K.filip_scores(t[r0:r0 + report_block], v[v0:v0 + volume_block], mask[r0:r0 + report_block],
                                     log_temp)
                S[r0:r0 + report_block, v0:v0 + volume_block] = _pick(out, self.direction)
        return S

    def evaluate(self, volumes, text, pair=None, ks=DEFAULT_KS, n_boot=0, topk=0, batch_size=8, report_block=64,
                 volume_block=64):
        """``RetrievalEvaluator.evaluate``'s arguments and result dict; ``text_latents`` [R, T, Dl] and
        ``image_latents`` [V, h w, Dl] hold the raw token latents that were scored.  Ranks follow the same rule
        (higher scores first, of equal scores the lower gallery index), from the score matrix
        (``kernels.score_ranks``); with topk > 0, ``score`` / ``idx`` [queries, topk] are the head of a stable
        descending sort of it."""
        mask = _key_mask(text)
        if not bool(mask.any(1).all()):
            raise ValueError('TokenRetrievalEvaluator: a report without a kept token (an all-zero attention_mask row)')
        t = self.text_latents(text, batch_size)
        v = self.image_latents(volumes, batch_size)
        R, V = t.shape[0], v.shape[0]
        if pair is None and R != V:
            raise ValueError(f'TokenRetrievalEvaluator: pair=None pairs report i with volume i, but there are {R} '
                             f'reports and {V} volumes')
        if topk and not 1 <= topk <= min(R, V):
            raise ValueError(f'TokenRetrievalEvaluator: 1 <= topk <= min(reports, volumes) = {min(R, V)}, got {topk}')
        S = self.scores(t, v, mask, report_block, volume_block)
        St = S.t().contiguous()
        if pair is None:
            r2v = K.score_ranks(S)
            v2r = K.score_ranks(St)
        else:
            pair = torch.as_tensor(pair).to(t.device)
            r2v = K.score_ranks(S, pair)
            # one query per report: its volume against all reports.  The volume's best-ranked own report
            # has none of its other reports above it, so its place there is the volume's rank
            per_report = K.score_ranks(St[pair.long()])
            v2r = torch.full((V,), R, device=t.device, dtype=torch.int32)
            v2r = v2r.scatter_reduce(0, pair.long(), per_report, 'amin')
            v2r = torch.where(v2r == R, torch.full_like(v2r, -1), v2r)
        res = dict(text_latents=t, image_latents=v, report_to_volume=_direction(r2v, ks, n_boot),
                   volume_to_report=_direction(v2r, ks, n_boot))
        if topk:
            for name, M in (('report_to_volume', S), ('volume_to_report', St)):
                val, idx = torch.sort(M, dim=1, descending=True, stable=True)
                res[name]['score'], res[name]['idx'] = val[:, :topk].contiguous(), idx[:, :topk].to(torch.int32)
        return res


__all__ = ['token_latents_text', 'token_latents_image', 'TokenZeroShotClassifier', 'TokenRetrievalEvaluator',
           'require_token_latents', 'DIRECTIONS']
