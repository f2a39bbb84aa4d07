"""Zero-shot pathology classification on the HIP path:
``ct_clip/ctclip_inference.py:261-338`` (``CTClipInference.train_step``).

The reference loops volume x pathology: for each of the 18 pathologies it tokenises the pair
("<p> is present.", "<p> is not present.") to 512 tokens, calls ``CTCLIP.forward(text, volume)``
in eval mode (``einsum('b d, b d -> b') * temp`` with the one volume broadcast over the two
prompts, ``ct_clip.py:805-807``), applies ``softmax(dim=0)`` (``ctclip_inference.py:92-104``) and
keeps entry 0 (``:312-315``) -- 18 image-tower encodes and 18 BERT passes per volume.

Here the work is factored without changing a number (eval mode is deterministic):
  * the 2P prompt latents are encoded ONCE (one BERT batch) and cached;
  * each volume batch goes through the image tower + projection ONCE;
  * one HIP kernel (``ctclip_zero_shot``) normalises, scores every (volume, prompt) pair and
    takes the pairwise softmax -> probs [N, P] (the reference's ``predictedall``).
"""
from __future__ import annotations

import torch

from . import functional as Fn
from . import kernels as K
from .ct_clip import require_cls_latents

# ct_clip/ctclip_inference.py:286-290
PATHOLOGIES = ('Medical material', 'Arterial wall calcification', 'Cardiomegaly', 'Pericardial effusion',
               'Coronary artery wall calcification', 'Hiatal hernia', 'Lymphadenopathy', 'Emphysema',
               'Atelectasis', 'Lung nodule', 'Lung opacity', 'Pulmonary Embolism', 'Pleural effusion',
               'Mosaic attenuation pattern', 'Peribronchial thickening', 'Consolidation', 'Bronchiectasis',
               'Interlobular septal thickening')


# the trainer's validation pass scores another list with another prompt pair
# (ct_clip/CTCLIPTrainer.py:378-408): entry 11 is 'Pulmonary fibrotic sequela' there
VALIDATION_PATHOLOGIES = PATHOLOGIES[:11] + ('Pulmonary fibrotic sequela',) + PATHOLOGIES[12:]
INFERENCE_TEMPLATE = ('{} is present.', '{} is not present.')
VALIDATION_TEMPLATE = ('There is {}.', 'There is no {}.')


def prompts(pathologies=PATHOLOGIES, template=INFERENCE_TEMPLATE):
    """The prompt pairs of ``ctclip_inference.py:306``, flattened: rows 2j / 2j+1.  ``template``:
    the (positive, negative) pair of format strings; ``VALIDATION_TEMPLATE`` gives the trainer's
    validation prompts (``CTCLIPTrainer.py:405-408``)."""
    pos, neg = template
    out = []
    for p in pathologies:
        out += [pos.format(p), neg.format(p)]
    return out


class ZeroShotClassifier:
    """``predict(volumes) -> (probs [N, P], scores [N, P, 2])`` for a ``ctclip_mi355x.CTCLIP``.

    Prompts: either ``tokenizer`` (an HF tokenizer, called as the reference does with
    ``padding='max_length', truncation=True, max_length=512``) or pre-tokenised ``text`` (any
    object with ``.input_ids`` / ``.attention_mask`` of 2P rows) via ``set_prompts``."""

    def __init__(self, model, pathologies=PATHOLOGIES, tokenizer=None, max_length=512, template=INFERENCE_TEMPLATE):
        require_cls_latents(model, 'ZeroShotClassifier')
        self.model = model
        self.pathologies = tuple(pathologies)
        self.max_length = max_length
        self.template = tuple(template)
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
        self._text = text
        self._t_raw = text_latents(self.model, text)
        return self

    def refresh(self):
        """Encode the prompts again with the model's current weights (the cached latents are those
        of the weights at ``set_prompts`` time; ``CTClipTrainer.validate`` calls this)."""
        if self._t_raw is None:
            raise RuntimeError('ZeroShotClassifier: no prompts (pass tokenizer= or call set_prompts)')
        return self.set_prompts(self._text)

    def image_latents(self, volumes):
        """Raw projected image latents [N, Dl] (image tower + VQ + pool + to_visual_latent)."""
        return image_latents(self.model, volumes)

    def predict(self, volumes, batch_size=8):
        if self._t_raw is None:
            raise RuntimeError('ZeroShotClassifier: no prompts (pass tokenizer= or call set_prompts)')
        log_temp = self.model.temperature.detach().reshape(1)
        probs, scores = [], []
        for i in range(0, volumes.shape[0], batch_size):
            p, s = K.zero_shot(self._t_raw, self.image_latents(volumes[i:i + batch_size]), log_temp)
            probs.append(p)
            scores.append(s)
        return torch.cat(probs), torch.cat(scores)

    def attribute(self, volumes, **kw):
        """``attribution.ZeroShotAttribution(self).maps(volumes, **kw)``: dict(maps, probs, scores), the
        exact split of each pathology's log-odds over the (t, h, w) token grid (the object, with its
        cached direction weights, is kept)."""
        from .attribution import ZeroShotAttribution
        if getattr(self, '_attribution', None) is None:
            self._attribution = ZeroShotAttribution(self)
        return self._attribution.maps(volumes, **kw)


class _eval:
    """Eval mode for the duration (the VQ codebook must not EMA-update during inference)."""

    def __init__(self, m):
        self.m = m

    def __enter__(self):
        self.was = self.m.training
        self.m.eval()

    def __exit__(self, *exc):
        self.m.train(self.was)


# the eval-mode, no-grad forwards behind ZeroShotClassifier and retrieval.RetrievalEvaluator
def text_latents(m, text):
    """Raw projected text latents [rows, Dl] of ``text`` (``.input_ids`` / ``.attention_mask``): BERT, the
    CLS row, to_text_latent."""
    require_cls_latents(m, 'zero_shot.text_latents')
    with torch.no_grad(), _eval(m):
        enc = m.text_transformer(text.input_ids, attention_mask=text.attention_mask)[0]
        return Fn.TextProjFn.apply(enc[:, 0, :].contiguous(), m.to_text_latent.weight)


def image_latents(m, volumes):
    """Raw projected image latents [N, Dl] (image tower + VQ + pool + to_visual_latent)."""
    require_cls_latents(m, 'zero_shot.image_latents')
    with torch.no_grad(), _eval(m):
        pooled, pooled_b = m.visual_transformer.encode_pooled(volumes)
        W = m.to_visual_latent.weight
        return m._project(W, m._visual_weight_bf16(W), pooled, pooled_b)
