"""Masked-language-model text pretraining (ct_clip/mlm.py:36-109) on the HIP BERT tower.

Signature and state_dict kept: ``MLM(transformer, *, dim, num_tokens, mask_prob=0.15, replace_prob=0.9,
random_token_prob=0., mask_token_id=2, pad_token_id=0, mask_ignore_token_ids=[])``, the head is
``to_logits = nn.Linear(dim, num_tokens)`` and ``forward(seq, **kwargs)`` returns the scalar loss.

Two deviations from the reference, both because its class cannot run on an external ``BertModel``
(the text tower CT-CLIP uses):

* the reference passes the transformer's output object to ``nn.Linear`` (:97-100).  This build takes the
  hidden states ``transformer(masked_seq, **kwargs)[0]``, (B, L, dim), the way CTCLIP reads its text tower.
* the reference strips a CLS column (:101) that only its built-in ``TextTransformer`` prepends, which
  leaves L - 1 logit rows against L labels.  Here logits and labels cover all L positions and nothing is
  stripped; list the tokenizer's CLS / SEP ids in ``mask_ignore_token_ids`` so they are never masked.

Masking is the reference's ``get_mask_subset_with_prob`` rule -- per row exactly ceil(mask_prob * n_b) of
the n_b positions that are neither pad nor ignored, a uniformly hashed subset -- but on the project's hash
stream instead of torch's generator (as BERT's dropout): one 64-bit seed per call, hashed from
``torch.initial_seed()`` and a per-module call counter (``mask_state`` / ``set_mask_state``), so the step
path has no host RNG call and no device -> host read.  (Where a row's eligible positions do not start at
position 0 the reference's ``mask_excess`` slice admits up to ceil(mask_prob * L) positions, ineligible
ones included; the rule above is the one its comment states.)

The head computes logits for the selected positions only: B * ceil(mask_prob * L) rows of ``num_tokens``
logits instead of B * L (csrc/mlm.hip).  With no selected position in the whole batch the
loss is NaN, as ``F.cross_entropy`` gives when every target is ignored.

Host tensors raise: there is no CPU path.  The class is stand-alone as in the reference; ``CTCLIP(use_mlm=
True)`` still raises.
"""
from __future__ import annotations

import torch
from torch import nn

from . import functional as Fn
from . import kernels as K

_M64 = 2 ** 64 - 1


class MLM(nn.Module):
    def __init__(self, transformer, *, dim, num_tokens, mask_prob=0.15, replace_prob=0.9, random_token_prob=0.,
                 mask_token_id=2, pad_token_id=0, mask_ignore_token_ids=[]):
        super().__init__()
        self.transformer = transformer
        self.mask_prob = mask_prob
        self.replace_prob = replace_prob
        self.num_tokens = num_tokens
        self.random_token_prob = random_token_prob
        self.pad_token_id = pad_token_id
        self.mask_token_id = mask_token_id
        self.mask_ignore_token_ids = set([*mask_ignore_token_ids, pad_token_id])
        self.to_logits = nn.Linear(dim, num_tokens)
        self._mask_calls = 0

    def mask_state(self):
        """The call counter the mask seeds are hashed from: with ``torch.initial_seed()`` it is the whole
        state of the mask stream."""
        return self._mask_calls

    def set_mask_state(self, n):
        """Continue the mask stream after call ``n`` (``mask_state`` of a saved run): the next call draws
        the mask that call n + 1 drew."""
        n = int(n)
        if n < 0:
            raise ValueError(f'MLM.set_mask_state: a call count, got {n}')
        self._mask_calls = n

    def _next_seed(self):
        self._mask_calls += 1
        return ((torch.initial_seed() * 0x2545F4914F6CDD1D + self._mask_calls * 0x9E3779B97F4A7C15)
                ^ 0x94D049BB133111EB) & _M64

    def mask(self, seq):
        """(masked_seq, labels, sel) of one call of the mask stream (kernels.mlm_mask); advances it."""
        if not isinstance(seq, torch.Tensor) or not seq.is_cuda:
            raise ValueError('MLM: token ids must be a device tensor (this package has no CPU path)')
        return K.mlm_mask(seq, seed=self._next_seed(), mask_prob=self.mask_prob, replace_prob=self.replace_prob,
                          random_token_prob=self.random_token_prob, num_tokens=self.num_tokens,
                          mask_token_id=self.mask_token_id, pad_token_id=self.pad_token_id,
                          ignore_ids=self.mask_ignore_token_ids)

    def forward(self, seq, **kwargs):
        masked_seq, labels, sel = self.mask(seq)
        hidden = self.transformer(masked_seq, **kwargs)[0]
        B, L = seq.shape
        if (not isinstance(hidden, torch.Tensor) or tuple(hidden.shape) != (B, L, self.to_logits.in_features)
                or hidden.dtype != torch.float32 or not hidden.is_cuda):
            raise ValueError(f'MLM: transformer(...)[0] must be f32 device hidden states '
                             f'{(B, L, self.to_logits.in_features)}, got '
                             f'{tuple(hidden.shape) if isinstance(hidden, torch.Tensor) else type(hidden)}')
        return Fn.MlmHeadFn.apply(hidden, sel, labels, self.to_logits.weight, self.to_logits.bias)
