"""Masked-language-model pretraining (ctclip_mi355x/mlm.py), the parts that need no GPU: the public
surface (export, the reference's constructor signature and state_dict keys, ct_clip/mlm.py:36-66), the
refusal of host tensors, the unchanged ``CTCLIP(use_mlm=True)`` refusal, and the fixture
tests/golden/golden_mlm.safetensors (tests/golden/make_golden_mlm.py) checked against its own tensors."""
import inspect
import os

import pytest
import torch
import torch.nn.functional as F
from torch import nn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'golden_mlm.safetensors')
PAD = 0


def test_module_is_exported():
    import ctclip_mi355x
    from ctclip_mi355x import mlm
    assert ctclip_mi355x.MLM is mlm.MLM and issubclass(mlm.MLM, nn.Module)


def test_constructor_defaults_and_state_dict_keys():
    from ctclip_mi355x import MLM
    from ctclip_mi355x.bert import BertConfig, BertModel
    sig = inspect.signature(MLM.__init__)
    names = list(sig.parameters)
    assert names == ['self', 'transformer', 'dim', 'num_tokens', 'mask_prob', 'replace_prob', 'random_token_prob',
                     'mask_token_id', 'pad_token_id', 'mask_ignore_token_ids']
    assert all(sig.parameters[n].kind is inspect.Parameter.KEYWORD_ONLY for n in names[2:])
    defaults = {n: sig.parameters[n].default for n in names[4:]}
    assert defaults == dict(mask_prob=0.15, replace_prob=0.9, random_token_prob=0., mask_token_id=2, pad_token_id=0,
                            mask_ignore_token_ids=[])
    bert = BertModel(BertConfig(vocab_size=50, hidden_size=64, num_hidden_layers=1, num_attention_heads=2,
                                intermediate_size=128, max_position_embeddings=16))
    m = MLM(bert, dim=64, num_tokens=50, mask_ignore_token_ids=[7, 8])
    assert m.mask_ignore_token_ids == {0, 7, 8}       # the pad id joins the ignore set, as the reference's
    assert tuple(m.to_logits.weight.shape) == (50, 64)
    keys = set(m.state_dict())
    assert keys == {'to_logits.weight', 'to_logits.bias'} | {'transformer.' + k for k in bert.state_dict()}
    assert m.mask_state() == 0
    m.set_mask_state(5)
    assert m.mask_state() == 5
    with pytest.raises(ValueError):
        m.set_mask_state(-1)


def test_host_tensors_raise():
    from ctclip_mi355x import MLM

    class _Never(nn.Module):
        def forward(self, *a, **k):
            raise AssertionError('the transformer must not run on host input')
    m = MLM(_Never(), dim=8, num_tokens=20)
    with pytest.raises(ValueError, match='device tensor'):
        m(torch.ones(2, 16, dtype=torch.int64))
    assert m.mask_state() == 0


def test_ctclip_use_mlm_still_raises():
    from ctclip_mi355x.ct_clip import CTCLIP

    class _Tower(nn.Module):
        def forward(self, *a, **k):
            return None
    with pytest.raises(NotImplementedError, match='outside the contrastive hot path'):
        CTCLIP(image_encoder=_Tower(), text_encoder=_Tower(), dim_text=8, dim_image=8, dim_latent=4, use_mlm=True)


def test_fixture_is_self_consistent():
    """Guards the fixture, not the code: the reference's loss is F.cross_entropy of the recorded tensors
    (the stub's table without its CLS column through to_logits, against the recorded labels)."""
    from safetensors.torch import load_file
    g = load_file(GOLDEN)
    B, L = g['ids'].shape
    assert (B, L) == (3, 16) and tuple(g['hidden'].shape) == (3, 17, 64) and tuple(g['weight'].shape) == (257, 64)
    logits = F.linear(g['hidden'][:, 1:], g['weight'], g['bias'])
    loss = F.cross_entropy(logits.transpose(1, 2), g['labels'], ignore_index=PAD)
    assert abs(loss.item() - g['loss'].item()) < 1e-6
    sel = g['labels'] != PAD
    assert torch.equal(g['labels'][sel], g['ids'][sel])
    assert sel.sum(-1).tolist() == [0, 1, 3]
    changed = g['masked_ids'] != g['ids']
    assert bool((g['masked_ids'][changed & sel] == 2).all())
