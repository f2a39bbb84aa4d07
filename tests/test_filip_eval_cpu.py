"""Evaluation of a use_all_token_embeds model (ctclip_mi355x.token_eval, kernels.filip_scores /
score_ranks, csrc/filip_eval.hip): the float64 restatements the GPU tests (test_gpu_filip_eval.py) measure
the kernels against, checked here against ``test_filip_cpu.filip_ref`` and a sort, and the module surface that
needs no GPU."""
import math
import os
import re
import types

import pytest
import torch

from test_filip_cpu import _tiny_model, filip_ref, ragged_mask

F64 = torch.float64
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------ restatements
def filip_scores_full(t, i, mask, log_temp):
    """t [R, T, Dl], i [V, I, Dl] raw token latents, mask [R, T] (every row with a kept token), in float64:
      tn, in = the tokens scaled to unit length (norm floor 1e-12);  S[x,y,t,i] = exp(log_temp) <tn[x,t], in[y,i]>
      A[x,y] = sum_t mask[x,t] max_i S / max(sum_t mask[x,t], 1e-6);  C[x,y] = mean_i max_{t: mask[x,t]} S
      idx[x,y,t] = the LOWEST i that attains max_i S (-1 at masked t), val[x,y,t] = that maximum (0 at masked t).
    Returns A, C, idx, val and S [R, V, T, I] (for the index checks)."""
    t, i, lt = t.to(F64), i.to(F64), torch.as_tensor(log_temp).to(F64).reshape(())
    m = mask.bool()
    I = i.shape[1]
    tn = t / t.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    inn = i / i.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    S = lt.exp() * torch.einsum('xtd,yid->xyti', tn, inn)
    mx = S.amax(3)                                                               # [x, y, t]
    idx = torch.where(S == mx[..., None], torch.arange(I).view(1, 1, 1, I), I).amin(3)
    mm = m[:, None, :].expand_as(mx)
    mf = m.to(F64)
    A = (mx * mf[:, None, :]).sum(2) / mf.sum(1).clamp_min(1e-6)[:, None]
    C = S.masked_fill(~m[:, None, :, None], -math.inf).amax(2).mean(2)
    return A, C, torch.where(mm, idx, -1), torch.where(mm, mx, 0.0), S


def filip_scores_ref(t, i, mask, log_temp):
    """``filip_scores_full`` without S: A [R, V], C [R, V], idx [R, V, T], val [R, V, T]."""
    return filip_scores_full(t, i, mask, log_temp)[:4]


def score_ranks_ref(S, pair=None):
    """rank_i = #{ j != pair_i : S_ij > S_i,pair_i or (S_ij == S_i,pair_i and j < pair_i) } in float64."""
    S = S.to(F64)
    N, M = S.shape
    pair = torch.arange(N) if pair is None else pair.long()
    sp = S.gather(1, pair[:, None])
    j = torch.arange(M)[None, :]
    before = (S > sp) | ((S == sp) & (j < pair[:, None]))
    return (before & (j != pair[:, None])).sum(1).to(torch.int32)


def scattered_mask(R, T, g):
    """Non-prefix masks: every row keeps a seeded scatter of tokens, at least one."""
    mask = (torch.rand(R, T, generator=g) < 0.4).to(torch.uint8)
    mask[torch.arange(R), torch.randint(0, T, (R,), generator=g)] = 1
    return mask


# ------------------------------------------------------------------------------ the restatements themselves
@pytest.mark.parametrize('shape', [(1, 1, 1, 4), (3, 5, 7, 8), (4, 9, 3, 16)])
def test_scores_ref_equals_the_loss_restatement_on_square_inputs(shape):
    Bg, T, I, Dl = shape
    g = torch.Generator().manual_seed(23 + Bg + T)
    t, i = torch.randn(Bg, T, Dl, generator=g, dtype=F64), torch.randn(Bg, I, Dl, generator=g, dtype=F64)
    lt = torch.tensor(math.log(5.0), dtype=F64)
    for mask in (ragged_mask(Bg, T, g), scattered_mask(Bg, T, g)):
        ref = filip_ref(t, i, mask, lt)
        A, C, idx, val = filip_scores_ref(t, i, mask, lt)
        assert (A - ref['A']).abs().max().item() < 1e-12 and (C - ref['C']).abs().max().item() < 1e-12
        mm = mask.bool()[:, None, :].expand(Bg, Bg, T)
        assert torch.equal(idx[mm], ref['idx_t2i'][mm]) and (idx[~mm] == -1).all() and (val[~mm] == 0).all()
        assert torch.equal(val[mm], ref['S'].amax(3)[mm])


def test_scores_ref_is_rectangular_and_position_invariant():
    g = torch.Generator().manual_seed(3)
    t, i = torch.randn(5, 6, 8, generator=g, dtype=F64), torch.randn(3, 4, 8, generator=g, dtype=F64)
    i[:, 3] = i[:, 1]
    mask = scattered_mask(5, 6, g)
    A, C, idx, val = filip_scores_ref(t, i, mask, 0.5)
    assert A.shape == C.shape == (5, 3) and idx.shape == val.shape == (5, 3, 6)
    assert (idx != 3).all()                                                    # the lowest duplicate wins
    for x in range(5):
        for y in range(3):
            a, c, ix, v = filip_scores_ref(t[x:x + 1], i[y:y + 1], mask[x:x + 1], 0.5)
            assert abs(a.item() - A[x, y].item()) < 1e-14 and abs(c.item() - C[x, y].item()) < 1e-14
            assert torch.equal(ix[0, 0], idx[x, y])


def test_rank_rule_with_duplicate_gallery_rows():
    g = torch.Generator().manual_seed(4)
    q, gal = torch.randn(6, 8, generator=g, dtype=F64), torch.randn(9, 8, generator=g, dtype=F64)
    gal[7] = gal[2]
    gal[5] = gal[2]
    q[1] = q[2] = q[0]                                                         # one query, three equal positives
    S = q @ gal.t()
    pair = torch.tensor([2, 5, 7, 0, 8, 2])
    got = score_ranks_ref(S, pair)
    # the place of the positive in a stable descending sort
    order = torch.sort(S, dim=1, descending=True, stable=True).indices
    want = (order == pair[:, None]).int().argmax(1).to(torch.int32)
    assert torch.equal(got, want)
    assert got[1] == got[0] + 1 and got[2] == got[0] + 2                      # duplicates rank in index order
    assert torch.equal(score_ranks_ref(S[:, :6]), (torch.sort(S[:, :6], dim=1, descending=True, stable=True).indices
                                                   == torch.arange(6)[:, None]).int().argmax(1).to(torch.int32))


# ------------------------------------------------------------------------------ module surface (no GPU)
def test_token_eval_imports_and_refuses_by_name():
    from ctclip_mi355x import kernels, token_eval
    from ctclip_mi355x.token_eval import (TokenRetrievalEvaluator, TokenZeroShotClassifier, token_latents_image,
                                          token_latents_text)
    assert callable(kernels.filip_scores) and callable(kernels.score_ranks)
    assert token_eval.DIRECTIONS == ('t2i', 'i2t', 'mean')
    plain = _tiny_model()
    text = types.SimpleNamespace(input_ids=torch.zeros(2, 4, dtype=torch.long), attention_mask=torch.ones(2, 4))
    for who, make in (('TokenZeroShotClassifier', lambda: TokenZeroShotClassifier(plain)),
                      ('TokenRetrievalEvaluator', lambda: TokenRetrievalEvaluator(plain)),
                      ('token_eval.token_latents_text', lambda: token_latents_text(plain, text)),
                      ('token_eval.token_latents_image', lambda: token_latents_image(plain, torch.zeros(1, 1, 10, 40, 40)))):
        with pytest.raises(NotImplementedError, match=f'{who} without CTCLIP\\(use_all_token_embeds=True\\)'):
            make()
    m = _tiny_model(use_all_token_embeds=True)
    for cls in (TokenZeroShotClassifier, TokenRetrievalEvaluator):
        assert cls(m).direction == 'mean' and cls(m, direction='t2i').direction == 't2i'
        with pytest.raises(ValueError, match='direction is one of'):
            cls(m, direction='both')
    zs = TokenZeroShotClassifier(m, pathologies=('a', 'b'))
    with pytest.raises(RuntimeError, match='no prompts'):
        zs.predict(torch.zeros(1, 1, 10, 40, 40))
    with pytest.raises(ValueError, match='expected 4 prompt rows'):
        zs.set_prompts(text)


def test_more_than_one_rank_is_refused_by_name(monkeypatch):
    from ctclip_mi355x import dist_sync
    from ctclip_mi355x.token_eval import TokenRetrievalEvaluator, TokenZeroShotClassifier
    m = _tiny_model(use_all_token_embeds=True)
    monkeypatch.setattr(dist_sync, 'world_rank', lambda: (2, 0))
    for cls in (TokenZeroShotClassifier, TokenRetrievalEvaluator):
        with pytest.raises(NotImplementedError, match=f'{cls.__name__} under torch.distributed with world size > 1'):
            cls(m)


def test_cls_evaluators_still_refuse_the_model():
    """The one-latent evaluators keep refusing a token model, message unchanged."""
    from ctclip_mi355x.attribution import ZeroShotAttribution
    from ctclip_mi355x.probe import LinearProbeEvaluator
    from ctclip_mi355x.retrieval import RetrievalEvaluator
    from ctclip_mi355x.zero_shot import ZeroShotClassifier
    m = _tiny_model(use_all_token_embeds=True)
    for who, make in (('ZeroShotClassifier', lambda: ZeroShotClassifier(m)),
                      ('RetrievalEvaluator', lambda: RetrievalEvaluator(m)),
                      ('LinearProbeEvaluator', lambda: LinearProbeEvaluator(m)),
                      ('ZeroShotAttribution', lambda: ZeroShotAttribution(types.SimpleNamespace(model=m)))):
        with pytest.raises(NotImplementedError, match=f'{who} with CTCLIP\\(use_all_token_embeds=True\\): the model '
                                                      'has no pooled latent pair'):
            make()


def test_wrapper_argument_checks():
    from ctclip_mi355x import kernels as K
    t, i = torch.zeros(2, 3, 16), torch.zeros(4, 5, 16)
    mask, lt = torch.ones(2, 3, dtype=torch.uint8), torch.zeros(1)
    with pytest.raises(ValueError, match='t_raw \\[R, T, Dl\\] / i_raw \\[V, I, Dl\\]'):
        K.filip_scores(t, torch.zeros(4, 5, 32), mask, lt)
    with pytest.raises(ValueError, match='f32 inputs'):
        K.filip_scores(t.double(), i, mask, lt)
    with pytest.raises(ValueError, match='mask uint8 / bool'):
        K.filip_scores(t, i, torch.ones(2, 4, dtype=torch.uint8), lt)
    mask[1] = 0
    with pytest.raises(ValueError, match='without a kept token'):
        K.filip_scores(t, i, mask, lt)
    with pytest.raises(ValueError, match='scores \\[N, M\\]'):
        K.score_ranks(torch.zeros(3))
    with pytest.raises(ValueError, match='expected a device tensor'):
        K.score_ranks(torch.zeros(3, 3))


def test_new_symbols_are_declared():
    hdr = open(os.path.join(REPO, 'include', 'ctclip_hip.h')).read()
    names = set(re.findall(r'\b(?:int|int64_t)\s+(ctclip_\w+)\s*\(', hdr))
    assert {'ctclip_filip_scores', 'ctclip_filip_scores_ws_bytes', 'ctclip_score_ranks'} <= names
    assert 'ctclip_filip_scores_args' in hdr and re.search(r'#define CTCLIP_ABI_VERSION 2\b', hdr)
    from ctclip_mi355x import _lib
    for n in ('ctclip_filip_scores', 'ctclip_filip_scores_ws_bytes', 'ctclip_score_ranks'):
        assert n in _lib._SIGS
    assert _lib._RESTYPES['ctclip_filip_scores_ws_bytes'] is _lib.c_i64
    fields = [f for f, _ in _lib.FilipScoresArgs._fields_]
    assert fields == ['t_raw', 'i_raw', 'mask', 'log_temp', 'R', 'V', 'T', 'I', 'Dl', 'pad', 'A', 'C', 'idx_t2i',
                      'val_t2i', 'ws', 'ws_bytes']
