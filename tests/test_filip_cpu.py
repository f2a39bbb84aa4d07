"""The fine-grained (FILIP) token-wise contrastive loss of CTCLIP(use_all_token_embeds=True)
(ct_clip/ct_clip.py:751-755, 829-878), restated in float64.  The reference cannot run its own branch
(the image tokens are flattened before the ndim == 3 assert), so there is no golden fixture: the
yardstick is ``filip_ref`` below, checked here against torch.autograd through the direct expression and
against the CLS loss restatement at T = I = 1.  The GPU tests (test_gpu_filip.py) check the HIP kernel
against it."""
import math
import types

import pytest
import torch
import torch.nn.functional as F

from test_loss_options_cpu import general_loss

F64 = torch.float64


# ------------------------------------------------------------------------------ restatement
def filip_ref(t_raw, i_raw, mask, log_temp, decoupled=False, i2t_over_text=False, idx=None):
    """t_raw [Bg, T, Dl], i_raw [Bg, I, Dl] raw token latents, mask [Bg, T], in float64:
      tn, in = the tokens scaled to unit length (norm floor 1e-12);  S[x,y,t,i] = exp(log_temp) <tn[x,t], in[y,i]>
      A[x,y] = sum_t mask[x,t] max_i S / max(sum_t mask[x,t], 1e-6);  C[x,y] = mean_i max_{t: mask[x,t]} S
      loss = 1/2 [mean_x(-log(e^A_xx + 1e-20) + log(sum_y e^A_xy + 1e-20)) + the same with C]; the C
      denominator runs over y (images; the reference), or over x with ``i2t_over_text``; ``decoupled``
      leaves the diagonal out of the denominators.
    A max belongs to the LOWEST index that attains it, and so does its whole gradient; with
    ``idx = (idx_t2i [Bg,Bg,T], idx_i2t [Bg,Bg,I])`` the routes are those indices instead.
    Returns a dict: loss, dt, di, dlt (analytic gradients), A, C, idx_t2i, idx_i2t, S."""
    t_raw, i_raw, lt = t_raw.to(F64), i_raw.to(F64), log_temp.to(F64).reshape(())
    m = mask.bool()
    Bg, T, _ = t_raw.shape
    I = i_raw.shape[1]
    nt, ni = t_raw.norm(dim=-1, keepdim=True), i_raw.norm(dim=-1, keepdim=True)
    tn, inn = t_raw / nt.clamp_min(1e-12), i_raw / ni.clamp_min(1e-12)
    temp = lt.exp()
    S = temp * torch.einsum('xtd,yid->xyti', tn, inn)
    if idx is None:
        it = torch.where(S == S.amax(3, keepdim=True), torch.arange(I).view(1, 1, 1, I), I).amin(3)
        Sm = S.masked_fill(~m[:, None, :, None], -math.inf)
        ii = torch.where(Sm == Sm.amax(2, keepdim=True), torch.arange(T).view(1, 1, T, 1), T).amin(2)
    else:
        it, ii = idx[0].long().clamp_min(0), idx[1].long()       # -1 marks a masked text token
    vt = S.gather(3, it[..., None]).squeeze(3)                   # [x, y, t]
    vi = S.gather(2, ii[:, :, None, :]).squeeze(2)               # [x, y, i]
    mf = m.to(F64)
    cnt = mf.sum(1).clamp_min(1e-6)
    A = (vt * mf[:, None, :]).sum(2) / cnt[:, None]
    C = vi.mean(2)
    eye = torch.eye(Bg, dtype=F64)
    off = 1.0 - eye if decoupled else torch.ones_like(eye)

    def direction(M, over_rows):
        """loss and d loss / d M of one direction; the denominator sums over the column index, or over
        the row index with ``over_rows``"""
        e = M.exp()
        tot = (e * off).sum(0 if over_rows else 1)
        own = e.diagonal()
        loss = (torch.log(tot + 1e-20) - torch.log(own + 1e-20)).mean()
        den = (tot + 1e-20)[None, :] if over_rows else (tot + 1e-20)[:, None]
        g = (e * off) / den - eye * (e / (e + 1e-20))
        return loss, g / Bg

    la, dA = direction(A, False)
    lc, dC = direction(C, i2t_over_text)
    dA, dC = 0.5 * dA, 0.5 * dC
    loss = 0.5 * (la + lc)
    dlt = (dA * A + dC * C).sum()
    wA = dA[:, :, None] * mf[:, None, :] / cnt[:, None, None]    # [x, y, t]
    wC = (dC[:, :, None] / I).expand(Bg, Bg, I)                   # [x, y, i]
    dS = torch.zeros_like(S)
    dS.scatter_add_(3, it[..., None], wA[..., None])
    dS.scatter_add_(2, ii[:, :, None, :], wC[:, :, None, :].contiguous())
    dtn = temp * torch.einsum('xyti,yid->xtd', dS, inn)
    din = temp * torch.einsum('xyti,xtd->yid', dS, tn)

    def unnorm(g, u, n):        # the l2norm backward; below the floor the latent is x / 1e-12, linear
        return torch.where(n > 1e-12, (g - u * (g * u).sum(-1, keepdim=True)) / n.clamp_min(1e-12), g / 1e-12)

    return dict(loss=loss, dt=unnorm(dtn, tn, nt), di=unnorm(din, inn, ni), dlt=dlt, A=A, C=C, idx_t2i=it,
                idx_i2t=ii, S=S)


def filip_direct(t_raw, i_raw, mask, log_temp, decoupled=False, i2t_over_text=False):
    """The same loss written with torch's own amax (for autograd on tie-free inputs)."""
    m = mask.bool()
    tn, inn = F.normalize(t_raw, dim=-1), F.normalize(i_raw, dim=-1)
    S = log_temp.exp() * torch.einsum('xtd,yid->xyti', tn, inn)
    mf = m.to(S.dtype)
    A = (S.amax(3) * mf[:, None, :]).sum(2) / mf.sum(1).clamp_min(1e-6)[:, None]
    C = S.masked_fill(~m[:, None, :, None], -torch.finfo(S.dtype).max).amax(2).mean(2)
    Bg = A.shape[0]
    off = 1.0 - torch.eye(Bg, dtype=S.dtype) if decoupled else torch.ones(Bg, Bg, dtype=S.dtype)

    def direction(M, over_rows):
        e = M.exp()
        return (torch.log((e * off).sum(0 if over_rows else 1) + 1e-20) - torch.log(e.diagonal() + 1e-20)).mean()

    return 0.5 * (direction(A, False) + direction(C, i2t_over_text))


def ragged_mask(Bg, T, g):
    """Row 0: the single token T - 1; row 1: every token; the rest: a seeded prefix of at least one."""
    mask = torch.zeros(Bg, T, dtype=torch.uint8)
    for b in range(Bg):
        if b == 0:
            mask[b, T - 1] = 1
        elif b == 1:
            mask[b] = 1
        else:
            mask[b, :int(torch.randint(1, T + 1, (1,), generator=g))] = 1
    return mask


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


# ------------------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize('over_text', [False, True])
@pytest.mark.parametrize('dcl', [False, True])
@pytest.mark.parametrize('shape', [(1, 1, 1, 4), (3, 5, 7, 8), (4, 9, 3, 16)])
def test_analytic_gradients_equal_autograd(shape, dcl, over_text):
    Bg, T, I, Dl = shape
    g = torch.Generator().manual_seed(17 + Bg + T)
    t = torch.randn(Bg, T, Dl, generator=g, dtype=F64).requires_grad_(True)
    i = torch.randn(Bg, I, Dl, generator=g, dtype=F64).requires_grad_(True)
    lt = torch.tensor(math.log(5.0), dtype=F64, requires_grad=True)
    mask = ragged_mask(Bg, T, g)
    loss = filip_direct(t, i, mask, lt, dcl, over_text)
    loss.backward()
    r = filip_ref(t.detach(), i.detach(), mask, lt.detach(), dcl, over_text)
    assert abs(r['loss'].item() - loss.item()) < 1e-12 * max(1.0, abs(loss.item()))
    assert rel(r['dt'], t.grad) < 1e-9 and rel(r['di'], i.grad) < 1e-9
    assert abs(r['dlt'].item() - lt.grad.item()) < 1e-9 * max(1e-3, abs(lt.grad.item()))
    assert (r['dt'][~mask.bool()] == 0).all()                    # masked text tokens take no part
    # forcing the restatement's own indices changes nothing
    r2 = filip_ref(t.detach(), i.detach(), mask, lt.detach(), dcl, over_text, idx=(r['idx_t2i'], r['idx_i2t']))
    assert torch.equal(r2['loss'], r['loss']) and torch.equal(r2['dt'], r['dt']) and torch.equal(r2['di'], r['di'])


@pytest.mark.parametrize('dcl', [False, True])
def test_single_token_case_is_the_cls_loss(dcl):
    """T = I = 1, all-ones mask: both maxima are the one score, so with the image -> text denominator over
    the texts the loss is the CLS loss of the same latents (test_loss_options_cpu.general_loss)."""
    g = torch.Generator().manual_seed(5)
    t, i = torch.randn(5, 1, 16, generator=g, dtype=F64), torch.randn(5, 1, 16, generator=g, dtype=F64)
    lt = torch.tensor(math.log(1 / 0.07), dtype=F64)
    r = filip_ref(t, i, torch.ones(5, 1, dtype=torch.uint8), lt, dcl, True)
    ref, _ = general_loss(t[:, 0][None], i[:, 0][None], lt, decoupled=dcl)
    assert abs(r['loss'].item() - ref.item()) < 1e-12 * max(1.0, abs(ref.item()))


def test_i2t_directions_differ():
    g = torch.Generator().manual_seed(6)
    t, i = torch.randn(4, 6, 8, generator=g, dtype=F64), torch.randn(4, 3, 8, generator=g, dtype=F64)
    lt = torch.tensor(1.5, dtype=F64)
    mask = ragged_mask(4, 6, g)
    a, b = filip_ref(t, i, mask, lt)['loss'], filip_ref(t, i, mask, lt, i2t_over_text=True)['loss']
    assert abs(a.item() - b.item()) > 1e-6


def test_lowest_index_takes_a_tie():
    g = torch.Generator().manual_seed(7)
    t, i = torch.randn(2, 4, 8, generator=g, dtype=F64), torch.randn(2, 5, 8, generator=g, dtype=F64)
    i[:, 3] = i[:, 1]
    t[:, 2] = t[:, 0]
    r = filip_ref(t, i, torch.ones(2, 4, dtype=torch.uint8), torch.tensor(0.0, dtype=F64))
    assert (r['idx_t2i'] != 3).all() and (r['idx_i2t'] != 2).all()


# ------------------------------------------------------------------------------ model surface (no GPU)
def _tiny_model(**kw):
    from ctclip_mi355x.bert import BertConfig
    from ctclip_mi355x.models import build_ctclip
    vit = dict(dim=64, codebook_size=64, image_size=40, patch_size=20, temporal_patch_size=10, spatial_depth=1,
               temporal_depth=1, dim_head=32, heads=2)
    bert = BertConfig(vocab_size=100, hidden_size=64, num_hidden_layers=1, num_attention_heads=2,
                      intermediate_size=128, max_position_embeddings=32)
    return build_ctclip(vit, bert, 32, **kw)


def test_build_ctclip_with_all_token_embeds():
    m = _tiny_model(use_all_token_embeds=True)
    assert m.use_all_token_embeds
    assert tuple(m.to_visual_latent.weight.shape) == (32, 64)        # [Dl, ViT token width]
    assert tuple(m.to_text_latent.weight.shape) == (32, 64)
    plain = _tiny_model()
    assert not plain.use_all_token_embeds and tuple(plain.to_visual_latent.weight.shape) == (32, 2 * 2 * 64)


def test_unsupported_combinations_raise_by_name(monkeypatch):
    from ctclip_mi355x import dist_sync
    from ctclip_mi355x.attribution import ZeroShotAttribution
    from ctclip_mi355x.probe import LinearProbeEvaluator
    from ctclip_mi355x.retrieval import RetrievalEvaluator
    from ctclip_mi355x.trainer import CTClipTrainer
    from ctclip_mi355x.zero_shot import ZeroShotClassifier
    with pytest.raises(NotImplementedError, match='use_all_token_embeds with extra_latent_projection'):
        _tiny_model(use_all_token_embeds=True, extra_latent_projection=True)
    m = _tiny_model(use_all_token_embeds=True)
    # dim_image has to be the image tower's token width: the flattened width (the CLS configuration's) or a
    # tower that states no width would make one token of the whole pooled volume
    from ctclip_mi355x.ct_clip import CTCLIP
    towers = dict(image_encoder=m.visual_transformer, text_encoder=m.text_transformer, dim_text=64, dim_latent=32)
    assert CTCLIP(**towers, dim_image=64, use_all_token_embeds=True).use_all_token_embeds
    with pytest.raises(NotImplementedError, match='token width'):
        CTCLIP(**towers, dim_image=2 * 2 * 64, use_all_token_embeds=True)
    with pytest.raises(NotImplementedError, match='token width'):
        CTCLIP(**{**towers, 'image_encoder': torch.nn.Identity()}, dim_image=64, use_all_token_embeds=True)
    text = types.SimpleNamespace(input_ids=torch.zeros(2, 4, dtype=torch.long), attention_mask=torch.ones(2, 4))
    image = torch.zeros(2, 1, 10, 40, 40)
    with pytest.raises(NotImplementedError, match='use_all_token_embeds with aug_image'):
        m(text, image, return_loss=True, aug_image=image.clone())
    with pytest.raises(NotImplementedError, match='use_all_token_embeds=True is not chunked'):
        CTClipTrainer.train_step_chunked(types.SimpleNamespace(model=m), text, image, 1)
    for who, make in (('ZeroShotClassifier', lambda: ZeroShotClassifier(m)),
                      ('RetrievalEvaluator', lambda: RetrievalEvaluator(m)),
                      ('LinearProbeEvaluator', lambda: LinearProbeEvaluator(m)),
                      ('ZeroShotAttribution', lambda: ZeroShotAttribution(types.SimpleNamespace(model=m)))):
        with pytest.raises(NotImplementedError, match=f'{who} with CTCLIP\\(use_all_token_embeds=True\\)'):
            make()
    monkeypatch.setattr(dist_sync, 'world_rank', lambda: (2, 0))
    with pytest.raises(NotImplementedError, match='world size > 1'):
        m(text, image, return_loss=True)
