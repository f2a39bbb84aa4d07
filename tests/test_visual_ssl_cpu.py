"""The SimSiam visual self-supervision head without a GPU: the float64 restatements and
bounds of visual_ssl_common.py are held against f32 torch (a correct evaluation stays inside them, two
deliberately wrong ones do not), ``VisualSSLHead`` on CPU against its float64 copy and torch's own
``BatchNorm1d`` bookkeeping, and the constructor / forward rules of ``CTCLIP(visual_ssl=...)``."""
import types

import pytest
import torch
from torch import nn

from visual_ssl_common import (EPS, FLAGS, MOM, SHAPES, head_ref64, linear_bn_bounds, linear_bn_ref, make_inputs,
                               simsiam_ref, simsiam_ref_grads, worst)


def _f32_linear_bn(inp, G, relu, wrong=None):
    """An f32 torch evaluation of Linear + BatchNorm1d (+ ReLU); ``wrong``: 'unbiased' normalises with the
    unbiased variance, 'drop_k' leaves the last k term out of the product."""
    X, W = inp['X'], inp['W']
    y = (X[:, :-1] @ W[:, :-1].t()) if wrong == 'drop_k' else X @ W.t()
    if inp['bias'] is not None:
        y = y + inp['bias']
    M, N = y.shape
    yg = y.view(G, M // G, N)
    mean = yg.mean(1, keepdim=True)
    var = yg.var(1, unbiased=wrong == 'unbiased', keepdim=True)
    rstd = (var + EPS).rsqrt()
    xhat = ((yg - mean) * rstd).reshape(M, N)
    out = xhat * inp['gamma'] + inp['beta'] if inp['gamma'] is not None else xhat
    return dict(out=out.clamp_min(0) if relu else out, xhat=xhat, rstd=rstd.reshape(G, N))


@pytest.mark.parametrize('affine,relu,bias', FLAGS)
@pytest.mark.parametrize('G,R,K,N', SHAPES)
def test_f32_restatement_inside_the_bounds_and_wrong_ones_outside(G, R, K, N, affine, relu, bias):
    inp = make_inputs(G, R, K, N, affine, bias)
    ref = linear_bn_ref(inp, G, relu)
    bound = linear_bn_bounds(inp, ref, G)
    got = _f32_linear_bn(inp, G, relu)
    for k in ('out', 'xhat', 'rstd'):
        assert worst(got[k], ref[k], bound[k]) <= 1.0, k
    for wrong in ('unbiased', 'drop_k'):
        bad = _f32_linear_bn(inp, G, relu, wrong=wrong)
        assert worst(bad['xhat'], ref['xhat'], bound['xhat']) > 1.0, wrong


def test_restatement_running_statistics_are_batchnorm1d():
    """The restatement's running statistics after one call on G groups are what G successive float64
    ``nn.BatchNorm1d`` calls leave, and its outputs are that module's."""
    G, R, K, N = 2, 8, 512, 4
    inp = make_inputs(G, R, K, N, True, False)
    ref = linear_bn_ref(inp, G, False)
    bn = nn.BatchNorm1d(N, eps=EPS, momentum=MOM).double()
    with torch.no_grad():
        bn.weight.copy_(inp['gamma'])
        bn.bias.copy_(inp['beta'])
        bn.running_mean.copy_(inp['running_mean'])
        bn.running_var.copy_(inp['running_var'])
    out = torch.cat([bn(ref['y'][g * R:(g + 1) * R]) for g in range(G)])
    assert torch.allclose(out, ref['out'], rtol=0, atol=1e-12)
    assert torch.allclose(bn.running_mean, ref['running_mean'], rtol=0, atol=1e-14)
    assert torch.allclose(bn.running_var, ref['running_var'], rtol=0, atol=1e-14)
    bn.eval()
    ev = linear_bn_ref(dict(inp, running_mean=bn.running_mean, running_var=bn.running_var), G, False,
                       use_running=True)
    assert torch.allclose(bn(ref['y']), ev['out'], rtol=0, atol=1e-12)


def test_loss_restatement_is_two_minus_two_cosine():
    g = torch.Generator().manual_seed(5)
    p1, p2, z1, z2 = (torch.randn(6, 24, generator=g, dtype=torch.float64) for _ in range(4))
    cs = nn.functional.cosine_similarity
    want = ((2 - 2 * cs(p1, z2, dim=-1)) + (2 - 2 * cs(p2, z1, dim=-1))).mean()
    assert abs(simsiam_ref(p1, p2, z1, z2).item() - want.item()) < 1e-13
    assert abs(simsiam_ref(p1, p2, p2, p1).item()) < 1e-13
    p1[2] = 0
    z1[4] = 0
    loss, d1, d2 = simsiam_ref_grads(p1, p2, z1, z2)
    assert torch.isfinite(loss) and torch.isfinite(d1).all() and torch.isfinite(d2).all()


# ------------------------------------------------------------------------------ the head on CPU
def _head(dim=12, hidden=20, proj=8, seed=0):
    from ctclip_mi355x.visual_ssl import VisualSSLHead
    torch.manual_seed(seed)
    return VisualSSLHead(dim, projection_size=proj, projection_hidden_size=hidden)


def test_head_layout_and_state_dict_keys():
    head = _head()
    pj, pd = head.projector, head.predictor
    assert [type(m) for m in pj] == [nn.Linear, nn.BatchNorm1d, nn.ReLU, nn.Linear, nn.BatchNorm1d, nn.ReLU,
                                     nn.Linear, nn.BatchNorm1d]
    assert [type(m) for m in pd] == [nn.Linear, nn.BatchNorm1d, nn.ReLU, nn.Linear]
    assert all(pj[i].bias is None for i in (0, 3, 6)) and not pj[7].affine and pj[1].affine and pj[4].affine
    assert pd[0].bias is not None and pd[3].bias is not None
    keys = set(head.state_dict())
    assert {'projector.0.weight', 'projector.1.weight', 'projector.1.running_mean', 'projector.7.running_var',
            'predictor.0.bias', 'predictor.1.running_var', 'predictor.3.weight', 'predictor.3.bias'} <= keys
    assert 'projector.7.weight' not in keys and 'projector.0.bias' not in keys
    from ctclip_mi355x import VisualSSLHead
    d = VisualSSLHead(512)
    assert d.projector[0].weight.shape == (4096, 512) and d.predictor[3].weight.shape == (256, 4096)
    assert d.projector[1].momentum == 0.1 and d.projector[1].eps == 1e-5


def test_head_on_cpu_equals_its_float64_copy_and_updates_the_statistics_once_per_view():
    head = _head()
    g = torch.Generator().manual_seed(1)
    views = torch.randn(2, 5, 12, generator=g)
    before = {k: v.clone() for k, v in head.state_dict().items()}
    ref, copy = head_ref64(head, views)              # the copy is made from the state before the forward
    loss = head(views)
    assert loss.shape == () and abs(loss.item() - ref.item()) < 1e-5
    # gradients reach every parameter and the input
    leaf = views.clone().requires_grad_(True)
    head.load_state_dict(before)
    head(leaf).backward()
    assert leaf.grad is not None and all(p.grad is not None and torch.isfinite(p.grad).all() for p in head.parameters())
    # one forward = two successive BatchNorm1d calls per layer (view 0, then view 1)
    for k, v in copy.state_dict().items():
        if 'running' in k:
            assert torch.allclose(head.state_dict()[k].double(), v, rtol=0, atol=1e-5), k
            assert not torch.equal(head.state_dict()[k], before[k]), k
        if 'num_batches_tracked' in k:
            assert head.state_dict()[k].item() == 2
    bn = nn.BatchNorm1d(20).double()
    with torch.no_grad():
        y = [views[g].double() @ before['projector.0.weight'].double().t() for g in range(2)]
        bn(y[0])
        bn(y[1])
    assert torch.allclose(head.projector[1].running_mean.double(), bn.running_mean, rtol=0, atol=1e-5)
    assert torch.allclose(head.projector[1].running_var.double(), bn.running_var, rtol=0, atol=1e-5)
    # eval mode: the running statistics, nothing updated
    head.eval()
    snap = {k: v.clone() for k, v in head.state_dict().items()}
    ref_eval, _ = head_ref64(head, views)
    assert abs(head(views).item() - ref_eval.item()) < 1e-5
    assert all(torch.equal(v, snap[k]) for k, v in head.state_dict().items())
    assert abs(ref_eval.item() - ref.item()) > 1e-6


def test_head_refusals():
    head = _head()
    with pytest.raises(ValueError, match='more than one volume'):
        head(torch.randn(2, 1, 12))
    head.eval()
    assert torch.isfinite(head(torch.randn(2, 1, 12)))       # eval mode has no batch statistics to miss
    for bad in (torch.randn(3, 4, 12), torch.randn(2, 4, 11), torch.randn(8, 12)):
        with pytest.raises(ValueError, match='views must be'):
            head(bad)
    from ctclip_mi355x.visual_ssl import VisualSSLHead
    with pytest.raises(ValueError, match='positive'):
        VisualSSLHead(0)


# ------------------------------------------------------------------------------ CTCLIP rules
class _Stop(Exception):
    pass


class _Tower(nn.Module):
    def forward(self, *a, **k):
        raise _Stop

    def encode_pooled(self, *a, **k):
        raise _Stop


def _model(**kw):
    from ctclip_mi355x.ct_clip import CTCLIP
    return CTCLIP(image_encoder=_Tower(), text_encoder=_Tower(), dim_text=8, dim_image=8, dim_latent=12, **kw)


def test_constructor_rules():
    plain = _model()
    assert plain.visual_ssl is None and not any(k.startswith('visual_ssl') for k in plain.state_dict())
    assert set(plain.state_dict()) == {'to_text_latent.weight', 'to_visual_latent.weight', 'temperature',
                                       'to_text_latent_extra.weight', 'to_visual_latent_extra.weight'}
    head = _head()
    m = _model(visual_ssl=head)
    assert m.visual_ssl is head and m.image_ssl_loss_weight == 0.05 and m.last_image_ssl_loss is None
    assert _model(visual_ssl=head, image_ssl_loss_weight=0.2, use_visual_ssl=True).image_ssl_loss_weight == 0.2
    assert {'visual_ssl.' + k for k in head.state_dict()} == set(m.state_dict()) - set(plain.state_dict())
    assert all(any(p is q for q in m.parameters()) for p in head.parameters())
    assert _model(visual_ssl=head, extra_latent_projection=True, decoupled_contrastive_learning=True)
    for other in (nn.Linear(2, 2), object(), 'simsiam'):
        with pytest.raises(NotImplementedError, match='outside the contrastive hot path'):
            _model(visual_ssl=other)
    with pytest.raises(NotImplementedError, match='outside the contrastive hot path'):
        _model(use_visual_ssl=True)
    with pytest.raises(NotImplementedError, match='visual_ssl with sigmoid_loss'):
        _model(visual_ssl=head, sigmoid_loss=True)
    tower = _Tower()
    tower.dim = 8
    from ctclip_mi355x.ct_clip import CTCLIP
    with pytest.raises(NotImplementedError, match='visual_ssl with use_all_token_embeds'):
        CTCLIP(image_encoder=tower, text_encoder=_Tower(), dim_text=8, dim_image=8, dim_latent=12,
               visual_ssl=head, use_all_token_embeds=True)
    with pytest.raises(ValueError, match='dim_latent'):
        _model(visual_ssl=_head(dim=16))


def test_forward_and_trainer_refusals(monkeypatch):
    text = types.SimpleNamespace(input_ids=torch.zeros(2, 4, dtype=torch.long), attention_mask=torch.ones(2, 4))
    image = torch.zeros(2, 1, 4, 8, 8)
    m = _model(visual_ssl=_head())
    with pytest.raises(ValueError, match='visual_ssl needs aug_image'):
        m(text, image, return_loss=True)
    with pytest.raises(_Stop):                         # without return_loss nothing changes
        m(text, image)
    with pytest.raises(_Stop):                         # a valid call reaches the towers
        m(text, image, return_loss=True, aug_image=image.clone())
    from ctclip_mi355x import dist_sync
    monkeypatch.setattr(dist_sync, 'world_rank', lambda: (2, 0))
    with pytest.raises(NotImplementedError, match='world size > 1'):
        m(text, image, return_loss=True, aug_image=image.clone())
    monkeypatch.undo()
    from ctclip_mi355x.trainer import CTClipTrainer
    tr = CTClipTrainer(m, overlap_grad_sync=False)
    assert all(any(p is q for q in tr.flat.params) for p in m.visual_ssl.parameters())
    with pytest.raises(NotImplementedError, match='visual_ssl is not chunked'):
        tr.train_step_chunked(text, image, 1)


def test_build_ctclip_builds_the_head():
    from ctclip_mi355x.bert import BertConfig
    from ctclip_mi355x.models import build_ctclip
    from ctclip_mi355x.visual_ssl import VisualSSLHead
    vit = dict(dim=64, codebook_size=64, image_size=40, patch_size=20, temporal_patch_size=10, spatial_depth=1,
               temporal_depth=1, dim_head=32, heads=2)
    bert = BertConfig(vocab_size=50, hidden_size=64, num_hidden_layers=1, num_attention_heads=2,
                      intermediate_size=48, max_position_embeddings=16)
    m = build_ctclip(vit, bert, 16, visual_ssl=dict(projection_size=8, projection_hidden_size=12),
                     image_ssl_loss_weight=0.1)
    assert isinstance(m.visual_ssl, VisualSSLHead) and m.visual_ssl.dim == 16 and m.image_ssl_loss_weight == 0.1
    assert m.visual_ssl.projector[0].weight.shape == (12, 16) and m.visual_ssl.predictor[3].weight.shape == (8, 12)
    assert build_ctclip(vit, bert, 16, visual_ssl=True).visual_ssl.projection_hidden_size == 4096
    assert build_ctclip(vit, bert, 16).visual_ssl is None
