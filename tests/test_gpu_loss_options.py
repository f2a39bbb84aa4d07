"""The general contrastive loss on the GPU (csrc/loss.hip ctclip_clip_loss_ex: image multiview pairs,
the extra CLOOB latent pair, decoupled contrastive learning; ct_clip/ct_clip.py:845-899) against the
fp32 torch restatement of test_loss_options_cpu.py (pinned there to the reference's own outputs),
and the same options through CTCLIP.forward, the trainer and torch.ops.ctclip.clip_infonce_ex."""
import math
import types

import pytest
import torch
import torch.nn.functional as F
from torch._subclasses.fake_tensor import FakeTensorMode

from oracle import ctclip_oracle as O
from oracle import weights as W
from test_loss_options_cpu import general_loss, loss_and_grads

pytestmark = pytest.mark.gpu
dev = 'cuda'
LT = math.log(1 / 0.07)          # exp(S) stays finite with unit latents (|S| <= 14.3)


@pytest.fixture(scope='module')
def K():
    from ctclip_mi355x import kernels
    return kernels


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def _inputs(Bg, Dl, Vi, extra, seed=0):
    g = torch.Generator(device=dev).manual_seed(1000 * Bg + Dl + 7 * Vi + seed)
    r = lambda v: torch.randn(v, Bg, Dl, device=dev, generator=g)
    t, i = r(1), r(Vi)
    tx, ix = (r(1), r(Vi)) if extra else (None, None)
    return t, i, tx, ix, torch.tensor([LT], device=dev)


def _weights(Vi):
    return (0.9, 0.1) if Vi > 1 else (1.0, 0.0)


# ------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize('extra', [False, True])
@pytest.mark.parametrize('dcl', [False, True])
@pytest.mark.parametrize('P', [1, 3])
@pytest.mark.parametrize('Dl', [64, 512])
@pytest.mark.parametrize('Bg', [2, 3, 8, 128])
def test_kernel_matches_restatement(K, Bg, Dl, P, dcl, extra):
    """Bg = 2: DCL's denominator is one term; Bg = 3 / Dl = 64: strides and tails; Bg = 128: the LDS
    limit.  Tolerances of test_torch_ops.test_clip_infonce: loss 1e-5 max(1, |ref|), gradients 1e-4."""
    t, i, tx, ix, lt = _inputs(Bg, Dl, P, extra)
    w_main, w_mv = _weights(P)
    loss, dt, di, dtx, dix, dlt, pair = K.clip_loss_ex(t, i, lt, tx, ix, dcl, w_main, w_mv)
    rl, rdt, rdi, rdtx, rdix, rdlt, rpair = loss_and_grads(t, i, lt, tx, ix, dcl, w_main, w_mv)
    print(f'loss {loss.item():.7f} ref {rl.item():.7f}; rel dt {rel(dt, rdt):.2e} di {rel(di, rdi):.2e} '
          f'dlt {rel(dlt, rdlt):.2e}')
    assert abs(loss.item() - rl.item()) < 1e-5 * max(1.0, abs(rl.item()))
    assert pair.shape == (P,) and (pair - rpair).abs().max().item() < 1e-5 * max(1.0, rpair.abs().max().item())
    assert rel(dt, rdt) < 1e-4 and rel(di, rdi) < 1e-4 and rel(dlt, rdlt) < 1e-4
    if extra:
        assert rel(dtx, rdtx) < 1e-4 and rel(dix, rdix) < 1e-4
    else:
        assert dtx is None and dix is None


@pytest.mark.parametrize('Bg,Dl', [(2, 64), (3, 512), (8, 512), (64, 512), (128, 64), (128, 512)])
def test_plain_case_equals_clip_loss_bitwise(K, Bg, Dl):
    """P = 1, no extra pair, decoupled off, w_main = 1: the same passes in the same order as the
    one-workgroup ctclip_clip_loss -- loss and every gradient bit for bit."""
    t, i, _, _, lt = _inputs(Bg, Dl, 1, False, seed=3)
    loss, dt, di, _, _, dlt, pair = K.clip_loss_ex(t, i, lt)
    l0, dt0, di0, dlt0 = K.clip_loss(t[0].contiguous(), i[0].contiguous(), lt)[:4]
    assert torch.equal(loss, l0) and torch.equal(pair, l0) and torch.equal(dlt, dlt0)
    assert torch.equal(dt[0], dt0) and torch.equal(di[0], di0)


def test_bit_reproducible(K):
    t, i, tx, ix, lt = _inputs(64, 512, 3, True, seed=5)
    a = K.clip_loss_ex(t, i, lt, tx, ix, True, 0.9, 0.1)
    b = K.clip_loss_ex(t, i, lt, tx, ix, True, 0.9, 0.1)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_batch_over_128_is_refused(K):
    from ctclip_mi355x._lib import KernelError
    t, i, _, _, lt = _inputs(129, 64, 1, False)
    with pytest.raises(KernelError, match='1003'):        # CT_ESHAPE
        K.clip_loss_ex(t, i, lt)


def test_zero_norm_rows_give_finite_gradients(K):
    """A zero latent row (norm below 1e-12) takes the kernel's g / max(n, 1e-12) branch, as in
    ctclip_clip_loss: everything stays finite."""
    t, i, tx, ix, lt = _inputs(8, 64, 2, True, seed=9)
    t[0, 1] = 0
    i[1, 3] = 0
    tx[0, 0] = 0
    ix[0, 7] = 0
    out = K.clip_loss_ex(t, i, lt, tx, ix, True, 0.9, 0.1)
    assert all(torch.isfinite(x).all() for x in out)
    ref = loss_and_grads(t, i, lt, tx, ix, True, 0.9, 0.1)
    assert abs(out[0].item() - ref[0].item()) < 1e-5 * max(1.0, abs(ref[0].item()))


# ------------------------------------------------------------------------------ torch.library op
def test_clip_infonce_ex_op():
    from ctclip_mi355x import ops
    t, i, tx, ix, lt = _inputs(8, 512, 2, True, seed=11)
    args = [x.clone().requires_grad_(True) for x in (t, i, lt, tx, ix)]
    loss = ops.clip_infonce_ex(*args, decoupled=True, w_main=0.9, w_multiview=0.1)
    ref = [x.detach().clone().requires_grad_(True) for x in (t, i, lt, tx, ix)]
    rl, _ = general_loss(ref[0], ref[1], ref[2], ref[3], ref[4], True, 0.9, 0.1)
    assert abs(loss.item() - rl.item()) < 1e-5 * max(1.0, abs(rl.item()))
    (2.0 * loss).backward()
    (2.0 * rl).backward()
    for a, b in zip(args, ref):
        assert rel(a.grad, b.grad) < 1e-4
    utils = ('test_schema', 'test_faketensor', 'test_autograd_registration')
    op = torch.ops.ctclip.clip_infonce_ex
    torch.library.opcheck(op, (t, i, lt, tx, ix, True, 0.9, 0.1), test_utils=utils)
    torch.library.opcheck(op, (t, i, lt, None, None, False, 0.9, 0.1), test_utils=utils)
    with FakeTensorMode():
        ft, fi = torch.empty(1, 8, 512, device=dev), torch.empty(3, 8, 512, device=dev)
        flt = torch.empty(1, device=dev)
        out = op(ft, fi, flt, ft, fi, True, 0.9, 0.1)
        assert out[0].shape == () and out[1].shape == ft.shape and out[2].shape == fi.shape
        assert out[3].shape == ft.shape and out[4].shape == fi.shape and out[5].shape == flt.shape
        assert out[6].shape == (3,)
        out = op(ft, fi, flt, None, None, False, 1.0, 0.0)
        assert out[3].shape == (0,) and out[4].shape == (0,)
    with pytest.raises(Exception):      # registered for the HIP device only
        op(t.cpu(), i.cpu(), lt.cpu(), None, None, False, 1.0, 0.0)


# ------------------------------------------------------------------------------ model level
def cfg_small(layers=2):
    vit = O.ViTConfig(dim=512, codebook_size=8192, image_size=160, patch_size=20, temporal_patch_size=10,
                      spatial_depth=layers, temporal_depth=layers, dim_head=32, heads=8, frames=40)
    bert = O.BertConfig(vocab_size=1000, hidden=768, layers=layers, heads=12, intermediate=3072, max_position=64)
    return O.ClipConfig(vit=vit, bert=bert, dim_latent=512)


PROJ = ('to_text_latent.weight', 'to_visual_latent.weight', 'to_text_latent_extra.weight',
        'to_visual_latent_extra.weight', 'temperature')


def build(cfg, **loss_options):
    from ctclip_mi355x.models import build_ctclip, set_finetune_trainable
    from ctclip_mi355x.bert import BertConfig
    v, b = cfg.vit, cfg.bert
    vit = dict(dim=v.dim, codebook_size=v.codebook_size, image_size=v.image_size, patch_size=v.patch_size,
               temporal_patch_size=v.temporal_patch_size, spatial_depth=v.spatial_depth,
               temporal_depth=v.temporal_depth, dim_head=v.dim_head, heads=v.heads)
    bert = BertConfig(vocab_size=b.vocab_size, hidden_size=b.hidden, num_hidden_layers=b.layers,
                      num_attention_heads=b.heads, intermediate_size=b.intermediate,
                      max_position_embeddings=b.max_position, hidden_dropout_prob=0.0,
                      attention_probs_dropout_prob=0.0)
    m = build_ctclip(vit, bert, cfg.dim_latent, **loss_options)
    m.load_state_dict(W.make_state_dict(cfg), strict=True)
    m = set_finetune_trainable(m)
    named = dict(m.named_parameters())
    for n in PROJ:                       # the heads train too here (frozen in the fine-tune recipe)
        named[n].requires_grad = True
    return m.cuda()


def _batch(cfg, B=2):
    hu, aug = W.make_hu(B, cfg.vit), W.make_hu(B, cfg.vit, seed=100)
    ids, mask = W.make_text(B, 32, cfg.bert.vocab_size, ragged=True)
    text = types.SimpleNamespace(input_ids=ids.cuda(), attention_mask=mask.cuda())
    return hu, aug, ids, mask, text


def test_model_dcl_extra_multiview_matches_oracle():
    """DCL + extra projection + one augmented view through CTCLIP.forward against the oracle's towers
    (one O.ctclip_forward per view, VQ indices forced to the HIP path's) + the restatement: latents
    and loss within 1e-3, projection / extra-projection / temperature gradients
    within 5e-2 relative (the tolerance of test_gpu_model.test_backward_grads)."""
    cfg = cfg_small()
    B = 2
    model = build(cfg, decoupled_contrastive_learning=True, extra_latent_projection=True)
    hu, aug, ids, mask, text = _batch(cfg, B)
    sd = W.make_state_dict(cfg)
    views = (hu, aug)

    def towers(idx):
        enc = []
        with torch.no_grad():
            for v, x in enumerate(views):
                enc.append(O.ctclip_forward(sd, ids, mask, O.normalize_hu(x), cfg, training=False,
                                            force_ind=idx.view(2 * B, -1)[v * B:(v + 1) * B]))
        cls = enc[0]['enc_text'][:, 0, :]
        pooled = torch.cat([e['enc_image'].mean(dim=1).reshape(B, -1) for e in enc], 0)
        return enc, cls, pooled

    # latents: the reference's 4-tuple, every view (int16 HU in, f32 views give the same bits)
    model.eval()
    with torch.no_grad():
        lat = model(text, hu.cuda(), return_loss=True, return_latents=True, aug_image=aug.cuda())
        idx = model.visual_transformer.vq.state.last_indices.cpu().clone()
        lat_f32 = model(text, O.normalize_hu(hu).cuda(), return_loss=True, return_latents=True,
                        aug_image=(O.normalize_hu(aug).cuda(),))
        s_t2i = model(text, hu.cuda())
        s_i2t = model(text, hu.cuda(), text_to_image=False)
    assert len(lat) == 4 and all(torch.equal(a, b) for a, b in zip(lat, lat_f32))
    enc, cls, pooled = towers(idx)
    ref_lat = (F.normalize(F.linear(cls, sd['to_text_latent.weight']), dim=-1),
               F.normalize(F.linear(pooled, sd['to_visual_latent.weight']), dim=-1),
               F.normalize(F.linear(cls, sd['to_text_latent_extra.weight']), dim=-1),
               F.normalize(F.linear(pooled, sd['to_visual_latent_extra.weight']), dim=-1))
    assert torch.equal(ref_lat[0], enc[0]['text_latents']) or (ref_lat[0] - enc[0]['text_latents']).abs().max() < 1e-6
    for n, a, b in zip(('text', 'image', 'text_extra', 'image_extra'), lat, ref_lat):
        err = (a.cpu() - b).abs().max().item()
        print(f'{n} latents max err {err:.2e}')
        assert a.shape == b.shape and err < 1e-3, n
    temp = sd['temperature'].exp()
    assert ((s_t2i.cpu() - (ref_lat[0] * ref_lat[1][:B]).sum(-1) * temp).abs().max().item()) < 1e-3
    assert ((s_i2t.cpu() - (ref_lat[2] * ref_lat[3][:B]).sum(-1) * temp).abs().max().item()) < 1e-3
    assert not torch.allclose(s_t2i, s_i2t)

    # loss + gradients of the heads
    model.train()
    model.zero_grad(set_to_none=True)
    loss = model(text, hu.cuda(), return_loss=True, aug_image=aug.cuda())
    idx2 = model.visual_transformer.vq.state.last_indices.cpu()
    loss.backward()
    torch.cuda.synchronize()
    if not torch.equal(idx, idx2):
        enc, cls, pooled = towers(idx2)
    p = {n: sd[n].clone().requires_grad_(True) for n in PROJ}
    proj = lambda x, n, v: F.linear(x, p[n]).view(v, B, -1)
    w_mv = float(model.multiview_loss_weight)
    ref, pair = general_loss(proj(cls, PROJ[0], 1), proj(pooled, PROJ[1], 2), p['temperature'], proj(cls, PROJ[2], 1),
                             proj(pooled, PROJ[3], 2), True, 1.0 - w_mv, w_mv)
    ref.backward()
    print(f'loss {loss.item():.6f} ref {ref.item():.6f} pairs {pair.tolist()}')
    assert abs(loss.item() - ref.item()) < 1e-3
    named = dict(model.named_parameters())
    bad = []
    for n in PROJ:
        r = rel(named[n].grad, p[n].grad)
        print(f'{n}: grad rel err {r:.2e}')
        if not r < 5e-2:
            bad.append((n, r))
    assert not bad, bad


def test_train_step_updates_extra_heads_bit_reproducibly():
    """One CTClipTrainer step with DCL + extra projection + one augmented view and the heads
    trainable: the extra projections get gradients, Adam and bf16 shadows (a nonzero update), and two
    identical steps from the same state give the same bits (no atomics in the new loss)."""
    from ctclip_mi355x.trainer import CTClipTrainer
    from ctclip_mi355x import functional as Fn
    cfg = cfg_small(layers=1)
    hu, aug, ids, mask, text = _batch(cfg)
    sd = W.make_state_dict(cfg)
    runs = []
    for _ in range(2):
        torch.manual_seed(0)
        model = build(cfg, decoupled_contrastive_learning=True, extra_latent_projection=True)
        tr = CTClipTrainer(model, lr=1e-4)
        loss = tr.train_step(text, hu.cuda(), aug_image=aug.cuda())
        tr.flush()
        torch.cuda.synchronize()
        assert torch.isfinite(loss) and tr.norm[0].item() > 0
        for n in ('to_text_latent_extra.weight', 'to_visual_latent_extra.weight'):
            prm = dict(model.named_parameters())[n]
            assert not torch.equal(prm.detach().cpu(), sd[n]), n
            sh = Fn.shadow_bf16(prm)
            assert sh is not None and torch.equal(sh, prm.detach().bfloat16()), n
        runs.append((loss.detach().clone(), tr.flat.data.clone(), tr.m.clone(), tr.v.clone()))
        del model, tr
    for a, b in zip(*runs):
        assert torch.equal(a, b)
