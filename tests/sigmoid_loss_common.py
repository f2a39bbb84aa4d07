"""The pairwise sigmoid (SigLIP) contrastive loss restated in torch, shared by
test_sigmoid_loss_cpu.py and test_gpu_sigmoid_loss.py:

    t^_i, i^_j = F.normalize(raw latents, eps 1e-12);  x_ij = exp(log_temp) <t^_i, i^_j> + bias;
    z_ij = +1 (i = j) / -1;  L = 1/Bg sum_ij softplus(-z_ij x_ij),

softplus evaluated as max(u, 0) + log1p(exp(-|u|)).  It follows the dtype of its inputs; the float64
reference is the restatement on float64 copies with autograd."""
import math
import types

import torch
import torch.nn.functional as F

LT_PAPER, B_PAPER = math.log(10.0), -10.0            # the paper's initialisation
TEMP_BIAS = [(LT_PAPER, B_PAPER), (1.0, 0.0), (math.log(1 / 0.07), -3.0)]


def softplus(u):
    return u.clamp_min(0) + torch.log1p(torch.exp(-u.abs()))


def sigmoid_loss(t_raw, i_raw, log_temp, bias):
    """The loss (0-d) of raw latents [Bg, Dl], log_temp and bias (0-d or [1])."""
    tn, inn = F.normalize(t_raw, dim=-1, eps=1e-12), F.normalize(i_raw, dim=-1, eps=1e-12)
    x = log_temp.reshape(()).exp() * (tn @ inn.t()) + bias.reshape(())
    z = 2.0 * torch.eye(x.shape[0], dtype=x.dtype, device=x.device) - 1.0
    return softplus(-z * x).sum() / x.shape[0]


def loss_and_grads(t_raw, i_raw, log_temp, bias):
    """(loss [1], dt, di, dlt [1], dbias [1]) by autograd, in the dtype of the inputs: the outputs of
    kernels.sigmoid_loss, and a stand-in for it as ``SigmoidLossFn``'s ``impl``."""
    a = [x.detach().clone().requires_grad_(True) for x in (t_raw, i_raw, log_temp, bias)]
    with torch.enable_grad():          # also called inside an autograd.Function forward
        loss = sigmoid_loss(*a)
        loss.backward()
    return loss.detach().reshape(1), a[0].grad, a[1].grad, a[2].grad.reshape(1), a[3].grad.reshape(1)


def ref64(t_raw, i_raw, log_temp, bias):
    """The float64 reference of f32 inputs (CPU)."""
    return loss_and_grads(*[x.detach().double().cpu() for x in (t_raw, i_raw, log_temp, bias)])


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def check(out, ref, what=''):
    """The project's loss tolerances (test_gpu_loss_tiled.py): loss 1e-5 max(1, |ref|); every gradient,
    dlt and dbias 1e-4 relative (norm of the difference over the norm of the reference)."""
    loss, dt, di, dlt, db = out
    rl, rdt, rdi, rdlt, rdb = ref
    print(f'{what} loss {loss.item():.7f} ref {rl.item():.7f}; rel dt {rel(dt, rdt):.2e} di {rel(di, rdi):.2e} '
          f'dlt {rel(dlt, rdlt):.2e} dbias {rel(db, rdb):.2e}')
    assert all(torch.isfinite(x).all() for x in out)
    assert abs(loss.item() - rl.item()) < 1e-5 * max(1.0, abs(rl.item()))
    assert dt.shape == rdt.shape and di.shape == rdi.shape
    assert rel(dt, rdt) < 1e-4 and rel(di, rdi) < 1e-4 and rel(dlt, rdlt) < 1e-4 and rel(db, rdb) < 1e-4


# ------------------------------------------------------------------------------ model level (GPU tests)
def cfg_small(layers=2):
    """The 2+2-layer small configuration of test_gpu_loss_options.py."""
    from oracle import ctclip_oracle as O
    vit = O.ViTConfig(dim=512, codebook_size=8192, image_size=160, patch_size=20, temporal_patch_size=10,
                      spatial_depth=layers, temporal_depth=layers, dim_head=32, heads=8, frames=40)
    bert = O.BertConfig(vocab_size=1000, hidden=768, layers=layers, heads=12, intermediate=3072, max_position=64)
    return O.ClipConfig(vit=vit, bert=bert, dim_latent=512)


HEADS = ('to_text_latent.weight', 'to_visual_latent.weight', 'temperature', 'logit_bias')


def build(cfg, seed=0, **options):
    """A CTCLIP on the oracle's seeded weights; with ``sigmoid_loss=True`` the bias keeps its constructor
    value (the seeded state_dict has the reference's keys only).  The heads train."""
    from oracle import weights as W
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
    m = build_ctclip(vit, bert, cfg.dim_latent, **options)
    res = m.load_state_dict(W.make_state_dict(cfg, seed=seed), strict=False)
    assert not res.unexpected_keys
    assert list(res.missing_keys) == (['logit_bias'] if options.get('sigmoid_loss') else [])
    m = set_finetune_trainable(m)
    named = dict(m.named_parameters())
    for n in HEADS:
        if n in named:
            named[n].requires_grad = True
    return m.cuda()


def batch(cfg, B=2, seed=0):
    from oracle import weights as W
    hu = W.make_hu(B, cfg.vit, seed=1234 + seed)
    ids, mask = W.make_text(B, 32, cfg.bert.vocab_size, seed=4321 + seed, ragged=True)
    return hu.cuda(), types.SimpleNamespace(input_ids=ids.cuda(), attention_mask=mask.cuda())
