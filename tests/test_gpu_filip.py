"""The fine-grained (FILIP) token-wise contrastive loss on the GPU (csrc/filip.hip, kernels.filip_loss,
functional.FilipLossFn, CTCLIP(use_all_token_embeds=True)) against the float64 restatement
``test_filip_cpu.filip_ref``.  The restatement is given the kernel's argmax indices (the forced-index idiom
of the VQ tests) after every chosen index has been shown to score, in float64, within the f32 accumulation
bound of the float64 maximum.  Tolerances: those of test_gpu_loss_options.test_kernel_matches_restatement
(loss 1e-5 max(1, |ref|), gradients 1e-4 relative), the same arithmetic class."""
import math
import types

import pytest
import torch

from oracle import ctclip_oracle as O
from oracle import weights as W
from test_filip_cpu import filip_ref, ragged_mask, rel

pytestmark = pytest.mark.gpu
dev = 'cuda'
SHAPES = [(1, 1, 1, 16), (2, 7, 4, 32), (3, 16, 16, 64), (3, 17, 65, 64), (5, 33, 63, 128), (2, 40, 576, 512),
          (4, 512, 64, 32)]
OPTIONS = [(False, False), (True, False), (False, True), (True, True)]      # (decoupled, i2t_over_text)
OUTPUTS = ('loss', 'dt', 'di', 'dlt', 'A', 'C', 'idx_t2i', 'idx_i2t')


@pytest.fixture(scope='module')
def K():
    from ctclip_mi355x import kernels
    return kernels


def _inputs(Bg, T, I, Dl, seed=0, garbage=1.0):
    """Seeded latents and a ragged mask; the masked text positions hold 1e4-scaled garbage."""
    g = torch.Generator().manual_seed(100 * Bg + T + 3 * I + Dl + seed)
    t, i = torch.randn(Bg, T, Dl, generator=g), torch.randn(Bg, I, Dl, generator=g)
    mask = ragged_mask(Bg, T, g)
    junk = 1e4 * garbage * torch.randn(Bg, T, Dl, generator=torch.Generator().manual_seed(seed + 99))
    t = torch.where(mask.bool()[..., None], t, junk)
    return t, i, mask


def _run(K, t, i, mask, lt, dcl=False, over=False):
    out = K.filip_loss(t.to(dev), i.to(dev), mask.to(dev), torch.tensor([lt], device=dev), decoupled=dcl,
                       i2t_over_text=over, want_logits=True, want_idx=True)
    return {k: v.cpu() for k, v in out.items()}


def _check_indices(out, ref, mask, lt, Dl):
    """Every index the kernel chose scores, in float64, within 4 Dl 2^-24 exp(log_temp) of the maximum
    (the f32 accumulation bound for unit vectors); masked text tokens carry -1."""
    S, m = ref['S'], mask.bool()
    bound = 4 * Dl * 2.0 ** -24 * math.exp(lt)
    it, ii = out['idx_t2i'].long(), out['idx_i2t'].long()
    Bg, T = m.shape
    mm = m[:, None, :].expand(Bg, Bg, T)
    assert (it[~mm] == -1).all()
    assert (it[mm] >= 0).all() and (it[mm] < S.shape[3]).all() and (ii >= 0).all() and (ii < T).all()
    assert m.gather(1, ii.reshape(Bg, -1)).all()                 # image -> text never picks a masked token
    gap_t = S.amax(3) - S.gather(3, it.clamp_min(0)[..., None]).squeeze(3)
    Sm = S.masked_fill(~m[:, None, :, None], -math.inf)
    gap_i = Sm.amax(2) - S.gather(2, ii[:, :, None, :]).squeeze(2)
    print(f'index gaps: t2i {gap_t[mm].max().item():.2e} i2t {gap_i.max().item():.2e} bound {bound:.2e}')
    assert gap_t[mm].max().item() <= bound and gap_i.max().item() <= bound


def _check_outputs(out, ref):
    rl = ref['loss'].item()
    errs = dict(loss=abs(out['loss'].item() - rl), A=(out['A'].double() - ref['A']).abs().max().item(),
                C=(out['C'].double() - ref['C']).abs().max().item(), dt=rel(out['dt'], ref['dt']),
                di=rel(out['di'], ref['di']), dlt=rel(out['dlt'].reshape(()), ref['dlt']))
    print('  '.join(f'{k} {v:.2e}' for k, v in errs.items()))
    assert errs['loss'] < 1e-5 * max(1.0, abs(rl))
    assert errs['A'] < 1e-5 * max(1.0, ref['A'].abs().max().item())
    assert errs['C'] < 1e-5 * max(1.0, ref['C'].abs().max().item())
    assert errs['dt'] < 1e-4 and errs['di'] < 1e-4 and errs['dlt'] < 1e-4


# ------------------------------------------------------------------------------ kernel
@pytest.mark.parametrize('lt', [0.0, math.log(14.0)])
@pytest.mark.parametrize('shape', SHAPES)
def test_kernel_matches_restatement(K, shape, lt):
    Bg, T, I, Dl = shape
    t, i, mask = _inputs(*shape)
    for dcl, over in OPTIONS:
        out = _run(K, t, i, mask, lt, dcl, over)
        ref = filip_ref(t, i, mask, torch.tensor(lt), dcl, over, idx=(out['idx_t2i'], out['idx_i2t']))
        _check_indices(out, ref, mask, lt, Dl)
        _check_outputs(out, ref)
        assert (out['dt'][~mask.bool()] == 0).all()


@pytest.mark.parametrize('shape', [(3, 17, 65, 64), (4, 512, 64, 32)])
def test_masked_garbage_moves_nothing(K, shape):
    t, i, mask = _inputs(*shape)
    t2 = _inputs(*shape, seed=1, garbage=3.0)[0]
    t2 = torch.where(mask.bool()[..., None], t, t2)                  # other garbage, same kept tokens
    assert not torch.equal(t, t2) or mask.all()
    a, b = _run(K, t, i, mask, 1.0), _run(K, t2, i, mask, 1.0)
    for k in OUTPUTS:
        assert torch.equal(a[k], b[k]), k


def test_ties_go_to_the_lowest_index(K):
    Bg, T, I, Dl = 2, 8, 8, 32
    g = torch.Generator().manual_seed(11)
    t, i = torch.randn(Bg, T, Dl, generator=g), torch.randn(Bg, I, Dl, generator=g)
    i[:, 5] = i[:, 2]
    t[:, 6] = t[:, 1]
    mask = torch.ones(Bg, T, dtype=torch.uint8)
    lt = math.log(14.0)
    out = _run(K, t, i, mask, lt)
    # the higher-index duplicate is never a winner, so no max route carries gradient to it
    assert (out['idx_t2i'] != 5).all() and (out['idx_i2t'] != 6).all()
    ref = filip_ref(t, i, mask, torch.tensor(lt))                   # its own lowest-index rule, not forced
    assert torch.equal(ref['idx_t2i'] == 2, out['idx_t2i'].long() == 2)
    assert torch.equal(ref['idx_i2t'] == 1, out['idx_i2t'].long() == 1)
    forced = filip_ref(t, i, mask, torch.tensor(lt), idx=(out['idx_t2i'], out['idx_i2t']))
    _check_outputs(out, forced)
    assert rel(out['di'][:, 2] + out['di'][:, 5], forced['di'][:, 2] + forced['di'][:, 5]) < 1e-4
    assert rel(out['dt'][:, 1] + out['dt'][:, 6], forced['dt'][:, 1] + forced['dt'][:, 6]) < 1e-4
    # the duplicates' own gradients: what is left to the higher index is its own column / row alone
    assert rel(out['di'][:, 5], forced['di'][:, 5]) < 1e-4 and rel(out['dt'][:, 6], forced['dt'][:, 6]) < 1e-4
    # de-duplicated scoring: text -> image without image token 5, image -> text without text token 6
    keep = [k for k in range(I) if k != 5]
    a2 = _run(K, t, i[:, keep].contiguous(), mask, lt)['A']
    m2 = mask.clone()
    m2[:, 6] = 0
    c2 = _run(K, t, i, m2, lt)['C']
    assert (a2 - out['A']).abs().max().item() < 1e-6 * 14 and (c2 - out['C']).abs().max().item() < 1e-6 * 14


def test_bit_reproducible(K):
    t, i, mask = _inputs(5, 33, 63, 128, seed=2)
    a, b = _run(K, t, i, mask, 2.0, True, False), _run(K, t, i, mask, 2.0, True, False)
    for k in OUTPUTS:
        assert torch.equal(a[k], b[k]), k


def test_zero_norm_rows_give_finite_gradients(K):
    t, i, mask = _inputs(3, 16, 16, 64, seed=4)
    t[1, 2] = 0
    i[2, 5] = 0
    out = _run(K, t, i, mask, 1.0)
    assert all(torch.isfinite(out[k]).all() for k in ('loss', 'dt', 'di', 'dlt', 'A', 'C'))


@pytest.mark.parametrize('shape', [(129, 1, 1, 16), (1, 513, 1, 16), (1, 1, 1025, 16), (1, 1, 1, 24), (1, 1, 1, 528)])
def test_unsupported_shapes_are_refused(K, shape):
    from ctclip_mi355x._lib import KernelError
    Bg, T, I, Dl = shape
    t, i = torch.zeros(Bg, T, Dl, device=dev), torch.zeros(Bg, I, Dl, device=dev)
    mask = torch.ones(Bg, T, dtype=torch.uint8, device=dev)
    with pytest.raises(KernelError, match='1003'):                 # CT_ESHAPE, before any launch
        K.filip_loss(t, i, mask, torch.zeros(1, device=dev))


def test_workspace_bound():
    from ctclip_mi355x import _lib
    Bg, T, I, Dl = 8, 512, 576, 512
    bound = 4 * Bg * Bg * (T + I) + 4 * Bg * (T + I) * (Dl + 2) + 64 * 1024
    for given in (0, 16):           # every optional output in the workspace, or in the caller's tensors
        a = _lib.FilipArgs(Bg=Bg, T=T, I=I, Dl=Dl, A=given, C=given, idx_t2i=given, idx_i2t=given)
        n = _lib.lib().ctclip_filip_ws_bytes(_lib.ctypes.byref(a))
        assert 0 < n <= bound, (n, bound)
    a = _lib.FilipArgs(Bg=Bg, T=T, I=I, Dl=520)
    assert _lib.lib().ctclip_filip_ws_bytes(_lib.ctypes.byref(a)) == 0


# ------------------------------------------------------------------------------ model level
def cfg_small(layers=2):
    vit = O.ViTConfig(dim=512, codebook_size=8192, image_size=160, patch_size=20, temporal_patch_size=10,
                      spatial_depth=layers, temporal_depth=layers, dim_head=32, heads=8, frames=40)
    bert = O.BertConfig(vocab_size=1000, hidden=768, layers=layers, heads=12, intermediate=3072, max_position=64)
    return O.ClipConfig(vit=vit, bert=bert, dim_latent=512)


HEADS = ('to_text_latent.weight', 'to_visual_latent.weight', 'temperature')


def state_dict(cfg):
    """The recipe weights, with the visual projections redrawn at the token width [Dl, d]."""
    sd = W.make_state_dict(cfg)
    g = torch.Generator().manual_seed(77)
    for n in ('to_visual_latent.weight', 'to_visual_latent_extra.weight'):
        sd[n] = 0.02 * torch.randn(cfg.dim_latent, cfg.vit.dim, generator=g)
    return sd


def build(cfg, **options):
    from ctclip_mi355x.bert import BertConfig
    from ctclip_mi355x.models import build_ctclip, set_finetune_trainable
    v, b = cfg.vit, cfg.bert
    vit = dict(dim=v.dim, codebook_size=v.codebook_size, image_size=v.image_size, patch_size=v.patch_size,
               temporal_patch_size=v.temporal_patch_size, spatial_depth=v.spatial_depth,
               temporal_depth=v.temporal_depth, dim_head=v.dim_head, heads=v.heads)
    bert = BertConfig(vocab_size=b.vocab_size, hidden_size=b.hidden, num_hidden_layers=b.layers,
                      num_attention_heads=b.heads, intermediate_size=b.intermediate,
                      max_position_embeddings=b.max_position, hidden_dropout_prob=0.0,
                      attention_probs_dropout_prob=0.0)
    m = build_ctclip(vit, bert, cfg.dim_latent, use_all_token_embeds=True, **options)
    m.load_state_dict(state_dict(cfg), strict=True)
    m = set_finetune_trainable(m)
    named = dict(m.named_parameters())
    for n in HEADS:
        named[n].requires_grad = True
    return m.cuda()


def _batch(cfg, B=2):
    hu = W.make_hu(B, cfg.vit)
    ids, mask = W.make_text(B, 32, cfg.bert.vocab_size, ragged=True)
    return hu, mask, types.SimpleNamespace(input_ids=ids.cuda(), attention_mask=mask.cuda())


def test_model_forward_and_head_gradients(K):
    cfg = cfg_small()
    B, Dl = 2, cfg.dim_latent
    model = build(cfg, decoupled_contrastive_learning=True).eval()
    hu, mask, text = _batch(cfg, B)
    lt = model.temperature.detach().cpu()
    with torch.no_grad():
        tn, inn, tokens = model(text, hu.cuda(), return_latents=True)
        sim = model(text, hu.cuda())
    assert tn.shape == (B, 32, Dl) and inn.shape == (B, 64, Dl) and tokens.shape == (B, 64, cfg.vit.dim)
    model.zero_grad(set_to_none=True)
    loss = model(text, hu.cuda(), return_loss=True)
    loss.backward()
    torch.cuda.synchronize()
    # forward: the loss of the model's own latents, the pair-wise token similarity
    ref = filip_ref(tn.cpu(), inn.cpu(), mask, lt, decoupled=True)
    print(f'loss {loss.item():.6f} ref {ref["loss"].item():.6f}')
    assert abs(loss.item() - ref['loss'].item()) < 1e-3
    want = torch.einsum('btd,bid->bti', tn.double(), inn.double()).cpu() * lt.double().exp()
    assert sim.shape == (B, 32, 64) and (sim.cpu().double() - want).abs().max().item() < 1e-3
    # backward: from the same raw latents, through the restatement with the kernel's indices
    with torch.no_grad():
        enc = model.text_transformer(text.input_ids, attention_mask=text.attention_mask)[0].contiguous()
        pooled = model.visual_transformer.encode_pooled(hu.cuda())[0].view(B, 64, cfg.vit.dim).contiguous()
        Wt, Wv = model.to_text_latent.weight.detach(), model.to_visual_latent.weight.detach()
        t_raw, i_raw = (enc @ Wt.t()).contiguous(), (pooled @ Wv.t()).contiguous()
        out = K.filip_loss(t_raw, i_raw, mask.to(torch.uint8).cuda(), lt.reshape(1).cuda(), decoupled=True,
                           want_idx=True)
    r = filip_ref(t_raw.cpu(), i_raw.cpu(), mask, lt, decoupled=True,
                  idx=(out['idx_t2i'].cpu(), out['idx_i2t'].cpu()))
    grads = {'to_text_latent.weight': r['dt'].reshape(-1, Dl).t() @ enc.cpu().double().reshape(-1, enc.shape[-1]),
             'to_visual_latent.weight': r['di'].reshape(-1, Dl).t() @ pooled.cpu().double().reshape(-1, cfg.vit.dim),
             'temperature': r['dlt']}
    named = dict(model.named_parameters())
    for n in HEADS:
        e = rel(named[n].grad, grads[n])
        print(f'{n}: grad rel err {e:.2e}')
        assert e < 5e-2, n


def test_train_step_bit_reproducible():
    from ctclip_mi355x.trainer import CTClipTrainer
    cfg = cfg_small(layers=1)
    hu, mask, text = _batch(cfg)
    sd = state_dict(cfg)
    runs = []
    for _ in range(2):
        torch.manual_seed(0)
        model = build(cfg)
        named = dict(model.named_parameters())
        tr = CTClipTrainer(model, lr=1e-4)
        losses = [tr.train_step(text, hu.cuda()).detach().clone() for _ in range(2)]
        tr.flush()
        torch.cuda.synchronize()
        assert all(torch.isfinite(x).all() for x in losses)
        for n in HEADS[:2]:
            assert not torch.equal(named[n].detach().cpu(), sd[n]), n
        changed = {tower: any(not torch.equal(p.detach().cpu(), sd[n]) for n, p in named.items()
                              if n.startswith(tower) and p.requires_grad and n in sd)
                   for tower in ('visual_transformer.', 'text_transformer.')}
        assert all(changed.values()), changed
        runs.append((*losses, tr.flat.data.clone(), tr.m.clone(), tr.v.clone()))
        del model, tr
    for a, b in zip(*runs):
        assert torch.equal(a, b)
