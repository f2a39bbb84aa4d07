"""Gradient audit: every parameter of the model and every autograd Function of functional.py against
the CPU oracle evaluated in float64 (GPU).

Part A  the whole contrastive step at the reduced parity config (test_gpu_model.cfg_small, B = 2,
        ragged text, train mode), every parameter made trainable so the REFERENCE decides which ones
        receive a gradient: 18 receive none, 3 are zero in exact arithmetic (softmax shift
        invariance), 99 are compared at the project's 5e-2 -- plain, inside kernels.ln_guard(), and
        in the precise 'f32' / 'split' towers.  (At B = 2 the step has 512 token rows, below the
        2,048-row granule of kernels.ln_fusable, so the guarded run takes the unfused kernels; the
        fused to_out + LayerNorm launch is compared with float64 in Part B at 2,048 rows.)
Part B  each Function alone, built from the project's own modules with perturbed parameters,
        bf16-representable inputs with a non-zero mean and a random upstream gradient: every output,
        every input gradient and every parameter gradient against float64 autograd through the
        matching oracle function.  Bounds: grad_audit_common (the project's existing ones); measured
        values: DESIGN.md, "Gradient audit".
Part C  sink semantics of the Functions that write .grad themselves: accumulation into a pre-filled
        .grad, two backwards without zeroing, no deferred reduction left pending.

Every row is printed as 'AUDIT <test> | <quantity> | <measured> | <bound>' before it is asserted."""
import contextlib
import types

import pytest
import torch
import torch.nn.functional as F

from oracle import ctclip_oracle as O
from oracle import weights as W

import grad_audit_common as C
from grad_audit_common import Rows, bf16r, leaf, module_sd, perturb, rel
from test_gpu_model import cfg_small

pytestmark = pytest.mark.gpu


def sync():
    torch.cuda.synchronize()


def rnd(*shape, seed, scale=1.0, mean=0.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + mean).cuda()


# ============================================================================= Part A
# zero in exact arithmetic: a key bias shifts every score of a softmax row by the same amount, and
# so does the CPB output bias.  (name, sibling whose gradient sets the scale)
STRUCTURAL_ZERO = [
    ('text_transformer.encoder.layer.0.attention.self.key.bias',
     'text_transformer.encoder.layer.0.attention.self.query.bias'),
    ('text_transformer.encoder.layer.1.attention.self.key.bias',
     'text_transformer.encoder.layer.1.attention.self.query.bias'),
    ('visual_transformer.spatial_rel_pos_bias.net.2.bias',
     'visual_transformer.spatial_rel_pos_bias.net.1.0.bias'),
]
# name -> (measured error, bound = 1.5 x measured, reason); at most 3 entries, never a weight matrix,
# and only a parameter whose gradient meets its Part B bound on controlled inputs
KNOWN_NOISY = {}


@pytest.fixture(scope='module')
def full():
    from ctclip_mi355x.models import build_ctclip
    from ctclip_mi355x.bert import BertConfig
    torch.manual_seed(0)
    cfg = cfg_small()
    v, b = cfg.vit, cfg.bert
    vit = dict(dim=v.dim, codebook_size=v.codebook_size, image_size=v.image_size, patch_size=v.patch_size,
               temporal_patch_size=v.temporal_patch_size, spatial_depth=v.spatial_depth,
               temporal_depth=v.temporal_depth, dim_head=v.dim_head, heads=v.heads)
    bert = BertConfig(vocab_size=b.vocab_size, hidden_size=b.hidden, num_hidden_layers=b.layers,
                      num_attention_heads=b.heads, intermediate_size=b.intermediate,
                      max_position_embeddings=b.max_position, hidden_dropout_prob=0.0,
                      attention_probs_dropout_prob=0.0)
    model = build_ctclip(vit, bert, cfg.dim_latent)
    sd = W.make_state_dict(cfg)
    model.load_state_dict(sd, strict=True)
    for p in model.parameters():          # all of them: the reference decides who gets a gradient
        p.requires_grad_(True)
    model = model.cuda()
    hu = W.make_hu(2, cfg.vit)
    ids, mask = W.make_text(2, 32, cfg.bert.vocab_size, ragged=True)
    assert (mask == 0).any()
    text = types.SimpleNamespace(input_ids=ids.cuda(), attention_mask=mask.cuda())
    return dict(cfg=cfg, model=model, sd=sd, hu=hu, ids=ids, mask=mask, text=text, refs={})


def _reference(full, idx):
    """float64 oracle forward + backward forced onto VQ indices idx, shared by the runs that agree on them."""
    key = idx.numpy().tobytes()
    if key not in full['refs']:
        sd = {k: (v.double() if v.is_floating_point() else v.clone()) for k, v in full['sd'].items()}
        for k, v in sd.items():
            if v.is_floating_point() and 'vq._codebook' not in k and not k.endswith('beta') and v.numel():
                v.requires_grad_(True)
        out = O.ctclip_forward(sd, full['ids'], full['mask'], O.normalize_hu(full['hu']).double(), full['cfg'],
                               training=True, force_ind=idx)
        out['loss'].backward()
        full['refs'][key] = (out['loss'].item(), {k: v.grad for k, v in sd.items() if v.requires_grad})
    return full['refs'][key]


@pytest.mark.parametrize('variant', ['plain', 'ln_guard', 'f32', 'split'])
def test_model_every_parameter(full, variant):
    from ctclip_mi355x import kernels as K, precise
    model = full['model']
    cbk = model.visual_transformer.vq._codebook
    emb0, cs0 = cbk.embed.clone(), cbk.cluster_size.clone()
    model.train()
    model.zero_grad(set_to_none=True)
    with contextlib.ExitStack() as st:
        if variant == 'ln_guard':
            st.enter_context(K.ln_guard())
        elif variant != 'plain':
            st.enter_context(precise.vit_precision_scope(variant))
        try:
            loss = model(full['text'], full['hu'].cuda(), return_loss=True)
            idx = model.visual_transformer.vq.state.last_indices.cpu()
            loss.backward()
            sync()
        finally:
            sync()
            cbk.embed.copy_(emb0)          # the train-mode forward's EMA update
            cbk.cluster_size.copy_(cs0)
    if variant == 'ln_guard':
        assert K.ln_fused_status() == 0
    assert not K._DEFERRED
    ref_loss, ref = _reference(full, idx)
    named = {n: p for n, p in model.named_parameters() if p.requires_grad and p.is_floating_point() and p.numel()}
    assert set(named) == set(ref), set(named) ^ set(ref)
    zero = dict(STRUCTURAL_ZERO)
    assert len(zero) == 3 and len(KNOWN_NOISY) <= 3
    for n in KNOWN_NOISY:
        assert named[n].ndim < 2 and n not in zero and ref[n] is not None, n
    none = [n for n in named if ref[n] is None]
    live = [n for n in named if ref[n] is not None and n not in zero]
    assert (len(none), len(zero), len(live)) == (18, 3, 99), (len(none), len(zero), len(live))
    rows = Rows(f'model[{variant}]')
    rows.add('loss (absolute)', abs(loss.item() - ref_loss), 1e-3)
    for n in none:
        g = named[n].grad
        rows.add(f'd {n} (none in the reference)', 0.0 if g is None or not g.count_nonzero().item() else float('inf'),
                 0.0)
    for n, sib in zero.items():
        s = ref[sib].norm().item()
        assert ref[n].norm().item() < 1e-12 * s, (n, ref[n].norm().item(), s)     # the list cannot grow silently
        g = named[n].grad
        rows.add(f'd {n} / |d sibling|', float('inf') if g is None else g.double().norm().item() / s, 5e-2)
    for n in live:
        g = named[n].grad
        bound = KNOWN_NOISY[n][1] if n in KNOWN_NOISY else C.MODEL_GRAD
        rows.add(f'd {n}', float('inf') if g is None else rel(g, ref[n]), bound)
    model.zero_grad(set_to_none=True)
    rows.check()


# ============================================================================= Part B: ViTLayerFn
VIT_SHAPES = {                      # B, T, Hg, Wg, mode, CPB table
    'sp5x7': (2, 2, 5, 7, 0, True),
    'sp8x8': (2, 4, 8, 8, 0, False),
    'tmT5': (2, 5, 4, 4, 1, False),
    'tmT32': (2, 32, 4, 4, 1, False),
    # 2,048 rows: what kernels.ln_fusable accepts (the fused to_out + LayerNorm launch under ln_guard)
    'sp8x8_2048': (8, 4, 8, 8, 0, True),
    'tmT32_2048': (4, 32, 4, 4, 1, False),
}
_VIT_CASES = {}


def vit_case(shape, heads):
    """Module, inputs and the float64 reference of one (shape, heads) case, computed once."""
    from ctclip_mi355x import attention as A, functional as Fn
    key = (shape, heads)
    if key in _VIT_CASES:
        return _VIT_CASES[key]
    B, T, Hg, Wg, mode, with_bias = VIT_SHAPES[shape]
    seed = 100 + sorted(VIT_SHAPES).index(shape) * 2 + (heads == 16)
    torch.manual_seed(seed)
    tr = C.spread_scales(perturb(A.Transformer(512, depth=1, dim_head=32, heads=heads), seed), seed).cuda()
    geo = Fn.Geo(B=B, T=T, Hg=Hg, Wg=Wg, heads=heads, dim_head=32, mode=mode)
    xf0 = bf16r(rnd(geo.M, 512, seed=seed + 1, mean=0.3))
    dy = rnd(geo.M, 512, seed=seed + 2, scale=1e-2)
    bias0 = rnd(heads, (2 * Hg - 1) * (2 * Wg - 1), seed=seed + 3, scale=0.5, mean=0.1) if with_bias else None
    sd = module_sd(tr, 'x.')
    x = leaf(xf0)
    u = leaf(bias0) if with_bias else None
    dense = u[:, C.cpb_bins(Hg, Wg)] if with_bias else None
    y = C.ref_transformer(sd, 'x.', x, geo, 1, dense)
    y.backward(dy.double().cpu())
    case = dict(tr=tr, geo=geo, xf0=xf0, dy=dy, bias0=bias0, sd=sd, y=y.detach(), dx=x.grad,
                du=u.grad if with_bias else None)
    _VIT_CASES[key] = case
    return case


def vit_run(case):
    tr = case['tr']
    xf = case['xf0'].clone().requires_grad_(True)
    bias = case['bias0'].clone().requires_grad_(True) if case['bias0'] is not None else None   # a fresh table per
    yf, yb = tr.run(xf, case['xf0'].bfloat16(), case['geo'], bias)                     # forward, as the model's
    yf.backward(case['dy'])
    return yf.detach(), yb, xf.grad, None if bias is None else bias.grad


_VIT_PARAMS = [(s, v) for s in ('sp5x7', 'sp8x8', 'tmT5', 'tmT32')
               for v in ('default', 'bf16', 'unfold', 'heads16', 'f32', 'split')] + \
              [('sp8x8_2048', 'guard'), ('tmT32_2048', 'guard')]


@pytest.mark.parametrize('shape,variant', _VIT_PARAMS)
def test_vit_layer(shape, variant, monkeypatch):
    from ctclip_mi355x import kernels as K
    case = vit_case(shape, 16 if variant == 'heads16' else 8)
    fused = []
    if variant == 'guard':
        real = K.linear_residual_ln
        monkeypatch.setattr(K, 'linear_residual_ln', lambda *a, **k: (fused.append(real(*a, **k)), fused[-1])[1])
    for p in case['tr'].parameters():
        p.grad = None
    with C.vit_variant(variant):
        yf, yb, dx, du = vit_run(case)
        sync()
    if variant == 'guard':
        assert fused and all(f is not None for f in fused), 'the fused to_out + LayerNorm launch did not run'
        assert K.ln_fused_status() == 0
    rows = Rows(f'ViTLayerFn[{shape}-{variant}]')
    rows.add('y', rel(yf, case['y']), C.F32 if variant in ('f32', 'split') else C.OUT_BF16)
    rows.add('y bf16 vs y', rel(yb.float(), yf), 2.0 ** -8)
    rows.add('dx', rel(dx, case['dx']), C.DX)
    if du is not None:
        rows.add('d bias table', rel(du, case['du']), C.DX)
    rows.params(case['tr'].named_parameters(), case['sd'], 'x.', C.DW)
    for p in case['tr'].parameters():
        p.grad = None
    rows.check()


# ============================================================================= Part B: CPBFn
def _cpb_pair(depth, seed, Hg=5, Wg=7, B=2, T=2):
    from ctclip_mi355x import attention as A, functional as Fn
    torch.manual_seed(seed)
    cpb = perturb(A.ContinuousPositionBias(dim=512, heads=8), seed).cuda()
    tr = C.spread_scales(perturb(A.Transformer(512, depth=depth, dim_head=32, heads=8), seed + 1), seed).cuda()
    geo = Fn.Geo(B=B, T=T, Hg=Hg, Wg=Wg, heads=8, dim_head=32, mode=0)
    xf0 = bf16r(rnd(geo.M, 512, seed=seed + 2, mean=0.3))
    dy = rnd(geo.M, 512, seed=seed + 3, scale=1e-2)
    return cpb, tr, geo, xf0, dy


def test_cpb_mlp_alone():
    """CPBFn by itself is f32 end to end: the dense bias and all six MLP gradients at the f32 bound."""
    cpb, _, _, _, _ = _cpb_pair(1, 300)
    h, w = 5, 7
    dd = rnd(8, h * w, h * w, seed=301)
    dense = cpb.dense(h, w)
    dense.backward(dd)
    sync()
    sd = module_sd(cpb, 'c.')
    ref = O.cpb_forward(sd, 'c.', h, w)
    ref.backward(dd.double().cpu())
    rows = Rows('CPBFn[alone 5x7]')
    rows.add('dense bias', rel(dense, ref), C.F32)
    rows.params(cpb.named_parameters(), sd, 'c.', C.F32)
    rows.check()


def test_cpb_two_layers_share_table():
    """Two layers read one CPB table: its gradient is the SUM of both layers' shares (one buffer,
    functional._ctclip_bias_acc), and it reaches all six MLP parameters."""
    cpb, tr, geo, xf0, dy = _cpb_pair(2, 310)
    got = []
    xf = xf0.clone().requires_grad_(True)
    u = cpb(geo.Hg, geo.Wg)
    u.register_hook(lambda g: got.append(g.detach().clone()))
    yf, _ = tr.run(xf, xf0.bfloat16(), geo, u)
    yf.backward(dy)
    sync()
    sd = module_sd(tr, 'x.')
    sd.update(module_sd(cpb, 'c.'))
    x = leaf(xf0)
    dense = O.cpb_forward(sd, 'c.', geo.Hg, geo.Wg)
    dense.retain_grad()
    y = C.ref_transformer(sd, 'x.', x, geo, 2, dense)
    y.backward(dy.double().cpu())
    bins = C.cpb_bins(geo.Hg, geo.Wg).reshape(-1)
    du_ref = torch.zeros(8, (2 * geo.Hg - 1) * (2 * geo.Wg - 1), dtype=torch.float64)
    du_ref.index_add_(1, bins, dense.grad.reshape(8, -1))
    assert len(got) == 1, 'the table gradient reaches autograd once, from the first layer'
    rows = Rows('CPBFn[2 layers 5x7]')
    rows.add('y', rel(yf, y), C.OUT_BF16)
    rows.add('dx', rel(xf.grad, x.grad), C.DX)
    rows.add('d bias table (sum of 2 layers)', rel(got[0], du_ref), C.DX)
    rows.params(cpb.named_parameters(), sd, 'c.', C.DW, {'net.2.bias': 'net.1.0.bias'})
    rows.params(tr.named_parameters(), sd, 'x.', C.DW)
    rows.check()


# ============================================================================= Part B: patch embedding, recon
def _small_vit(seed):
    from ctclip_mi355x import ctvit
    torch.manual_seed(seed)
    vt = ctvit.CTViT(dim=512, codebook_size=1024, image_size=100, patch_size=20, temporal_patch_size=10,
                     spatial_depth=1, temporal_depth=1, dim_head=32, heads=8)
    cfg = O.ViTConfig(dim=512, codebook_size=1024, image_size=100, patch_size=20, temporal_patch_size=10,
                      spatial_depth=1, temporal_depth=1, dim_head=32, heads=8, frames=30)
    return perturb(vt, seed).cuda(), cfg


def _video(kind, cfg, seed):
    g = torch.Generator().manual_seed(seed)
    shape = (2, 1, cfg.frames, cfg.image_size, cfg.image_size)
    if kind == 'hu':                 # offset so the patches' mean is not zero; some values clamp
        hu = torch.randint(-1200, 1201, shape, generator=g, dtype=torch.int16) // 2 + 300
        return hu, O.normalize_hu(hu).double()
    v = bf16r((torch.rand(shape, generator=g) * 1.6 - 0.6).cuda()).clamp(-1, 1).contiguous()
    return v.cpu(), v.cpu().double()


def _patch_run(vt, video):
    from ctclip_mi355x import functional as Fn
    pe = vt.to_patch_emb
    return Fn.PatchEmbedFn.apply(video, pe[1].weight, pe[1].bias, pe[2].weight, pe[2].bias, pe[3].weight,
                                 pe[3].bias, vt.temporal_patch_size, vt.patch_size[0],
                                 video.dtype == torch.int16, vt._offsets(video.shape, video.device))


@pytest.mark.parametrize('kind', ['hu', 'f32'])
def test_patch_embed(kind):
    vt, cfg = _small_vit(400)
    video, vref = _video(kind, cfg, 401)
    M = 2 * cfg.t_tokens * cfg.grid ** 2
    dy = rnd(M, 512, seed=402, scale=1e-2)
    yf, yb = _patch_run(vt, video.cuda().contiguous())
    yf.backward(dy)
    sync()
    sd = module_sd(vt, 'v.')
    ref = O.patch_embed(sd, 'v.', vref, cfg).reshape(M, 512)
    ref.backward(dy.double().cpu())
    rows = Rows(f'PatchEmbedFn[{kind}]')
    rows.add('y', rel(yf, ref), C.OUT_BF16)
    rows.add('y bf16 vs y', rel(yb.float(), yf), 2.0 ** -8)
    rows.params(vt.to_patch_emb.named_parameters(), sd, 'v.to_patch_emb.', C.DW)
    rows.check()


def test_recon():
    from ctclip_mi355x import functional as Fn
    vt, cfg = _small_vit(410)
    video, vref = _video('hu', cfg, 411)
    B, T, g = 2, cfg.t_tokens, cfg.grid
    M = B * T * g * g
    xf0 = bf16r(rnd(M, 512, seed=412, scale=0.5, mean=0.2))
    xf = xf0.clone().requires_grad_(True)
    vid = video.cuda().contiguous()
    loss, recon = Fn.ReconFn.apply(xf, xf0.bfloat16(), vt.to_pixels[0].weight, vt.to_pixels[0].bias, vid, True,
                                   vt.temporal_patch_size, vt.patch_size[0], vt._offsets(vid.shape, vid.device), True)
    (loss * 0.7).backward()
    sync()
    sd = module_sd(vt, 'v.')
    x = leaf(xf0)
    rr = O.to_pixels(sd, 'v.', x.reshape(B, T, g, g, 512), cfg)
    rl = F.mse_loss(vref, rr)
    (rl * 0.7).backward()
    rows = Rows('ReconFn')
    rows.add('loss', abs(loss.item() - rl.item()) / abs(rl.item()), C.OUT_BF16)
    rows.add('recon', rel(recon, rr), C.OUT_BF16)
    rows.add('dx', rel(xf.grad, x.grad), C.DX)
    rows.params(vt.to_pixels.named_parameters(), sd, 'v.to_pixels.', C.DW)
    rows.check()


# ============================================================================= Part B: NormFn, VQPoolFn
def test_norm_fn():
    from ctclip_mi355x import attention as A, functional as Fn
    ln = perturb(A.LayerNorm(512), 500, scale=0.1).cuda()
    xf0 = bf16r(rnd(150, 512, seed=501, scale=1.3, mean=0.4))
    dy = rnd(150, 512, seed=502)
    xf = xf0.clone().requires_grad_(True)
    yf, yb = Fn.NormFn.apply(xf, xf0.bfloat16(), ln.gamma)
    yf.backward(dy)
    sync()
    sd = module_sd(ln, 'n.')
    x = leaf(xf0)
    y = O._ln(x, sd['n.gamma'], sd['n.beta'])
    y.backward(dy.double().cpu())
    rows = Rows('NormFn')
    rows.add('y (f32 in, f32 out)', rel(yf, y), C.F32)
    rows.add('y bf16 vs y', rel(yb.float(), yf), 2.0 ** -8)
    rows.add('dx', rel(xf.grad, x.grad), C.DX)
    rows.params(ln.named_parameters(), sd, 'n.', C.DW)
    rows.check()


def test_vq_pool_straight_through():
    """VQPoolFn in training mode: the pooled codes and the quantised tokens are the codebook rows of
    the chosen indices (exact f32), the input gradient is the straight-through one of both outputs."""
    from ctclip_mi355x import functional as Fn
    B, T, Hg, Wg, D, Cn = 2, 3, 3, 4, 512, 1024
    geo = Fn.Geo(B=B, T=T, Hg=Hg, Wg=Wg, heads=8, dim_head=32, mode=0)
    zf0 = bf16r(rnd(geo.M, D, seed=510, mean=0.1))
    embed = F.normalize(rnd(1, Cn, D, seed=511), dim=-1)
    emb0 = embed.clone()          # (the train-mode call updates the codebook in place afterwards)
    cluster = torch.zeros(1, Cn, device='cuda')
    dp = rnd(B, Hg * Wg * D, seed=512)
    dt = rnd(geo.M, D, seed=513)
    zf = zf0.clone().requires_grad_(True)
    state = Fn.VQState()
    pooled, pooled_b, toks = Fn.VQPoolFn.apply(zf, zf0.bfloat16(), embed, cluster, geo, True, 0.8, state, True)
    idx = state.last_indices.cpu()
    torch.autograd.backward([pooled, toks], [dp, dt])
    sync()
    z = leaf(zf0)
    q, _, _, _ = O.vq_forward(z.reshape(B, -1, D), emb0.double().cpu(), torch.zeros(1, Cn, dtype=torch.float64),
                               True, 0.8, force_ind=idx.reshape(B, -1))
    rp = q.reshape(B, T, Hg * Wg, D).mean(dim=1).reshape(B, -1)
    torch.autograd.backward([rp, q.reshape(-1, D)], [dp.double().cpu(), dt.double().cpu()])
    rows = Rows('VQPoolFn')
    rows.add('pooled', rel(pooled, rp), C.F32)
    rows.add('pooled bf16 vs pooled', rel(pooled_b.float(), pooled), 2.0 ** -8)
    rows.add('tokens', rel(toks, q.reshape(-1, D)), C.F32)
    rows.add('dz (straight-through)', rel(zf.grad, z.grad), C.F32)
    rows.check()


# ============================================================================= Part B: projections, loss
@pytest.mark.parametrize('mode', ['bf16', 'f32'])
def test_projections(mode):
    """ImageProjFn and TextProjFn against clip_latents (raw latents l2-normalised by torch on both sides)."""
    from ctclip_mi355x import functional as Fn, kernels as K, precise
    B, hw, D, Dt, Dl = 2, 9, 512, 768, 512
    Wi = rnd(Dl, hw * D, seed=600, scale=(hw * D) ** -0.5).requires_grad_(True)
    Wt = rnd(Dl, Dt, seed=601, scale=Dt ** -0.5).requires_grad_(True)
    pooled0 = bf16r(rnd(B, hw * D, seed=602, scale=0.05, mean=0.01))
    cls0 = rnd(B, Dt, seed=603, mean=0.1)
    dti, dii = rnd(B, Dl, seed=604), rnd(B, Dl, seed=605)
    pooled, cls = pooled0.clone().requires_grad_(True), cls0.clone().requires_grad_(True)
    with precise.vit_precision_scope(mode):
        i_raw = Fn.ImageProjFn.apply(pooled, pooled0.bfloat16(), Wi, K.cast_bf16(Wi.detach()))
        t_raw = Fn.TextProjFn.apply(cls, Wt)
        torch.autograd.backward([F.normalize(t_raw, dim=-1), F.normalize(i_raw, dim=-1)], [dti, dii])
    sync()
    sd = {'to_text_latent.weight': leaf(Wt), 'to_visual_latent.weight': leaf(Wi)}
    p, c = leaf(pooled0), leaf(cls0)
    t_lat, i_lat = O.clip_latents(sd, c.reshape(B, 1, Dt), p.reshape(B, 1, 3, 3, D))
    torch.autograd.backward([t_lat, i_lat], [dti.double().cpu(), dii.double().cpu()])
    rows = Rows(f'Proj[{mode}]')
    rows.add('image latents', rel(F.normalize(i_raw, dim=-1), i_lat), C.F32 if mode == 'f32' else C.OUT_BF16)
    rows.add('d pooled', rel(pooled.grad, p.grad), C.DX)
    rows.add('d to_visual_latent.weight', rel(Wi.grad, sd['to_visual_latent.weight'].grad), C.DW)
    rows.add('text latents', rel(F.normalize(t_raw, dim=-1), t_lat), C.F32)
    rows.add('d cls', rel(cls.grad, c.grad), C.F32)
    rows.add('d to_text_latent.weight', rel(Wt.grad, sd['to_text_latent.weight'].grad), C.F32)
    rows.check()


@pytest.mark.parametrize('fn', ['ClipLossFn', 'ClipLossExFn'])
@pytest.mark.parametrize('B', [2, 5, 16])
def test_clip_loss(fn, B):
    from ctclip_mi355x import functional as Fn
    Dl = 512
    t0, i0 = rnd(B, Dl, seed=700 + B, mean=0.1), rnd(B, Dl, seed=710 + B, mean=-0.05)
    t, i = t0.clone().requires_grad_(True), i0.clone().requires_grad_(True)
    temp = torch.tensor(0.8, device='cuda', requires_grad=True)
    if fn == 'ClipLossFn':
        loss = Fn.ClipLossFn.apply(t, i, temp, None, None)
    else:
        loss = Fn.ClipLossExFn.apply(t.view(1, B, Dl), i.view(1, B, Dl), None, None, temp, False, 1.0, 0.0, None, None)
    (loss * 0.7).backward()
    sync()
    tr, ir, tp = leaf(t0), leaf(i0), leaf(temp)
    rl = O.infonce(F.normalize(tr, dim=-1), F.normalize(ir, dim=-1), tp)
    (rl * 0.7).backward()
    rows = Rows(f'{fn}[B={B}]')
    rows.add('loss', abs(loss.item() - rl.item()) / abs(rl.item()), C.F32)
    rows.add('d text latents', rel(t.grad, tr.grad), C.F32)
    rows.add('d image latents', rel(i.grad, ir.grad), C.F32)
    rows.add('d temperature', rel(temp.grad, tp.grad), C.F32)
    rows.check()


# ============================================================================= Part B: BERT
def _bert(seed):
    from ctclip_mi355x import bert
    torch.manual_seed(seed)
    c = bert.BertConfig(vocab_size=1000, hidden_size=768, num_hidden_layers=1, num_attention_heads=12,
                        intermediate_size=3072, max_position_embeddings=64, hidden_dropout_prob=0.0,
                        attention_probs_dropout_prob=0.0)
    cfg = O.BertConfig(vocab_size=1000, hidden=768, layers=1, heads=12, intermediate=3072, max_position=64)
    return perturb(bert.BertModel(c), seed).cuda(), cfg


def _text(kind, L, seed):
    """B = 3 rows: full, half and two tokens long, padded on the right -- or row 1 padded on the left."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(5, 1000, (3, L), generator=g)
    mask = torch.ones(3, L, dtype=torch.long)
    mask[1, L // 2 + 1:] = 0
    mask[2, 2:] = 0
    if kind == 'left':
        mask[1] = mask[1].flip(0)
    ids[mask == 0] = 0
    return ids, mask


def _bert_layer_run(model, xf, xb, kmask, B, L):
    from ctclip_mi355x import functional as Fn
    c, lyr = model.config, model.encoder.layer[0]
    a = lyr.attention
    return Fn.BertLayerFn.apply(
        xf, xb, kmask, B, L, c.num_attention_heads, c.layer_norm_eps,
        a.self.query.weight, a.self.query.bias, a.self.key.weight, a.self.key.bias,
        a.self.value.weight, a.self.value.bias, a.output.dense.weight, a.output.dense.bias,
        a.output.LayerNorm.weight, a.output.LayerNorm.bias, lyr.intermediate.dense.weight,
        lyr.intermediate.dense.bias, lyr.output.dense.weight, lyr.output.dense.bias,
        lyr.output.LayerNorm.weight, lyr.output.LayerNorm.bias, (0.0, 0.0, 0, 0, 0))


def _bert_embed_run(model, ids):
    from ctclip_mi355x import functional as Fn
    c, e = model.config, model.embeddings
    return Fn.BertEmbedFn.apply(ids, e.word_embeddings.weight, e.position_embeddings.weight,
                                e.token_type_embeddings.weight, e.LayerNorm.weight, e.LayerNorm.bias,
                                c.layer_norm_eps, (0.0, 0), c.pad_token_id)


@pytest.mark.parametrize('kind', ['right', 'left'])
@pytest.mark.parametrize('L', [5, 32])
def test_bert_embed(kind, L):
    """BertEmbedFn reads f32 tables and an f32 gradient only: everything at the f32 bound; the pad
    id's row of the word table gets exactly nothing."""
    model, cfg = _bert(800)
    ids, mask = _text(kind, L, 801 + L)
    dy = rnd(3 * L, 768, seed=802)
    yf, yb = _bert_embed_run(model, ids.cuda())
    yf.backward(dy)
    sync()
    sd = module_sd(model, 'b.')
    ref = O.bert_embed(sd, 'b.', ids, cfg).reshape(3 * L, 768)
    ref.backward(dy.double().cpu())
    rows = Rows(f'BertEmbedFn[{kind} L={L}]')
    rows.add('y', rel(yf, ref), C.F32)
    rows.add('y bf16 vs y', rel(yb.float(), yf), 2.0 ** -8)
    rows.params(model.embeddings.named_parameters(), sd, 'b.embeddings.', C.F32)
    rows.add('pad row of d word_embeddings', model.embeddings.word_embeddings.weight.grad[0].abs().max().item(), 0.0)
    rows.check()


@pytest.mark.parametrize('kind', ['right', 'left'])
@pytest.mark.parametrize('L', [5, 32])
def test_bert_layer(kind, L):
    model, cfg = _bert(810)
    ids, mask = _text(kind, L, 811 + L)
    B = 3
    kmask = mask.to(torch.int32).cuda().contiguous()
    xf0 = bf16r(rnd(B * L, 768, seed=812, mean=0.2))
    dy = rnd(B * L, 768, seed=813, scale=1e-2)
    xf = xf0.clone().requires_grad_(True)
    yf, yb = _bert_layer_run(model, xf, xf0.bfloat16(), kmask, B, L)
    yf.backward(dy)
    sync()
    sd = module_sd(model, 'b.')
    x = leaf(xf0)
    lp = 'b.encoder.layer.0.'
    y = O.bert_layer(sd, lp, x.reshape(B, L, 768), O.bert_add_mask(mask), cfg).reshape(B * L, 768)
    y.backward(dy.double().cpu())
    rows = Rows(f'BertLayerFn[{kind} L={L}]')
    rows.add('y', rel(yf, y), C.OUT_BF16)
    rows.add('y bf16 vs y', rel(yb.float(), yf), 2.0 ** -8)
    rows.add('dx', rel(xf.grad, x.grad), C.DX)
    rows.params(model.encoder.layer[0].named_parameters(), sd, lp, C.DW,
                {'attention.self.key.bias': 'attention.self.query.bias'})
    # pad rows contribute nothing: other values in them leave every token row's output bit-identical,
    # and with no upstream gradient on them they get no input gradient
    pad = (mask.reshape(-1) == 0).cuda()
    for p in model.parameters():
        p.grad = None
    x2 = xf0.clone()
    x2[pad] = bf16r(rnd(int(pad.sum()), 768, seed=814, scale=3.0))
    x2.requires_grad_(True)
    y2, _ = _bert_layer_run(model, x2, x2.detach().bfloat16(), kmask, B, L)
    y2.backward(dy * (~pad)[:, None])
    sync()
    rows.add('token rows after changing the pad rows', (y2.detach()[~pad] - yf.detach()[~pad]).abs().max().item(), 0.0)
    rows.add('dx of pad rows without upstream gradient', x2.grad[pad].abs().max().item(), 0.0)
    rows.check()


# ============================================================================= Part C: sink semantics
@pytest.mark.parametrize('variant', ['default', 'unfold'])
@pytest.mark.parametrize('mode', [0, 1])
def test_sinks_vit_layers_and_cpb(mode, variant):
    """Two ViT layers (mode 0: sharing the table of a CPB module, so CPBFn's sinks too)."""
    from ctclip_mi355x import functional as Fn, kernels as K
    cpb, tr, geo, xf0, dy = _cpb_pair(2, 900 + mode, Hg=8, Wg=8, B=2, T=4)
    geo = Fn.Geo(B=2, T=4, Hg=8, Wg=8, heads=8, dim_head=32, mode=mode)

    def run():
        with C.vit_variant(variant):
            u = cpb(geo.Hg, geo.Wg) if mode == 0 else None
            yf, _ = tr.run(xf0.clone().requires_grad_(True), xf0.bfloat16(), geo, u)
            yf.backward(dy)
    params = list(tr.parameters()) + (list(cpb.parameters()) if mode == 0 else [])
    C.sink_checks(f'sinks ViTLayerFn+CPBFn[mode {mode} {variant}]', run, params, K, sync)


def test_sinks_bert_layer():
    from ctclip_mi355x import kernels as K
    model, _ = _bert(910)
    ids, mask = _text('right', 32, 911)
    kmask = mask.to(torch.int32).cuda().contiguous()
    xf0 = bf16r(rnd(96, 768, seed=912, mean=0.2))
    dy = rnd(96, 768, seed=913, scale=1e-2)

    def run():
        yf, _ = _bert_embed_run(model, ids.cuda())
        yf.backward(dy)
        yf, _ = _bert_layer_run(model, xf0.clone().requires_grad_(True), xf0.bfloat16(), kmask, 3, 32)
        yf.backward(dy)
    params = list(model.embeddings.parameters()) + list(model.encoder.layer[0].parameters())
    C.sink_checks('sinks BertEmbedFn+BertLayerFn', run, params, K, sync)


def test_sinks_patch_embed():
    from ctclip_mi355x import kernels as K
    vt, cfg = _small_vit(920)
    video, _ = _video('hu', cfg, 921)
    vid = video.cuda().contiguous()
    dy = rnd(2 * cfg.t_tokens * cfg.grid ** 2, 512, seed=922, scale=1e-2)

    def run():
        yf, _ = _patch_run(vt, vid)
        yf.backward(dy)
    C.sink_checks('sinks PatchEmbedFn', run, list(vt.to_patch_emb.parameters()), K, sync)
