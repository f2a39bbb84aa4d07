"""Zero-shot attribution maps on the GPU: ctclip_attr_weights / ctclip_attr_map against the float64
restatement of tests/test_attribution_cpu.py, ZeroShotAttribution on the tiny model, its cache, and
CTClipTrainer.attribute's status guard.

Bounds: 1e-5 normwise for f32-accumulated products against float64 (the project's bound for f32 GEMM
results, tests/test_gpu_gemm.py); bit equality where every product and partial sum is
exact in f32; completeness against ``predict`` at 4x the gap measured here in float64 between the
log-odds with ``pooled`` rounded to bf16 (what the projection multiplies) and unrounded (what the map
sums) -- DESIGN.md §24."""
import types

import pytest
import torch

from oracle import ctclip_oracle as O
from oracle import weights as W
from test_attribution_cpu import (attribution_reference, direction_rows, map_reference, pooled_reference,
                                  scale_reference)

pytestmark = pytest.mark.gpu

F64 = torch.float64


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ------------------------------------------------------------------------------------ attr_weights
# K = HW * D ends inside a wave's 128-column chunk at 64 and 320, inside a workgroup's 512 columns past
# the first workgroup at 576; 1536 and 32768 end on a workgroup boundary
@pytest.mark.parametrize('R,Dl,HW,D', [(1, 64, 1, 64), (3, 64, 5, 64), (36, 512, 64, 512), (7, 512, 3, 512),
                                       (17, 64, 9, 64)])
def test_attr_weights_matches_f64(R, Dl, HW, D):
    from ctclip_mi355x import kernels as K
    g = torch.Generator().manual_seed(R * 1000 + HW)
    Wb = (torch.randn(Dl, HW * D, generator=g) / Dl ** 0.5).bfloat16()
    dirs = torch.randn(R, Dl, generator=g)
    V = K.attr_weights(dirs.cuda(), Wb.cuda(), HW, D)
    assert V.shape == (R, HW, D) and V.dtype == torch.float32
    ref = (dirs.double() @ Wb.double()).reshape(R, HW, D)
    err = rel(V, ref)
    print(f'attr_weights R={R} Dl={Dl} K={HW * D}: normwise rel err {err:.3e}')
    assert err <= 1e-5
    assert same_bits(V, K.attr_weights(dirs.cuda(), Wb.cuda(), HW, D))


def test_attr_weights_refuses_too_many_rows():
    from ctclip_mi355x import kernels as K
    from ctclip_mi355x._lib import KernelError
    assert K.ATTR_MAX_ROWS >= 36
    dirs = torch.zeros(K.ATTR_MAX_ROWS + 1, 64, device='cuda')
    Wb = torch.zeros(64, 64, device='cuda', dtype=torch.bfloat16)
    with pytest.raises(KernelError, match='1003'):            # CT_ESHAPE
        K.attr_weights(dirs, Wb, 1, 64)
    assert K.attr_weights(dirs[:K.ATTR_MAX_ROWS], Wb, 1, 64).shape == (K.ATTR_MAX_ROWS, 1, 64)


# ---------------------------------------------------------------------------------------- attr_map
MAP_SHAPES = [(1, 1, 1, 1, 64, 16), (3, 5, 4, 5, 64, 16), (2, 36, 4, 64, 512, 8192)]


def _indices(g, N, T, HW, codes):
    """Random codes with 0 and codes - 1 among them (where there are two tokens to hold them); every
    token of the LAST volume has one code."""
    idx = torch.randint(0, codes, (N, T * HW), generator=g, dtype=torch.int32)
    idx[N - 1] = codes - 1 if N == 1 else codes // 2
    if N > 1:
        idx[0, 0], idx[0, -1] = 0, codes - 1
    return idx.reshape(-1)


@pytest.mark.parametrize('N,R,T,HW,D,codes', MAP_SHAPES)
def test_attr_map_raw_is_exact(N, R, T, HW, D, codes):
    """Small integers (|k| <= 7) times a power of two per direction row and per code: inside one dot
    product every product is an integer multiple of ONE power of two, at most 49 of them, and a partial
    sum holds at most 512 * 49 < 2^15 -- every step is exact in f32, so the kernel must give the float64
    result bit for bit, whatever its summation order."""
    from ctclip_mi355x import kernels as K
    g = torch.Generator().manual_seed(N + R + HW)
    V = torch.randint(-7, 8, (R, HW, D), generator=g).float() * 2.0 ** -(torch.arange(R) % 3 + 1).float().view(R, 1, 1)
    cb = torch.randint(-7, 8, (codes, D), generator=g).float() * 2.0 ** -(torch.arange(codes) % 4).float().view(-1, 1)
    idx = _indices(g, N, T, HW, codes)
    out = K.attr_map(V.cuda(), idx.cuda(), cb.cuda(), N, T, HW)
    assert out.shape == (N, R, T, HW) and out.dtype == torch.float32
    ref = map_reference(V, cb, idx, T, HW)
    assert torch.equal(out.cpu().double(), ref)
    # one code everywhere in the last volume: its map does not depend on t
    assert torch.equal(out[N - 1], out[N - 1, :, :1].expand(R, T, HW))
    assert bool((out[N - 1] != 0).any())


@pytest.mark.parametrize('N,R,T,HW,D,codes', MAP_SHAPES[1:])
def test_attr_map_normalised(N, R, T, HW, D, codes):
    from ctclip_mi355x import kernels as K
    g = torch.Generator().manual_seed(7 * N + R)
    Dl = 96 if D == 64 else 512
    V = torch.randn(R, HW, D, generator=g)
    cb = torch.nn.functional.normalize(torch.randn(codes, D, generator=g), dim=-1)
    idx = _indices(g, N, T, HW, codes)
    i_raw = torch.randn(N, Dl, generator=g) * 3.0
    log_temp = torch.tensor([0.9])
    args = (idx.cuda(), cb.cuda(), N, T, HW, i_raw.cuda(), log_temp.cuda())
    out = K.attr_map(V.cuda(), *args)
    scale = scale_reference(log_temp, T, i_raw.double().norm(dim=-1))
    err = rel(out, map_reference(V, cb, idx, T, HW, scale))
    print(f'attr_map N={N} R={R} T={T} HW={HW} D={D}: normwise rel err {err:.3e}')
    assert err <= 1e-5
    assert same_bits(out, K.attr_map(V.cuda(), *args))
    # s_n on its own: V . C = 1 for every token (one nonzero product, exact), so out = s_n
    V1 = torch.zeros(R, HW, D)
    V1[:, :, 0] = 1.0
    cb1 = cb.clone()
    cb1[:, 0] = 1.0
    s = K.attr_map(V1.cuda(), idx.cuda(), cb1.cuda(), N, T, HW, i_raw.cuda(), log_temp.cuda()).cpu().double()
    s_err = ((s - scale.view(N, 1, 1, 1)).abs() / scale.view(N, 1, 1, 1)).max().item()
    print(f'  s_n max rel err {s_err:.3e}')
    assert s_err <= 1e-6


# ------------------------------------------------------------------------------------- model level
def _prompts(model, cfg, P, seed=99):
    from ctclip_mi355x.zero_shot import ZeroShotClassifier, PATHOLOGIES
    pids, pmask = W.make_text(2 * P, 32, cfg.bert.vocab_size, seed=seed, ragged=True)
    zs = ZeroShotClassifier(model, pathologies=PATHOLOGIES[:P])
    zs.set_prompts(types.SimpleNamespace(input_ids=pids.cuda(), attention_mask=pmask.cuda()))
    return zs


@pytest.fixture(scope='module')
def tiny():
    """tests/test_gpu_eval.py's recipe: cfg_small (T = 4, HW = 64, D = 512), P = 3, 4 volumes."""
    from test_gpu_model import build, cfg_small
    from ctclip_mi355x import kernels as K
    torch.manual_seed(0)
    cfg = cfg_small()
    model = build(cfg)
    zs = _prompts(model, cfg, 3)
    video = O.normalize_hu(W.make_hu(4, cfg.vit)).cuda()
    K.reset_ln_status()
    return cfg, model, zs, video


def _operands(model, zs, video):
    """The model's own operands for ``video`` as ONE batch, on the host: (bf16 weight as f64-exact f32,
    codebook, indices, raw prompt latents, log temperature, raw image latents)."""
    i_raw = zs.image_latents(video)
    vt = model.visual_transformer
    idx = vt.vq.state.last_indices.cpu()
    Wv = model.to_visual_latent.weight
    Wb = model._visual_weight_bf16(Wv).float().cpu()
    embed = vt._codebook_tensors()[0]
    cb = embed.view(-1, embed.shape[-1]).float().cpu()
    return Wb, cb, idx, zs._t_raw.cpu(), model.temperature.detach().cpu(), i_raw.cpu()


def _reference(model, zs, video, which='log_odds'):
    Wb, cb, idx, t_raw, log_temp, i_raw = _operands(model, zs, video)
    hg, wg = model.visual_transformer.patch_height_width
    HW, D = hg * wg, cb.shape[1]
    T = idx.numel() // (video.shape[0] * HW)
    ref = attribution_reference(Wb, cb, idx, t_raw, log_temp, T, HW, D, which, norm=i_raw.double().norm(dim=-1))
    return ref, (T, hg, wg)


def test_maps_match_reference(tiny):
    cfg, model, zs, video = tiny
    res = zs.attribute(video, batch_size=4)
    ref, (T, hg, wg) = _reference(model, zs, video)
    assert (T, hg, wg) == (4, 8, 8)
    assert res['maps'].shape == (4, 3, T, hg, wg) and res['maps'].dtype == torch.float32
    err = rel(res['maps'].reshape(4, 3, T, hg * wg), ref)
    print(f'model maps vs f64 restatement: normwise rel err {err:.3e}')
    assert err <= 1e-5
    probs, scores = zs.predict(video, batch_size=4)
    assert torch.equal(res['probs'], probs) and torch.equal(res['scores'], scores)
    # 'scores': the split of each score; rows (j, 0) / (j, 1) are the pair's normalised prompt latents
    res_s = zs.attribute(video, batch_size=4, which='scores')
    ref_s, _ = _reference(model, zs, video, which='scores')
    assert res_s['maps'].shape == (4, 3, 2, T, hg, wg)
    err_s = rel(res_s['maps'].reshape(4, 6, T, hg * wg), ref_s)
    print(f"model maps ('scores') vs f64 restatement: normwise rel err {err_s:.3e}")
    assert err_s <= 1e-5
    assert torch.equal(res_s['probs'], probs)


def test_maps_do_not_depend_on_batch_size(tiny):
    cfg, model, zs, video = tiny
    a = zs.attribute(video, batch_size=4)
    b = zs.attribute(video, batch_size=2)
    assert same_bits(a['maps'], b['maps'])
    assert torch.equal(a['probs'], b['probs']) and torch.equal(a['scores'], b['scores'])


def test_completeness_against_predict(tiny):
    """sum over the grid of maps == scores[..., 0] - scores[..., 1] of ``predict``, up to the one
    difference between the two computations: the projection multiplies ``pooled`` rounded to bf16, the
    map sums f32 codebook rows.  That gap is measured here in float64 from the model's own operands."""
    cfg, model, zs, video = tiny
    res = zs.attribute(video, batch_size=4)
    Wb, cb, idx, t_raw, log_temp, _ = _operands(model, zs, video)
    T, HW, D = 4, 64, cb.shape[1]
    pooled = pooled_reference(cb, idx, T, HW, D)
    d = direction_rows(t_raw, 'log_odds')
    tau = torch.exp(log_temp.double().reshape(()))

    def log_odds(p):
        v = p @ Wb.double().t()
        return tau * (v / v.norm(dim=-1, keepdim=True)) @ d.t()
    gap = (log_odds(pooled.float().bfloat16().double()) - log_odds(pooled)).abs().max().item()
    scores = zs.predict(video, batch_size=4)[1]
    miss = (res['maps'].double().sum(dim=(2, 3, 4)) - (scores[..., 0].double() - scores[..., 1].double())).abs().max().item()
    print(f'completeness: measured bf16-pooled gap {gap:.3e}, bound {4 * gap:.3e}, |sum maps - log-odds| {miss:.3e}')
    assert gap > 0
    assert miss <= 4 * gap
    logit = torch.logit(res['probs'].double())
    print(f'  |sum maps - logit(probs)| {(res["maps"].double().sum(dim=(2, 3, 4)) - logit).abs().max().item():.3e}')


def test_refusals(tiny):
    from ctclip_mi355x import precise
    cfg, model, zs, video = tiny
    with pytest.raises(ValueError, match='which'):
        zs.attribute(video[:1], which='gradients')
    with precise.vit_precision_scope('f32'):
        with pytest.raises(NotImplementedError):
            zs.attribute(video[:1])
    model.extra_latent_projection = True
    try:
        with pytest.raises(NotImplementedError):
            zs.attribute(video[:1], text_to_image=False)
    finally:
        model.extra_latent_projection = False


def test_to_volume_on_device(tiny):
    from ctclip_mi355x import to_volume
    cfg, model, zs, video = tiny
    maps = zs.attribute(video[:1])['maps']
    v = cfg.vit
    vol = to_volume(maps, (v.temporal_patch_size, v.patch_size, v.patch_size))
    assert vol.shape[2:] == video.shape[2:]
    assert (vol.double().sum(dim=(2, 3, 4)) - maps.double().sum(dim=(2, 3, 4))).abs().max().item() <= 1e-4


# ------------------------------------------------------------------------------ cache invalidation
def test_cache_follows_the_weights_and_the_prompts():
    """V is kept between calls and rebuilt when to_visual_latent changes (an Adam step through the
    trainer's arena: pointer and version stay, the weights epoch moves) and when the classifier's prompt
    latents are encoded again."""
    from test_gpu_model import build, cfg_small
    from ctclip_mi355x import kernels as K
    from ctclip_mi355x.trainer import CTClipTrainer
    torch.manual_seed(0)
    cfg = cfg_small()
    model = build(cfg)
    model.to_visual_latent.weight.requires_grad = True
    zs = _prompts(model, cfg, 3)
    video = O.normalize_hu(W.make_hu(2, cfg.vit)).cuda()
    ids, mask = W.make_text(2, 32, cfg.bert.vocab_size, ragged=True)
    text = types.SimpleNamespace(input_ids=ids.cuda(), attention_mask=mask.cuda())
    K.reset_ln_status()
    tr = CTClipTrainer(model, lr=1e-3)

    def current():
        return zs._attribution._cache['log_odds'][2][0]

    def check(res):
        ref, (T, hg, wg) = _reference(model, zs, video)
        err = rel(res['maps'].reshape(2, 3, T, hg * wg), ref)
        print(f'  maps vs f64 restatement: {err:.3e}')
        assert err <= 1e-5
    r0 = zs.attribute(video)
    check(r0)
    V0 = current()
    zs.attribute(video)
    assert current() is V0                                    # kept
    tr.train_step(text, video)
    tr.flush()
    r1 = zs.attribute(video)                                  # the stale prompt latents, the new weight
    V1 = current()
    assert V1 is not V0 and not torch.equal(V1, V0)
    assert not torch.equal(r1['maps'], r0['maps'])
    check(r1)
    t_old = zs._t_raw
    zs.refresh()
    assert zs._t_raw is not t_old
    r2 = zs.attribute(video)
    assert current() is not V1 and not torch.equal(current(), V1)
    assert not torch.equal(r2['maps'], r1['maps'])
    check(r2)
    model.eval()


# ------------------------------------------------------------------------- CTClipTrainer.attribute
def test_trainer_attribute_owns_its_status_bits(tiny):
    from ctclip_mi355x import kernels as K
    from ctclip_mi355x.trainer import CTClipTrainer, EvalGuardError, StepGuardError
    cfg, model, zs, video = tiny
    ids, mask = W.make_text(2, 32, cfg.bert.vocab_size, ragged=True)
    text = types.SimpleNamespace(input_ids=ids.cuda(), attention_mask=mask.cuda())
    K.reset_ln_status()
    model.train()
    tr = CTClipTrainer(model, lr=1e-3)
    tr.train_step(text, video[:2])
    tr.check()
    word = K.status_word(video.device)
    snap = word.clone()
    bad = video[:2].clone()
    bad[1, 0, 17, 33, 71] = float('nan')
    assert model.training
    with pytest.raises(EvalGuardError) as ei:
        tr.attribute(bad, classifier=zs)
    assert isinstance(ei.value, StepGuardError) and ei.value.bits != 0
    print('flagged attribution:', ei.value)
    assert torch.equal(word, snap) and model.training
    before = tr.flat.data.clone()
    loss = tr.train_step(text, video[:2])
    tr.check()                                                # not blamed for the attribution's bits
    assert torch.isfinite(loss) and not torch.equal(before, tr.flat.data)
    res = tr.attribute(video[:2])                             # the classifier passed before
    assert bool(torch.isfinite(res['maps']).all()) and bool(torch.isfinite(res['probs']).all())
    assert res['maps'].shape == (2, 3, 4, 8, 8)
    assert model.training and torch.equal(word, snap)
    ref, (T, hg, wg) = _reference(model, zs, video[:2])
    assert rel(res['maps'].reshape(2, 3, T, hg * wg), ref) <= 1e-5
    model.eval()
    tr.attribute(video[:2])
    assert not model.training
