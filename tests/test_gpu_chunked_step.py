"""The chunked train step (CTClipTrainer.train_step_chunked) on the GPU: the loss and the
gradient of ONE batch of Bg pairs, computed with `chunk` pairs' activations alive at a time.

Tolerances against the CPU oracle are the ones tests/test_gpu_model.py applies to the one-shot step:
loss |d| < 1e-3 (test_backward_grads), gradients 5e-2 relative on that test's parameter list, the
codebook after the EMA 5e-3 relative.  That file has no tolerance for parameters AFTER an optimizer
step against the oracle (the oracle has no optimizer), so the parameters are compared with an f64
restatement of clip + Adam applied to the step's own measured arena gradient: step 1 of Adam moves
every element by lr * g c / (|g c| + eps), |.| <= lr, computed in f32 -- allowed 1e-5 lr plus one f32
ulp of the parameter."""
import types

import pytest
import torch

from oracle import ctclip_oracle as O
from oracle import weights as W

pytestmark = pytest.mark.gpu

LR = 1e-3
LOSS_TOL = 1e-3          # tests/test_gpu_model.py::test_backward_grads
GRAD_TOL = 5e-2          # ... its `checks` table, every entry
EMBED_TOL = 5e-3         # ... the codebook after the EMA
GRAD_NAMES = [
    'visual_transformer.to_patch_emb.2.weight',
    'visual_transformer.to_patch_emb.1.weight',
    'visual_transformer.to_patch_emb.3.weight',
    'visual_transformer.spatial_rel_pos_bias.net.0.0.weight',
    'visual_transformer.spatial_rel_pos_bias.net.2.weight',
    'visual_transformer.enc_spatial_transformer.layers.0.0.dsconv.weight',
    'visual_transformer.enc_spatial_transformer.layers.0.1.to_q.weight',
    'visual_transformer.enc_spatial_transformer.layers.0.1.to_kv.weight',
    'visual_transformer.enc_spatial_transformer.layers.0.1.q_scale',
    'visual_transformer.enc_spatial_transformer.layers.1.3.1.weight',
    'visual_transformer.enc_spatial_transformer.layers.1.3.4.weight',
    'visual_transformer.enc_temporal_transformer.layers.0.0.dsconv.weight',
    'visual_transformer.enc_temporal_transformer.layers.1.1.to_out.weight',
    'visual_transformer.enc_temporal_transformer.norm_out.gamma',
    'text_transformer.embeddings.word_embeddings.weight',
    'text_transformer.encoder.layer.0.attention.self.query.weight',
    'text_transformer.encoder.layer.1.output.dense.weight',
    'text_transformer.encoder.layer.1.output.LayerNorm.bias',
]


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


@pytest.fixture(scope='module')
def K():
    from ctclip_mi355x import kernels
    return kernels


def batch(cfg, n, seed=0):
    hu = W.make_hu(n, cfg.vit, seed=1234 + seed)
    ids, mask = W.make_text(n, 32, cfg.bert.vocab_size, seed=4321 + seed, ragged=True)
    return hu, ids, mask, types.SimpleNamespace(input_ids=ids.cuda(), attention_mask=mask.cuda())


def trainer(cfg, K, dropout=0.0, lr=LR, **kw):
    from test_gpu_model import build
    from ctclip_mi355x.trainer import CTClipTrainer
    K.reset_ln_status()
    torch.manual_seed(0)
    tr = CTClipTrainer(build(cfg, dropout=dropout), lr=lr, **kw)
    tr.keep_chunk_latents = True
    return tr


def spy_grad(tr):
    """The arena gradient as optimizer_step finds it (both towers' streams joined), cloned."""
    from ctclip_mi355x import streams
    got = {}
    inner = tr.optimizer_step

    def step():
        streams.join_text(tr.device)
        streams.join_aux(tr.device)
        got['grad'] = tr.flat.grad[:tr.flat.numel].clone()
        inner()
    tr.optimizer_step = step
    return got


def ema_f64(embed, cluster, xn, idx, decay=0.8):
    """vector_quantize_pytorch's cosine-codebook EMA (oracle.vq_forward) on given indices, in f64."""
    C, D = embed.shape[-2:]
    e, cs, x = embed.double().reshape(C, D).cpu(), cluster.double().reshape(C).cpu(), xn.double().cpu()
    idx = idx.long().cpu().reshape(-1)
    bins = torch.bincount(idx, minlength=C).double()
    esum = torch.zeros(C, D, dtype=torch.float64).index_add_(0, idx, x)
    en = torch.nn.functional.normalize(esum / bins.clamp_min(1)[:, None], dim=-1)
    new = torch.where(bins[:, None] > 0, e * decay + en * (1 - decay), e)
    return new, cs * decay + bins * (1 - decay)


@pytest.fixture(scope='module')
def runs(K):
    """Bg = 4 on cfg_small, dropout 0, from the same initial state: chunk 2, chunk 3 (ragged tail) and
    the one-shot train_step; the oracle once, on the concatenated batch, forced onto the chunk-2
    run's VQ indices.  Left unchanged by the tests."""
    from test_gpu_model import cfg_small
    cfg = cfg_small()
    hu, ids, mask, text = batch(cfg, 4)
    out = {'cfg': cfg}
    for name, chunk in (('c2', 2), ('c3', 3), ('one', None)):
        tr = trainer(cfg, K)
        vt = tr.model.visual_transformer
        cbk = vt.vq._codebook
        r = {'p0': tr.flat.data.clone(), 'temp': tr.model.temperature.detach().reshape(1).clone(), 'embed0': cbk.embed.clone(), 'cluster0': cbk.cluster_size.clone()}
        if name == 'c2':
            tr.model.train()
            with torch.no_grad():
                zf, _, _ = vt.encode_tokens(hu.cuda())
            out['xn'] = torch.nn.functional.normalize(zf.double(), dim=-1).cpu()
        got = spy_grad(tr)
        if chunk is None:
            r['loss'] = tr.train_step(text, hu.cuda()).reshape(1).clone()
            r['indices'] = vt.vq.state.last_indices.clone().cpu()
        else:
            r['loss'] = tr.train_step_chunked(text, hu.cuda(), chunk).reshape(1).clone()
            r['indices'] = torch.cat(tr.last_chunked['indices']).cpu()
            r['caches'] = (tr.last_chunked['text_cache'].clone(), tr.last_chunked['image_cache'].clone())
        tr.flush()
        torch.cuda.synchronize()
        r.update(grad=got['grad'], p1=tr.flat.data.clone(), norm=tr.norm.clone(), embed1=cbk.embed.clone(),
                 cluster1=cbk.cluster_size.clone(), steps=tr.steps,
                 views={n: where for n, where in _named_views(tr)}, buckets=list(tr.grad_sync.buckets),
                 hyper=(tr.lr, tr.betas, tr.eps, tr.max_grad_norm))
        out[name] = r
        del tr
    with torch.no_grad():      # the oracle's own VQ choice: how many indices the one-shot path flips against it
        free = O.ctclip_forward(W.make_state_dict(cfg), ids, mask, O.normalize_hu(hu), cfg, training=False)
    out['oracle_indices'] = free['indices'].reshape(-1).long()
    sd = W.make_state_dict(cfg)
    for k, v in sd.items():
        if k.startswith(('visual_transformer.', 'text_transformer.')) and v.is_floating_point() and \
                'vq._codebook' not in k and not k.endswith('beta') and v.numel():
            v.requires_grad_(True)
    ref = O.ctclip_forward(sd, ids, mask, O.normalize_hu(hu), cfg, training=True, force_ind=out['c2']['indices'])
    ref['loss'].backward()
    out['oracle'] = {'loss': ref['loss'].item(), 'new_embed': ref['new_embed'].detach(),
                     'grad': {n: sd[n].grad for n in GRAD_NAMES}}
    return out


def _named_views(tr):
    where = {id(p): (off, k) for p, (off, k, _) in zip(tr.flat.params, tr.flat.views)}
    return [(n, where[id(p)]) for n, p in tr.model.named_parameters() if id(p) in where]


@pytest.mark.parametrize('name', ['c2', 'c3'])
def test_gradient_of_the_global_batch(runs, name):
    """Loss, arena gradient before the optimizer step and parameters after it, chunk 2 and chunk 3
    (ragged tail) at Bg = 4, against the oracle on the concatenated 4-pair batch with the tolerances of
    the one-shot step (module docstring).  Printed, not asserted: the relative difference of the
    chunked and one-shot gradients per bucket (DESIGN.md §21 records them)."""
    r, one, orc = runs[name], runs['one'], runs['oracle']
    flips = (r['indices'] != runs['c2']['indices']).sum().item()
    print(f'{name}: loss {r["loss"].item():.6f} oracle {orc["loss"]:.6f} one-shot {one["loss"].item():.6f}; '
          f'{flips} VQ indices differ from the run the oracle was forced onto')
    assert r['steps'] == 1
    assert abs(r['loss'].item() - orc['loss']) < LOSS_TOL
    bad = []
    for n in GRAD_NAMES:
        off, k = r['views'][n]
        e = rel(r['grad'][off:off + k], orc['grad'][n].reshape(-1))
        o1, k1 = one['views'][n]
        print(f'{n}: grad rel err vs oracle {e:.2e} (one-shot {rel(one["grad"][o1:o1 + k1], orc["grad"][n].reshape(-1)):.2e})')
        if not e < GRAD_TOL:
            bad.append((n, e))
    assert not bad, bad
    for tag, off, n in r['buckets']:
        print(f'bucket {tag}: chunked vs one-shot gradient rel diff {rel(r["grad"][off:off + n], one["grad"][off:off + n]):.3e}')
    assert rel(r['embed1'], orc['new_embed']) < EMBED_TOL
    # one clip, one Adam on the accumulated gradient: f64 restatement from the measured gradient
    lr, (b1, b2), eps, mx = r['hyper']
    g = r['grad'].double()
    norm = g.norm().item()
    coef = min(1.0, mx / (norm + 1e-6))
    assert abs(r['norm'][0].item() - norm) <= 1e-5 * norm and abs(r['norm'][1].item() - coef) <= 1e-5 * coef
    gc = g * coef
    want = r['p0'].double() - lr * gc / (gc.abs() + eps)
    err = (r['p1'].double() - want).abs()
    allow = 1e-5 * lr + want.abs() * 2.0 ** -23
    print(f'{name}: parameters vs f64 clip + Adam of the measured gradient: max |d| {err.max().item():.3e}, '
          f'moved {(r["p1"] != r["p0"]).float().mean().item():.3f} of them; vs one-shot parameters rel '
          f'{rel(r["p1"] - r["p0"], one["p1"] - one["p0"]):.3e}')
    assert (err <= allow).all(), (err - allow).max().item()
    assert (r['p1'] != r['p0']).float().mean().item() > 0.5


def test_negatives_are_global(runs, K):
    """Bg = 4 / chunk 2 at the name-seeded initial weights: the returned loss is the loss kernel's on
    the trainer's own caches, bit for bit; within the oracle tolerance of the oracle's 4-pair loss; and
    NOT the mean of the two 2-pair losses (about ln 4 against about ln 2 at initialisation)."""
    from ctclip_mi355x import functional as Fn
    r = runs['c2']
    tc, ic = r['caches']
    lt = r['temp']
    assert not Fn.loss_uses_tiled(4)
    again = K.clip_loss(tc[0], ic[0], lt)[0]
    assert torch.equal(again.reshape(1), r['loss'])
    assert abs(r['loss'].item() - runs['oracle']['loss']) < LOSS_TOL
    halves = [K.clip_loss(tc[0, s:s + 2].contiguous(), ic[0, s:s + 2].contiguous(), lt)[0].item() for s in (0, 2)]
    mean2 = sum(halves) / 2
    print(f'global loss {r["loss"].item():.6f}, mean of the 2-pair losses {mean2:.6f}')
    assert abs(r['loss'].item() - mean2) > LOSS_TOL


def test_dropout_masks_replay(K):
    """BERT dropout 0.1: pass 2's raw text latents equal the cached pass-1 rows bit for bit for every
    chunk (same shapes, kernels and seeds: the call state is rewound per chunk), and the call state
    after the step is that of as many direct forward calls as there were chunks."""
    from test_gpu_model import cfg_small
    cfg = cfg_small()
    hu, ids, mask, text = batch(cfg, 4)
    tr = trainer(cfg, K, dropout=0.1)
    tt = tr.model.text_transformer
    s0 = tt.dropout_state()
    tr.train_step_chunked(text, hu.cuda(), 3)
    tr.flush()
    torch.cuda.synchronize()
    lc = tr.last_chunked
    assert lc['dropout_states'] == [s0, s0 + 1]
    t2, i2 = torch.cat(lc['pass2_text']), torch.cat(lc['pass2_image'])
    print('image latents pass 2 vs cache: max |d|', (i2 - lc['image_cache'][0]).abs().max().item())
    assert torch.equal(t2, lc['text_cache'][0])
    assert tt.dropout_state() == s0 + 2
    # dropout is really on: the same rows without it differ
    tr0 = trainer(cfg, K, dropout=0.0)
    tc0, _, _ = tr0._chunked_pass1(text, hu.cuda(), 3)
    torch.cuda.synchronize()
    assert not torch.equal(tc0[0], lc['text_cache'][0])
    # ... and direct forward calls count the same way
    n0 = tr0.model.text_transformer.dropout_state()
    with torch.no_grad():
        for s in (0, 3):
            tr0.model.text_transformer(text.input_ids[s:s + 3], attention_mask=text.attention_mask[s:s + 3])
    assert tr0.model.text_transformer.dropout_state() - n0 == tt.dropout_state() - s0


def test_codebook_ema_once_from_the_old_codebook(runs, K):
    """Pass 1 alone leaves the codebook and cluster sizes bit-identical.  After the whole step:
    cluster sizes equal the one-shot step's exactly when the VQ indices agree (integer counts through
    the same f32 expression), else the flipped share stays within the share the one-shot path flips
    against the oracle; the codebook of both runs against an f64 restatement of the EMA on the run's own
    indices, the chunked deviation at most 4x the one-shot one."""
    cfg = runs['cfg']
    hu, ids, mask, text = batch(cfg, 4)
    tr = trainer(cfg, K)
    cbk = tr.model.visual_transformer.vq._codebook
    e0, c0 = cbk.embed.clone(), cbk.cluster_size.clone()
    tr._chunked_pass1(text, hu.cuda(), 2)
    tr.flush()
    torch.cuda.synchronize()
    assert torch.equal(e0, cbk.embed) and torch.equal(c0, cbk.cluster_size)
    dev = {}
    for name in ('c2', 'c3', 'one'):
        r = runs[name]
        assert not torch.equal(r['embed1'], r['embed0'])
        want_e, want_c = ema_f64(r['embed0'], r['cluster0'], runs['xn'], r['indices'])
        dev[name] = rel(r['embed1'].reshape(want_e.shape), want_e)
        assert rel(r['cluster1'].reshape(-1), want_c) < 1e-6
    print('codebook vs f64 EMA of the own indices:', {k: f'{v:.3e}' for k, v in dev.items()})
    for name in ('c2', 'c3'):
        r, one = runs[name], runs['one']
        flips = (r['indices'] != one['indices']).sum().item()
        print(f'{name}: {flips} of {one["indices"].numel()} VQ indices differ from the one-shot step')
        if flips == 0:
            assert torch.equal(r['cluster1'], one['cluster1'])
            assert torch.equal(r['embed1'], one['embed1'])      # fixed-point sums: order-free
        else:
            # within what the one-shot path itself flips against the oracle's free choice
            # (test_gpu_model.py::test_forward_latents_and_loss counts the same thing)
            own = (one['indices'].long() != runs['oracle_indices']).sum().item()
            print(f'one-shot vs oracle: {own} indices differ')
            assert flips <= own
        assert dev[name] <= 4 * dev['one'] + 1e-12


def test_nan_in_a_middle_chunk_skips_the_whole_step(K):
    """test_gpu_guards.py::test_nonfinite_step_is_skipped_and_raises for the chunked step: a NaN voxel
    in the second chunk of three.  Nobody applies the step: parameters, moments, codebook and cluster
    sizes bit-identical, gradients cleared, NonFiniteStepError from check(); after reset_ln_status() a
    clean chunked step trains."""
    from test_gpu_model import cfg_small
    from ctclip_mi355x.trainer import NonFiniteStepError
    cfg = cfg_small()
    hu, ids, mask, text = batch(cfg, 6)
    video = O.normalize_hu(hu).cuda()
    bad = video.clone()
    bad[3, 0, 17, 33, 71] = float('nan')
    tr = trainer(cfg, K)
    tr.train_step_chunked(text, video, 2)           # one good step first (moments non-zero)
    tr.check()
    cbk = tr.model.visual_transformer.vq._codebook
    tr.flush()
    snap = (tr.flat.data.clone(), tr.m.clone(), tr.v.clone(), cbk.embed.clone(), cbk.cluster_size.clone())
    tr.train_step_chunked(text, bad, 2)
    with pytest.raises(NonFiniteStepError) as ei:
        tr.check()
    tr.flush()                                      # (the held codebook update is queued, guarded, by now)
    torch.cuda.synchronize()
    print('flagged chunked step:', ei.value.bits)
    assert ei.value.bits & 4
    for a, b, n in zip(snap, (tr.flat.data, tr.m, tr.v, cbk.embed, cbk.cluster_size),
                       ('params', 'adam m', 'adam v', 'codebook', 'cluster size')):
        assert torch.equal(a, b), n
    assert tr.flat.grad[:tr.flat.numel].abs().max().item() == 0.0
    K.reset_ln_status()
    loss = tr.train_step_chunked(text, video, 2)
    tr.check()
    tr.flush()
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and not torch.equal(snap[0], tr.flat.data)
    assert not torch.equal(snap[3], cbk.embed)


def test_chunked_step_saves_memory(K):
    """Bg = 8 on cfg_small: the peak allocation above the resting level of train_step_chunked(chunk=2)
    is strictly below the one-shot train_step's (both warmed up, peak statistics reset between)."""
    from test_gpu_model import cfg_small
    cfg = cfg_small()
    hu, ids, mask, text = batch(cfg, 8)
    v = hu.cuda()
    tr = trainer(cfg, K, lr=1e-5)
    tr.keep_chunk_latents = False
    delta = {}
    for name, step in (('chunked', lambda: tr.train_step_chunked(text, v, 2)), ('one-shot', lambda: tr.train_step(text, v))):
        step()
        tr.flush()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        step()
        tr.flush()
        torch.cuda.synchronize()
        delta[name] = torch.cuda.max_memory_allocated() - base
    print({k: f'{v / 2 ** 20:.1f} MiB' for k, v in delta.items()})
    assert delta['chunked'] < delta['one-shot']


def test_beyond_128_rows_on_one_device(K):
    """Bg = 132 / chunk 12 on the 80-pixel 1 + 1-layer model, loss dispatch 'auto' (the tiled kernels
    above 128 rows): finite loss, bit-equal to clip_loss_tiled on the caches, the weights move, and a
    second run from the same state leaves bit-identical parameters."""
    from test_model_layout import _small_cfg, _product
    from ctclip_mi355x import functional as Fn
    from ctclip_mi355x.models import set_finetune_trainable
    from ctclip_mi355x.trainer import CTClipTrainer
    cfg = _small_cfg()
    Bg = 132
    hu = W.make_hu(Bg, cfg.vit).cuda()
    ids, mask = W.make_text(Bg, 32, cfg.bert.vocab_size, ragged=True)
    text = types.SimpleNamespace(input_ids=ids.cuda(), attention_mask=mask.cuda())
    old = Fn.set_loss_tiled('auto')
    outs = []
    try:
        assert Fn.loss_uses_tiled(Bg)
        for _ in range(2):
            K.reset_ln_status()
            torch.manual_seed(0)
            model = _product(cfg)
            # (BERT dropout off: the dropout-fused LayerNorm backward takes hidden sizes above 512 only,
            # this model's text tower is 256 wide; the replay with dropout is test_dropout_masks_replay's)
            model.text_transformer.config.hidden_dropout_prob = 0.0
            model.text_transformer.config.attention_probs_dropout_prob = 0.0
            model.load_state_dict(W.make_state_dict(cfg), strict=True)
            tr = CTClipTrainer(set_finetune_trainable(model).cuda(), lr=LR)
            p0 = tr.flat.data.clone()
            loss = tr.train_step_chunked(text, hu, 12)
            tr.flush()
            torch.cuda.synchronize()
            lc = tr.last_chunked
            again = K.clip_loss_tiled(lc['text_cache'], lc['image_cache'], model.temperature.detach().reshape(1))[0]
            assert torch.isfinite(loss).all() and torch.equal(again.reshape(1), loss.reshape(1))
            assert not torch.equal(p0, tr.flat.data)
            cbk = model.visual_transformer.vq._codebook
            outs.append((loss.clone(), tr.flat.data.clone(), tr.m.clone(), tr.v.clone(), cbk.embed.clone(),
                         cbk.cluster_size.clone()))
            del tr, model
    finally:
        Fn.set_loss_tiled(old)
    print('Bg = 132 loss', outs[0][0].item())
    for a, b, n in zip(outs[0], outs[1], ('loss', 'params', 'adam m', 'adam v', 'codebook', 'cluster size')):
        assert torch.equal(a, b), n


def test_resume_after_chunked_step(K, tmp_path):
    """Two chunked steps (dropout 0.1) against one chunked step, save, a fresh trainer, load, one
    chunked step: parameters, moments and codebook bit-equal (DESIGN.md §18's promise for train_step)."""
    from test_gpu_model import cfg_small
    cfg = cfg_small()
    data = [batch(cfg, 4, seed=s) for s in range(2)]

    def state(tr):
        tr.flush()
        torch.cuda.synchronize()
        cbk = tr.model.visual_transformer.vq._codebook
        views = dict(_named_views(tr))
        return {n: (tr.flat.data[o:o + k].clone(), tr.m[o:o + k].clone(), tr.v[o:o + k].clone())
                for n, (o, k) in views.items()}, cbk.embed.clone(), cbk.cluster_size.clone()
    a = trainer(cfg, K, dropout=0.1, lr=1e-4)
    la = [a.train_step_chunked(d[3], d[0].cuda(), 2) for d in data]
    sa = state(a)
    b = trainer(cfg, K, dropout=0.1, lr=1e-4)
    b.train_step_chunked(data[0][3], data[0][0].cuda(), 2)
    path = str(tmp_path / 'chunked.pt')
    b.save(path)
    del b
    torch.manual_seed(77)
    c = trainer(cfg, K, dropout=0.1, lr=1e-4)
    torch.manual_seed(77)
    res = c.load(path)
    assert res['step'] == 1 and c.model.text_transformer.dropout_state() == 2
    lc = c.train_step_chunked(data[1][3], data[1][0].cuda(), 2)
    sc = state(c)
    assert c.steps == 2 and torch.equal(lc, la[1])
    for n in sa[0]:
        for x, y, what in zip(sa[0][n], sc[0][n], ('param', 'm', 'v')):
            assert torch.equal(x, y), (n, what)
    assert torch.equal(sa[1], sc[1]) and torch.equal(sa[2], sc[2])


def test_deferred_text_adam_chunked_matches(K):
    """CTClipTrainer(defer_text_adam=True): the previous step's text Adam is queued by pass 1's first
    text forward.  Two chunked steps (dropout 0.1) then flush: losses and parameters bit-identical to
    the immediate placement, as test_gpu_model.py::test_deferred_text_adam_matches for train_step."""
    from test_gpu_model import cfg_small
    cfg = cfg_small()
    hu, ids, mask, text = batch(cfg, 4)
    outs = []
    for defer in (False, True):
        tr = trainer(cfg, K, dropout=0.1, lr=1e-4, defer_text_adam=defer)
        losses = [tr.train_step_chunked(text, hu.cuda(), 2) for _ in range(2)]
        tr.flush()
        torch.cuda.synchronize()
        cbk = tr.model.visual_transformer.vq._codebook
        outs.append((torch.stack(losses), tr.flat.data.clone(), tr.m.clone(), cbk.embed.clone()))
        del tr
    for a, b, n in zip(outs[0], outs[1], ('losses', 'params', 'adam m', 'codebook')):
        assert torch.equal(a, b), n


def test_refusals_and_one_chunk(K):
    """aug_image, extra_latent_projection=True: NotImplementedError; chunk 0, differing row counts:
    ValueError; nothing was stepped.  chunk >= Bg is one chunk: the same loss bit for bit as chunk = Bg."""
    from test_gpu_model import cfg_small
    cfg = cfg_small()
    hu, ids, mask, text = batch(cfg, 2)
    v = hu.cuda()
    tr = trainer(cfg, K)
    with pytest.raises(NotImplementedError):
        tr.train_step_chunked(text, v, 1, aug_image=v)
    tr.model.extra_latent_projection = True
    try:
        with pytest.raises(NotImplementedError):
            tr.train_step_chunked(text, v, 1)
    finally:
        tr.model.extra_latent_projection = False
    with pytest.raises(ValueError):
        tr.train_step_chunked(text, v, 0)
    with pytest.raises(ValueError):
        tr.train_step_chunked(text, v[:1], 1)
    assert tr.steps == 0 and tr.flat.grad.abs().max().item() == 0.0
    la = tr.train_step_chunked(text, v, 2)
    tr2 = trainer(cfg, K)
    lb = tr2.train_step_chunked(text, v, 5)
    tr.flush(), tr2.flush()
    torch.cuda.synchronize()
    assert torch.equal(la, lb) and torch.equal(tr.flat.data, tr2.flat.data)
