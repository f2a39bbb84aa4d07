"""CTClipTrainer.save / load on the GPU: a run that is stopped and continued computes the bits of one
that never stopped.

Config of tests/test_gpu_guards.py (base widths, 160x160x40 volume -> 4x8x8 tokens, 2+2 ViT layers, 2
BERT layers), BERT dropout on, B = 2, four steps on four fixed int16 volumes / ragged token sets.
Every comparison of a resumed run with the uninterrupted one is ``torch.equal`` per parameter NAME
(the arena order is the trainer's own business); the one tolerance, across ``overlap_grad_sync``
modes, is derived in test_resume_across_layouts."""
import os
import types

import pytest
import torch

from oracle import ctclip_oracle as O
from oracle import weights as W

pytestmark = pytest.mark.gpu

LR, STEPS, STOP = 1e-4, 4, 2


def cfg_small():
    vit = O.ViTConfig(dim=512, codebook_size=8192, image_size=160, patch_size=20, temporal_patch_size=10,
                      spatial_depth=2, temporal_depth=2, dim_head=32, heads=8, frames=40)
    bert = O.BertConfig(vocab_size=1000, hidden=768, layers=2, heads=12, intermediate=3072, max_position=64)
    return O.ClipConfig(vit=vit, bert=bert, dim_latent=512)


def build(cfg, seed=0, dropout=0.1, sd=None):
    from ctclip_mi355x.models import build_ctclip, set_finetune_trainable
    from ctclip_mi355x.bert import BertConfig
    v, b = cfg.vit, cfg.bert
    vit = dict(dim=v.dim, codebook_size=v.codebook_size, image_size=v.image_size, patch_size=v.patch_size,
               temporal_patch_size=v.temporal_patch_size, spatial_depth=v.spatial_depth,
               temporal_depth=v.temporal_depth, dim_head=v.dim_head, heads=v.heads)
    bert = BertConfig(vocab_size=b.vocab_size, hidden_size=b.hidden, num_hidden_layers=b.layers,
                      num_attention_heads=b.heads, intermediate_size=b.intermediate,
                      max_position_embeddings=b.max_position,
                      hidden_dropout_prob=dropout, attention_probs_dropout_prob=dropout)
    m = build_ctclip(vit, bert, cfg.dim_latent)
    m.load_state_dict(W.make_state_dict(cfg, seed=seed) if sd is None else sd, strict=True)
    return set_finetune_trainable(m).cuda()


@pytest.fixture(scope='module')
def K():
    from ctclip_mi355x import kernels
    return kernels


def make_data():
    cfg = cfg_small()
    vols, texts = [], []
    for s in range(STEPS):
        vols.append(W.make_hu(2, cfg.vit, seed=1234 + s).cuda())
        ids, mask = W.make_text(2, 32, cfg.bert.vocab_size, seed=4321 + s, ragged=True)
        texts.append(types.SimpleNamespace(input_ids=ids.cuda(), attention_mask=mask.cuda()))
    assert vols[0].dtype == torch.int16 and not torch.equal(vols[0], vols[1])
    return cfg, vols, texts


@pytest.fixture(scope='module')
def data():
    return make_data()


def snapshot(tr):
    """Everything a resumed run must reproduce, per parameter name (clones: left unchanged afterwards)."""
    tr.flush()
    torch.cuda.synchronize()
    where = {id(p): (off, k) for p, (off, k, _) in zip(tr.flat.params, tr.flat.views)}
    out = {'param': {}, 'm': {}, 'v': {}}
    for n, p in tr.model.named_parameters():
        out['param'][n] = p.detach().clone()
        if id(p) in where:
            off, k = where[id(p)]
            out['m'][n] = tr.m[off:off + k].view_as(p).clone()
            out['v'][n] = tr.v[off:off + k].view_as(p).clone()
    assert len(out['m']) == len(where) > 10
    cbk = tr.model.visual_transformer.vq._codebook
    out['codebook'] = {'embed': cbk.embed.clone(), 'cluster_size': cbk.cluster_size.clone()}
    return out


def fresh_trainer(cfg, K, **kw):
    from ctclip_mi355x.trainer import CTClipTrainer
    K.reset_ln_status()
    torch.manual_seed(0)            # the dropout masks hash torch.initial_seed()
    return CTClipTrainer(build(cfg, seed=0), lr=LR, **kw)


_RUNS = {}


def uninterrupted(data, K, n=STEPS, **kw):
    """Run A: ``n`` steps, never stopped.  Computed once per setting and shared."""
    key = (n,) + tuple(sorted(kw.items()))
    if key not in _RUNS:
        cfg, vols, texts = data
        tr = fresh_trainer(cfg, K, **kw)
        losses = [tr.train_step(texts[s], vols[s]) for s in range(n)]
        snap = snapshot(tr)
        snap['losses'] = torch.stack(losses).clone()
        _RUNS[key] = snap
        del tr
    return _RUNS[key]


def stranger(cfg, **kw):
    """A new trainer over a model that shares nothing with the saved run: other weights, another seed
    (so another dropout stream, until load restores it), a text tower that has counted no call."""
    from ctclip_mi355x.trainer import CTClipTrainer
    torch.manual_seed(77)
    return CTClipTrainer(build(cfg, seed=7), lr=LR, **kw)


def assert_same(a, b, what=('param', 'm', 'v', 'codebook')):
    for grp in what:
        assert a[grp].keys() == b[grp].keys()
        for n in a[grp]:
            assert torch.equal(a[grp][n], b[grp][n]), \
                f'{grp} {n}: max |d| {(a[grp][n].double() - b[grp][n].double()).abs().max().item():.3e}'


def resume(data, K, path, save_kw, load_kw, upto=STEPS):
    """Run B: STOP steps, save (no explicit flush), then a stranger loads and runs steps STOP+1..upto."""
    cfg, vols, texts = data
    tr = fresh_trainer(cfg, K, **save_kw)
    for s in range(STOP):
        tr.train_step(texts[s], vols[s])
    tr.save(path)
    del tr
    tr2 = stranger(cfg, **load_kw)
    probe = 'text_transformer.encoder.layer.0.output.dense.weight'
    ck = torch.load(path, map_location='cpu', weights_only=True)
    assert not torch.equal(dict(tr2.model.named_parameters())[probe].detach().cpu(), ck['model'][probe])
    res = tr2.load(path)
    assert res['step'] == STOP == tr2.steps and not res['missing_keys'] and not res['unexpected_keys']
    assert res['hyper_mismatch'] == {}
    assert torch.initial_seed() == 0 and tr2.model.text_transformer.dropout_state() == STOP
    losses = [tr2.train_step(texts[s], vols[s]) for s in range(STOP, upto)]
    snap = snapshot(tr2)
    snap['losses'] = torch.stack(losses).clone()
    return snap


@pytest.fixture(scope='module')
def ck_plain(data, K, tmp_path_factory):
    """The checkpoint of the default trainer (wd 0, bucket order) after STOP steps, written once."""
    cfg, vols, texts = data
    path = str(tmp_path_factory.mktemp('ck') / 'plain.pt')
    tr = fresh_trainer(cfg, K)
    for s in range(STOP):
        tr.train_step(texts[s], vols[s])
    tr.save(path)
    return path


def test_bit_exact_resume(data, K, ck_plain):
    """4 steps against 2 steps + save | new model, new trainer, load + 2 steps: the losses of steps 3
    and 4, every parameter, m and v per parameter and the VQ codebook buffers, bit for bit."""
    cfg, vols, texts = data
    a = uninterrupted(data, K)
    tr2 = stranger(cfg)
    res = tr2.load(ck_plain)
    assert res['step'] == STOP and res['hyper_mismatch'] == {}
    assert torch.initial_seed() == 0 and tr2.model.text_transformer.dropout_state() == STOP
    losses = torch.stack([tr2.train_step(texts[s], vols[s]) for s in range(STOP, STEPS)])
    b = snapshot(tr2)
    assert tr2.steps == STEPS
    assert torch.equal(losses, a['losses'][STOP:]), (losses, a['losses'])
    assert_same(a, b)
    # the stop really was in the middle of something: the steps moved the state it restored
    ck = torch.load(ck_plain, map_location='cpu', weights_only=True)
    n = 'text_transformer.encoder.layer.0.output.dense.weight'
    assert not torch.equal(ck['model'][n], a['param'][n].cpu()) and ck['optim']['exp_avg'][n].abs().max() > 0


@pytest.mark.parametrize('kw', [dict(wd=0.1), dict(defer_text_adam=True)], ids=['wd', 'defer_text_adam'])
def test_bit_exact_resume_variants(data, K, tmp_path, kw):
    """wd = 0.1: the partitioned arena order and two Adam launches per bucket.  defer_text_adam: save()
    straight after train_step, the text tower's Adam of that step not yet queued."""
    from ctclip_mi355x import streams
    cfg, vols, texts = data
    path = str(tmp_path / 'ck.pt')
    a = uninterrupted(data, K, **kw)
    if kw.get('defer_text_adam'):
        # save() with the Adam pending writes what flush() followed by a read gives
        tr = fresh_trainer(cfg, K, **kw)
        for s in range(STOP):
            tr.train_step(texts[s], vols[s])
        assert streams.pending_text(tr.device)
        tr.save(path)
        assert not streams.pending_text(tr.device)
        tr.flush()
        torch.cuda.synchronize()
        ck = torch.load(path, map_location='cpu', weights_only=True)
        n_text = 0
        for k, v in tr.model.state_dict().items():
            if k.startswith('text_transformer.'):
                n_text += 1
                assert torch.equal(v.cpu(), ck['model'][k]), k
        assert n_text > 10
        del tr
    b = resume(data, K, path, kw, kw)
    assert torch.equal(b['losses'], a['losses'][STOP:]), (b['losses'], a['losses'])
    assert_same(a, b)


def _rel_l2(a, b):
    """||a - b|| / ||b|| over all trainable parameters together, in float64."""
    num = sum((a['param'][n].double() - b['param'][n].double()).pow(2).sum().item() for n in b['m'])
    den = sum(b['param'][n].double().pow(2).sum().item() for n in b['m'])
    return (num / den) ** 0.5


# ||p(overlap_grad_sync=False) - p(True)|| / ||p(True)|| over the trainable parameters after THREE
# uninterrupted steps of this file's run in either mode, measured without any save.
# No earlier test compares the two modes; they differ in the arena order, hence in the summation
# order of the gradient norm and the last bits of the clip coefficient.  Measured on the commit before
# save / load existed: 9.24e-13 after one step (1 of 99 parameters differs), 8.869771875e-10 after three
# (72 of 99, max |d| 2.98e-8, losses equal to the last bit); the same mode twice: 0.
MODES_REL_L2 = 8.869771875e-10


def test_resume_across_layouts(data, K, ck_plain):
    """Saved from overlap_grad_sync=True, loaded into overlap_grad_sync=False, one further step: the
    parameters agree with the uninterrupted run (three steps, True) to within twice what three
    uninterrupted steps in the other mode differ by -- one of the resumed run's three steps ran in the
    other mode, all three of the measured pair did."""
    cfg, vols, texts = data
    a = uninterrupted(data, K, n=STOP + 1)
    mode = uninterrupted(data, K, n=STOP + 1, overlap_grad_sync=False)
    tr2 = stranger(cfg, overlap_grad_sync=False)
    tr2.load(ck_plain)
    loss = tr2.train_step(texts[STOP], vols[STOP])
    b = snapshot(tr2)
    d_modes, d_res = _rel_l2(mode, a), _rel_l2(b, a)
    print(f'overlap modes, 3 uninterrupted steps: rel L2 {d_modes:.6e}; resumed across modes: {d_res:.6e}; '
          f'loss {loss.item():.9f} vs {a["losses"][STOP].item():.9f}')
    assert d_res <= 2 * MODES_REL_L2, (d_res, MODES_REL_L2)


def test_shadows_and_caches_after_load(data, K, ck_plain):
    """After load every bf16 hi / lo shadow is the cast kernel's image of the loaded f32 value and is
    reported current; with MX-fp8 on, an eval forward equals that of a freshly built model holding the
    checkpoint's weights (the epoch-keyed caches were filled from the stranger's weights before)."""
    from ctclip_mi355x import functional as Fn
    cfg, vols, texts = data
    tr2 = stranger(cfg)
    model = tr2.model
    old = Fn.set_vit_fp8(True)
    try:
        model.eval()
        with torch.no_grad():
            stale = model(texts[0], vols[0], return_loss=True).clone()     # fills the caches
        epoch = K.weights_epoch()
        tr2.load(ck_plain)
        assert K.weights_epoch() > epoch
        ck = torch.load(ck_plain, map_location='cpu', weights_only=True)
        for n, p in model.named_parameters():
            assert torch.equal(p.detach().cpu(), ck['model'][n]), n
            if not p.requires_grad:
                continue
            hi, lo = K.cast_bf16_split(p.detach().contiguous())
            sh = Fn.shadow_bf16(p)
            assert sh is not None, n
            assert torch.equal(sh, hi) and torch.equal(p._ctclip_bf16_lo, lo), n
        model.eval()
        ref = build(cfg, sd=ck['model']).eval()
        with torch.no_grad():
            got = (model(texts[0], vols[0], return_loss=True), model.visual_transformer.encode_tokens(vols[0])[0])
            want = (ref(texts[0], vols[0], return_loss=True), ref.visual_transformer.encode_tokens(vols[0])[0])
        torch.cuda.synchronize()
        assert torch.equal(got[0], want[0]), (got[0].item(), want[0].item())
        assert torch.equal(got[1], want[1])
        assert not torch.equal(got[0], stale)
    finally:
        Fn.set_vit_fp8(old)


def test_save_raises_for_flagged_step_and_keeps_file(data, K, tmp_path):
    """A step on a volume with a NaN voxel trips the non-finite guard (tests/test_gpu_guards.py): the
    save after it raises from its flush() and the checkpoint already at ``path`` stays as it was.  Only
    the status word is read; nothing faults."""
    from ctclip_mi355x.trainer import NonFiniteStepError
    cfg, vols, texts = data
    path = tmp_path / 'ck.pt'
    video = O.normalize_hu(vols[0].cpu()).cuda()
    bad = video.clone()
    bad[1, 0, 17, 33, 71] = float('nan')
    tr = fresh_trainer(cfg, K)
    try:
        tr.train_step(texts[0], video)
        tr.save(str(path))
        before = path.read_bytes()
        tr.train_step(texts[1], bad)
        with pytest.raises(NonFiniteStepError):
            tr.save(str(path))
        torch.cuda.synchronize()
        assert path.read_bytes() == before
        assert sorted(os.listdir(tmp_path)) == ['ck.pt']
    finally:
        K.reset_ln_status()
    ck = torch.load(str(path), map_location='cpu', weights_only=True)
    assert ck['optim']['step'] == 1
