"""CTClipTrainer.save / load on CPU arenas (no GPU; the host logic of ctclip_mi355x/checkpoint.py).

The trainer runs no step here, so the towers are the narrow ones of tests/test_model_layout.py (the
package layout, the name-keyed optimizer state, the refusals, the atomic write and the rank protocol do
not depend on the widths); tests/test_gpu_checkpoint.py resumes real steps at the parity config."""
import os
import socket
import warnings

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

WORLD = 2


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _model(seed):
    from ctclip_mi355x.models import build_ctclip, set_finetune_trainable
    from ctclip_mi355x.bert import BertConfig
    torch.manual_seed(seed)
    vit = dict(dim=512, codebook_size=512, image_size=80, patch_size=20, temporal_patch_size=10, spatial_depth=1,
               temporal_depth=1, dim_head=32, heads=8)
    bert = BertConfig(vocab_size=500, hidden_size=256, num_hidden_layers=1, num_attention_heads=4,
                      intermediate_size=512, max_position_embeddings=64)
    return set_finetune_trainable(build_ctclip(vit, bert, 64))


def _fill(tr, seed, steps=7, drop_calls=5):
    """Distinct values everywhere a checkpoint looks: weights, both moments, codebook, counters."""
    g = torch.Generator().manual_seed(seed)
    tr.flat.data.copy_(torch.randn(tr.flat.numel, generator=g))
    tr.m.copy_(torch.randn(tr.flat.numel, generator=g))
    tr.v.copy_(torch.rand(tr.flat.numel, generator=g))
    cbk = tr.model.visual_transformer.vq._codebook
    cbk.embed.copy_(torch.randn(cbk.embed.shape, generator=g))
    cbk.cluster_size.copy_(torch.rand(cbk.cluster_size.shape, generator=g))
    tr.steps = steps
    tr.model.text_transformer.set_dropout_state(drop_calls)


def _moments(tr):
    """{name: (m slice, v slice)} read straight from the arenas through FlatParams.views."""
    where = {id(p): (off, k) for p, (off, k, _) in zip(tr.flat.params, tr.flat.views)}
    out = {}
    for n, p in tr.model.named_parameters():
        if id(p) in where:
            off, k = where[id(p)]
            out[n] = (tr.m[off:off + k].view_as(p), tr.v[off:off + k].view_as(p))
    assert len(out) == len(where)
    return out


def _same_state(a, b):
    sa, sb = a.model.state_dict(), b.model.state_dict()
    assert sa.keys() == sb.keys()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    ma, mb = _moments(a), _moments(b)
    assert ma.keys() == mb.keys() and len(ma) > 10
    for n in ma:
        assert torch.equal(ma[n][0], mb[n][0]), n
        assert torch.equal(ma[n][1], mb[n][1]), n
    assert a.steps == b.steps


@pytest.fixture(scope='module')
def source(tmp_path_factory):
    """One filled trainer (wd = 0, bucket order) and its checkpoint, shared and left unchanged."""
    from ctclip_mi355x.trainer import CTClipTrainer
    tr = CTClipTrainer(_model(0), wd=0.0, overlap_grad_sync=True)
    _fill(tr, 1)
    path = str(tmp_path_factory.mktemp('ck') / 'ck.pt')
    torch.manual_seed(1234)
    torch.rand(3)                      # the generator is past its seed: the state, not the seed, is saved
    tr.save(path)
    after = torch.rand(4)              # what the saved generator state draws next
    return tr, path, after


def test_layout_independence(source):
    """wd = 0 / bucket order -> wd = 0.1 / one bucket, decayed parameters first: another arena order on
    each side, the same state per NAME afterwards."""
    from ctclip_mi355x.trainer import CTClipTrainer
    src, path, after = source
    dst = CTClipTrainer(_model(3), wd=0.1, overlap_grad_sync=False)
    order = lambda t: [id(p) for p in t.flat.params]      # noqa: E731
    names = {id(p): n for n, p in src.model.named_parameters()}
    names.update({id(p): n for n, p in dst.model.named_parameters()})
    assert [names[i] for i in order(src)] != [names[i] for i in order(dst)]
    torch.manual_seed(99)
    with pytest.warns(UserWarning, match='wd'):
        res = dst.load(path)
    _same_state(src, dst)
    assert res['step'] == 7 == dst.steps == dst.ln_steps_checked
    assert res['missing_keys'] == [] and res['unexpected_keys'] == []
    assert res['hyper_mismatch'] == {'wd': (0.0, 0.1)}
    assert dst.wd == 0.1                                   # the constructor's holds
    assert dst.flat.grad.abs().max().item() == 0.0
    # RNG: the dropout counter, the seed and the generator state continue the saved run
    assert dst.model.text_transformer.dropout_state() == 5
    assert torch.initial_seed() == 1234
    assert torch.equal(torch.rand(4), after)
    # restore_rng=False leaves all three alone
    dst.model.text_transformer.set_dropout_state(11)
    torch.manual_seed(99)
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        dst.load(path, restore_rng=False)
    assert dst.model.text_transformer.dropout_state() == 11 and torch.initial_seed() == 99


def test_file_contents(source):
    src, path, _ = source
    pkg = torch.load(path, map_location='cpu', weights_only=True)
    assert pkg['format'] == 1
    assert set(pkg) == {'format', 'model', 'optim', 'hyper', 'rng'}
    assert pkg['model'].keys() == src.model.state_dict().keys()

    def walk(o):
        if isinstance(o, torch.Tensor):
            assert o.device.type == 'cpu'
            # compact: never a view that drags a whole arena into the file
            assert o.untyped_storage().nbytes() == o.numel() * o.element_size()
        elif isinstance(o, dict):
            assert all(isinstance(k, str) for k in o)
            for v in o.values():
                walk(v)
        elif isinstance(o, (list, tuple)):
            for v in o:
                walk(v)
        else:
            assert type(o) in (str, int, float, bool), type(o)
    walk(pkg)
    trainable = [n for n, p in src.model.named_parameters() if p.requires_grad]
    frozen = [n for n, p in src.model.named_parameters() if not p.requires_grad]
    assert frozen and set(pkg['optim']) == {'exp_avg', 'exp_avg_sq', 'step'}
    assert list(pkg['optim']['exp_avg']) == trainable == list(pkg['optim']['exp_avg_sq'])
    assert pkg['optim']['step'] == 7
    assert pkg['hyper'] == dict(lr=1.25e-6, wd=0.0, betas=(0.9, 0.99), eps=1e-8, max_grad_norm=0.5)
    assert pkg['rng']['initial_seed'] == 1234 and pkg['rng']['dropout_calls'] == 5
    assert pkg['rng']['cpu'].dtype == torch.uint8


def _fresh(seed=3, **kw):
    from ctclip_mi355x.trainer import CTClipTrainer
    tr = CTClipTrainer(_model(seed), **kw)
    _fill(tr, 50 + seed, steps=2)
    snap = (tr.flat.data.clone(), tr.m.clone(), tr.v.clone(), tr.steps)
    return tr, snap


def _untouched(tr, snap, weights=True):
    if weights:
        assert torch.equal(tr.flat.data, snap[0])
    assert torch.equal(tr.m, snap[1]) and torch.equal(tr.v, snap[2]) and tr.steps == snap[3]


def test_refusals_missing_and_misshapen_optimizer_entry(source, tmp_path):
    _, path, _ = source
    pkg = torch.load(path, map_location='cpu', weights_only=True)
    name = 'text_transformer.encoder.layer.0.attention.self.key.weight'
    dst, snap = _fresh()
    for strict in (True, False):
        bad = dict(pkg, optim=dict(pkg['optim'], exp_avg_sq={k: v for k, v in pkg['optim']['exp_avg_sq'].items()
                                                            if k != name}))
        torch.save(bad, str(tmp_path / 'missing.pt'))
        with pytest.raises(KeyError, match=name.replace('.', r'\.')):
            dst.load(str(tmp_path / 'missing.pt'), strict=strict)
        _untouched(dst, snap)              # nothing half-read: not even the weights
        bad = dict(pkg, optim=dict(pkg['optim'], exp_avg=dict(pkg['optim']['exp_avg'],
                                                              **{name: pkg['optim']['exp_avg'][name][:, :-1]})))
        torch.save(bad, str(tmp_path / 'shape.pt'))
        with pytest.raises(ValueError, match=name.replace('.', r'\.')):
            dst.load(str(tmp_path / 'shape.pt'), strict=strict)
        _untouched(dst, snap)
    # optimizer state for a name that is not trainable here: raises under strict, listed otherwise
    extra = dict(pkg, optim=dict(pkg['optim'], exp_avg=dict(pkg['optim']['exp_avg'], ghost=torch.zeros(2)),
                                 exp_avg_sq=dict(pkg['optim']['exp_avg_sq'], ghost=torch.zeros(2))))
    torch.save(extra, str(tmp_path / 'extra.pt'))
    with pytest.raises(KeyError, match='ghost'):
        dst.load(str(tmp_path / 'extra.pt'))
    _untouched(dst, snap)
    res = dst.load(str(tmp_path / 'extra.pt'), strict=False)
    assert res['unexpected_keys'] == ['optim.ghost'] and res['step'] == 7
    # another format version is refused, not guessed at
    torch.save(dict(pkg, format=2), str(tmp_path / 'v2.pt'))
    with pytest.raises(ValueError, match='format'):
        dst.load(str(tmp_path / 'v2.pt'))


def test_refusal_foreign_optimizer(source, tmp_path):
    """The reference trainer's {model, optim} with a positional torch.optim.Adam state: the weights are
    loaded, the optimizer state is refused with the reason, moments and step count stay."""
    from ctclip_mi355x.checkpoint import ForeignOptimizerError
    src, _, _ = source
    ref = _model(0)
    opt = torch.optim.Adam([p for p in ref.parameters() if p.requires_grad], lr=1e-3)
    for p in opt.param_groups[0]['params'][:3]:
        p.grad = torch.ones_like(p)
    opt.step()
    sd = {k: v.detach().clone() for k, v in src.model.state_dict().items()}
    torch.save({'model': sd, 'optim': opt.state_dict()}, str(tmp_path / 'ref.pt'))
    dst, snap = _fresh()
    with pytest.raises(ForeignOptimizerError, match=r'set\(\) of parameters') as ei:
        dst.load(str(tmp_path / 'ref.pt'))
    assert ei.value.result['step'] == 2 and ei.value.result['missing_keys'] == []
    _untouched(dst, snap, weights=False)
    for k, v in dst.model.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_bare_state_dict_with_module_prefix_loads_every_weight(source, tmp_path):
    """The reference's periodic save (CTCLIPTrainer.py:456-464) of a wrapped model: every key starts
    with 'module.'.  Every weight is loaded; moments and step count are left alone."""
    src, _, _ = source
    sd = {k: v.detach().clone() for k, v in src.model.state_dict().items()}
    torch.save({'module.' + k: v for k, v in sd.items()}, str(tmp_path / 'CTClip.100.pt'))
    dst, snap = _fresh()
    assert not torch.equal(dst.flat.data, src.flat.data)
    res = dst.load(str(tmp_path / 'CTClip.100.pt'))
    assert res['missing_keys'] == [] and res['unexpected_keys'] == [] and res['step'] == 2
    got = dst.model.state_dict()
    assert got.keys() == sd.keys()
    for k in sd:
        assert torch.equal(got[k], sd[k]), k
    for n, p in dst.model.named_parameters():      # ... and the trainable ones landed in the arena
        if p.requires_grad:
            assert dst.flat.data.data_ptr() <= p.data_ptr() < dst.flat.data.data_ptr() + 4 * dst.flat.numel
    _untouched(dst, snap, weights=False)


def test_atomic_write(source, tmp_path, monkeypatch):
    src, path, _ = source
    target = tmp_path / 'ck.pt'
    target.write_bytes(open(path, 'rb').read())
    before = target.read_bytes()
    real = torch.save

    def boom(obj, f, *a, **kw):
        f.write(b'half a checkpoint')           # the temporary file is open and written to
        raise OSError('disk full')
    monkeypatch.setattr(torch, 'save', boom)
    with pytest.raises(OSError, match='disk full'):
        src.save(str(target))
    monkeypatch.setattr(torch, 'save', real)
    assert target.read_bytes() == before
    assert sorted(os.listdir(tmp_path)) == ['ck.pt']
    src.save(str(target))                        # and a good write replaces it, leaving no .tmp either
    assert sorted(os.listdir(tmp_path)) == ['ck.pt']
    assert torch.load(str(target), weights_only=True)['optim']['step'] == 7


# ------------------------------------------------------------------ gloo, N = 2
def _rank_worker(rank, port, ck_dir, out_dir):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=WORLD)
    try:
        from ctclip_mi355x.trainer import CTClipTrainer
        path = os.path.join(ck_dir, 'ck.pt')
        src = CTClipTrainer(_model(0))
        _fill(src, 1)
        if rank != 0:
            def refuse(*a, **kw):
                raise AssertionError('a rank other than 0 wrote the checkpoint')
            real, torch.save = torch.save, refuse
        src.save(path)                         # both ranks call; returns on both (barrier inside)
        if rank != 0:
            torch.save = real
        assert os.listdir(ck_dir) == ['ck.pt']  # rank 0 finished the write before anyone left the barrier
        dst = CTClipTrainer(_model(10 + rank), wd=0.1 * rank, overlap_grad_sync=rank == 0)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            res = dst.load(path)
        assert res['step'] == 7
        _same_state(src, dst)
        # ... and the two ranks hold equal state, name by name (their arena orders differ)
        mine = torch.cat([torch.cat([p.detach().reshape(-1), m.reshape(-1), v.reshape(-1)])
                          for (n, p), (m, v) in zip(((n, q) for n, q in dst.model.named_parameters()
                                                     if q.requires_grad), _moments(dst).values())])
        both = [torch.empty_like(mine) for _ in range(WORLD)]
        dist.all_gather(both, mine)
        assert torch.equal(both[0], both[1])
        open(os.path.join(out_dir, f'ok{rank}'), 'w').close()
    finally:
        dist.destroy_process_group()


def test_two_ranks_save_once_and_load_equal(tmp_path):
    ck, out = tmp_path / 'ck', tmp_path / 'out'
    ck.mkdir()
    out.mkdir()
    mp.spawn(_rank_worker, args=(_free_port(), str(ck), str(out)), nprocs=WORLD, join=True)
    assert all((out / f'ok{r}').exists() for r in range(WORLD))
    assert os.listdir(ck) == ['ck.pt']
