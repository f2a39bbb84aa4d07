"""The pairwise sigmoid (SigLIP) loss without a GPU: the torch restatement of
sigmoid_loss_common.py against a hand-written double loop and finite differences, ``SigmoidLossFn``'s
exchange logic under gloo with the restatement standing in for the kernel, CTCLIP's constructor options,
and the C header / ctypes table entries of the new entry point."""
import math
import os
import re
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from sigmoid_loss_common import TEMP_BIAS, loss_and_grads, sigmoid_loss

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLD, B, DIN, DL = 2, 3, 16, 8


def _latents(Bg, Dl, seed, dtype=torch.float64):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(Bg, Dl, generator=g, dtype=dtype), torch.randn(Bg, Dl, generator=g, dtype=dtype)


# ------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('lt,b', TEMP_BIAS)
def test_restatement_against_double_loop(lt, b):
    """Bg = 3: every pair by hand in Python floats (f64), log(1 + exp(.)) written out."""
    t, i = _latents(3, 5, 1)
    loss = sigmoid_loss(t, i, torch.tensor(lt, dtype=torch.float64), torch.tensor(b, dtype=torch.float64)).item()
    tl, il = t.tolist(), i.tolist()
    norm = lambda v: max(math.sqrt(sum(x * x for x in v)), 1e-12)
    tot = 0.0
    for a in range(3):
        for c in range(3):
            cos = sum(x * y for x, y in zip(tl[a], il[c])) / (norm(tl[a]) * norm(il[c]))
            x = math.exp(lt) * cos + b
            z = 1.0 if a == c else -1.0
            tot += math.log(1.0 + math.exp(-z * x))
    assert abs(loss - tot / 3) < 1e-12 * max(1.0, abs(tot / 3))


def test_restatement_softplus_is_stable():
    """|x| = 40 and 800 on both signs: finite, softplus(u) = u for large u and exp(u) for very negative u."""
    from sigmoid_loss_common import softplus
    u = torch.tensor([-800.0, -40.0, 0.0, 40.0, 800.0], dtype=torch.float64)
    s = softplus(u)
    assert torch.isfinite(s).all()
    assert s[0].item() == 0.0 and s[4].item() == 800.0 and abs(s[2].item() - math.log(2)) < 1e-15
    assert abs(s[1].item() - math.exp(-40.0)) < 1e-30 and abs(s[3].item() - 40.0) < 1e-14


@pytest.mark.parametrize('lt,b', TEMP_BIAS)
def test_restatement_gradients_against_finite_differences(lt, b):
    """Central differences in f64, step 1e-6: truncation ~1e-12 |f'''|, rounding ~1e-16 |f| / 1e-6 = 1e-10,
    against gradients of order 1e-3 .. 1: 1e-6 relative per tensor."""
    t, i = _latents(4, 6, 2)
    ltt, bt = torch.tensor([lt], dtype=torch.float64), torch.tensor([b], dtype=torch.float64)
    _, dt, di, dlt, db = loss_and_grads(t, i, ltt, bt)
    args = [t, i, ltt, bt]
    h = 1e-6
    for k, g in enumerate((dt, di, dlt, db)):
        fd = torch.zeros_like(args[k])
        for e in range(args[k].numel()):
            hi = [a.clone() for a in args]
            lo = [a.clone() for a in args]
            hi[k].view(-1)[e] += h
            lo[k].view(-1)[e] -= h
            fd.view(-1)[e] = (sigmoid_loss(*hi) - sigmoid_loss(*lo)) / (2 * h)
        assert ((fd - g).norm() / g.norm()).item() < 1e-6, k


def test_restatement_gradient_formulas():
    """The closed forms the kernel evaluates: g = -z sigmoid(-z x) / Bg, dbias = sum g, dlt = temp sum g s."""
    t, i = _latents(5, 7, 3)
    lt, b = torch.tensor([0.7], dtype=torch.float64), torch.tensor([-1.5], dtype=torch.float64)
    _, dt, di, dlt, db = loss_and_grads(t, i, lt, b)
    tn, inn = torch.nn.functional.normalize(t, dim=-1), torch.nn.functional.normalize(i, dim=-1)
    s = tn @ inn.t()
    z = 2.0 * torch.eye(5, dtype=torch.float64) - 1.0
    g = -z * torch.sigmoid(-z * (lt.exp() * s + b)) / 5
    assert abs(db.item() - g.sum().item()) < 1e-14
    assert abs(dlt.item() - (lt.exp() * (g * s).sum()).item()) < 1e-14
    dtn = lt.exp() * g @ inn                      # then the l2norm backward
    ref = (dtn - tn * (dtn * tn).sum(-1, keepdim=True)) / t.norm(dim=-1, keepdim=True)
    assert ((dt - ref).norm() / ref.norm()).item() < 1e-13


# ------------------------------------------------------------------------------ exchange under gloo
def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _problem():
    g = torch.Generator().manual_seed(17)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float()
    return r(WORLD * B, DIN), r(WORLD * B, DIN), r(DIN, DL), r(DIN, DL)


def _single_process():
    xt, xi, wt, wi = _problem()
    prm = [wt.requires_grad_(True), wi.requires_grad_(True), torch.tensor(1.2, requires_grad=True),
           torch.tensor(-2.0, requires_grad=True)]
    t, i = xt @ prm[0], xi @ prm[1]
    t.retain_grad()
    i.retain_grad()
    loss = 3.0 * sigmoid_loss(t, i, prm[2], prm[3])
    loss.backward()
    return loss.detach() / 3.0, t.grad, i.grad, [p.grad for p in prm]


def _worker(rank, port, out_dir):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=WORLD)
    try:
        from ctclip_mi355x import dist_sync
        from ctclip_mi355x.functional import SigmoidLossFn
        xt, xi, wt0, wi0 = _problem()
        ref_loss, ref_dt, ref_di, ref_g = _single_process()
        rows = slice(rank * B, (rank + 1) * B)
        for early in (False, True):
            prm = [torch.nn.Parameter(wt0.clone()), torch.nn.Parameter(wi0.clone()),
                   torch.nn.Parameter(torch.tensor(1.2)), torch.nn.Parameter(torch.tensor(-2.0))]
            t, i = xt[rows] @ prm[0], xi[rows] @ prm[1]
            t.retain_grad()
            i.retain_grad()
            h = dist_sync.start_gather(t) if early else None      # the gather CTCLIP.encode starts early
            loss = SigmoidLossFn.apply(t, i, prm[2], prm[3], loss_and_grads, h)
            (3.0 * loss).backward()                               # a non-unit upstream gradient
            # every rank holds the same global loss; its own rows' latent gradients are the global batch's
            assert torch.allclose(loss.detach(), ref_loss, rtol=1e-6, atol=1e-6), (loss.item(), ref_loss.item())
            torch.testing.assert_close(t.grad, ref_dt[rows], rtol=1e-5, atol=1e-7)
            torch.testing.assert_close(i.grad, ref_di[rows], rtol=1e-5, atol=1e-7)
            # dlt and dbias are the full values scaled by 1 / world: the SUM all-reduce gives them once
            for p, r in zip(prm, ref_g):
                dist.all_reduce(p.grad)
                torch.testing.assert_close(p.grad, r, rtol=1e-5, atol=1e-6)
        open(os.path.join(out_dir, f'ok{rank}'), 'w').close()
    finally:
        dist.destroy_process_group()


def test_two_rank_exchange_equals_single_process(tmp_path):
    mp.spawn(_worker, args=(_free_port(), str(tmp_path)), nprocs=WORLD, join=True)
    assert all((tmp_path / f'ok{r}').exists() for r in range(WORLD))


def test_single_process_function_with_impl():
    from ctclip_mi355x.functional import SigmoidLossFn
    xt, xi, wt0, wi0 = _problem()
    prm = [wt0.clone().requires_grad_(True), wi0.clone().requires_grad_(True),
           torch.tensor(1.2, requires_grad=True), torch.tensor(-2.0, requires_grad=True)]
    loss = SigmoidLossFn.apply(xt @ prm[0], xi @ prm[1], prm[2], prm[3], loss_and_grads)
    (3.0 * loss).backward()
    ref_loss, _, _, ref_g = _single_process()
    assert torch.allclose(loss.detach(), ref_loss)
    for p, r in zip(prm, ref_g):
        torch.testing.assert_close(p.grad, r, rtol=1e-5, atol=1e-6)


# ------------------------------------------------------------------------------ constructor
def _ctclip(**kw):
    from ctclip_mi355x.ct_clip import CTCLIP
    enc = torch.nn.Linear(4, 4)
    enc.dim = 4
    return CTCLIP(image_encoder=enc, text_encoder=torch.nn.Linear(4, 4), dim_text=4, dim_image=4, dim_latent=4, **kw)


def test_constructor_registers_the_bias_only_with_the_option():
    plain = _ctclip()
    assert 'logit_bias' not in plain.state_dict() and not hasattr(plain, 'logit_bias') and not plain.sigmoid_loss
    assert plain.temperature.item() == 1.0
    m = _ctclip(sigmoid_loss=True)
    assert set(m.state_dict()) - set(plain.state_dict()) == {'logit_bias'}
    assert isinstance(m.logit_bias, torch.nn.Parameter) and m.logit_bias.ndim == 0 and m.logit_bias.item() == -10.0
    assert m.temperature.item() == 1.0                      # keeps its constructor value
    m = _ctclip(sigmoid_loss=True, sigmoid_bias_init=-3.0, sigmoid_temperature_init=math.log(10.0))
    assert m.logit_bias.item() == -3.0 and abs(m.temperature.item() - math.log(10.0)) < 1e-7
    assert _ctclip(sigmoid_temperature_init=2.0).temperature.item() == 1.0      # an InfoNCE model ignores it
    # a plain state_dict into a sigmoid model: the bias is reported missing
    res = m.load_state_dict(plain.state_dict(), strict=False)
    assert list(res.missing_keys) == ['logit_bias'] and not res.unexpected_keys


def test_head_bucket_keeps_scalars_behind_the_projections():
    """The optimizer arena is packed: both scalars sort behind every parameter whose size is a multiple of
    8, so the projections' bf16 shadows keep their 16-byte alignment."""
    m = _ctclip(sigmoid_loss=True)
    m.visual_transformer.enc_temporal_transformer = torch.nn.Identity()
    m.visual_transformer.enc_spatial_transformer = torch.nn.Identity()
    head = dict(m.grad_buckets())['head']
    assert any(p is m.logit_bias for p in head)
    sizes = [p.numel() % 8 != 0 for p in head]
    assert sizes == sorted(sizes) and sizes[-2:] == [True, True]


@pytest.mark.parametrize('name', ['decoupled_contrastive_learning', 'extra_latent_projection', 'use_all_token_embeds'])
def test_refused_combinations_raise_by_name(name):
    with pytest.raises(NotImplementedError, match=f'sigmoid_loss with {name}'):
        _ctclip(sigmoid_loss=True, **{name: True})


def test_aug_image_is_refused_by_name():
    m = _ctclip(sigmoid_loss=True)
    x = torch.zeros(2, 4)
    with pytest.raises(NotImplementedError, match='sigmoid_loss with aug_image'):
        m(None, x, return_loss=True, aug_image=x)


# ------------------------------------------------------------------------------ C-ABI
def test_header_and_ctypes_table_declare_the_entry_points():
    from ctclip_mi355x import _lib
    h = open(os.path.join(REPO, 'include', 'ctclip_hip.h')).read()
    assert re.search(r'int ctclip_sigmoid_loss\(const ctclip_sigmoid_loss_args\* a, void\* stream\);', h)
    assert re.search(r'int64_t ctclip_sigmoid_loss_ws_bytes\(const ctclip_sigmoid_loss_args\* a\);', h)
    assert 'ctclip_sigmoid_loss' in _lib._SIGS and 'ctclip_sigmoid_loss_ws_bytes' in _lib._SIGS
    assert _lib._RESTYPES['ctclip_sigmoid_loss_ws_bytes'] is _lib.c_i64
    assert _lib.ABI_VERSION == 2
    # the struct mirrors the header field for field
    body = re.search(r'typedef struct \{([^}]*)\} ctclip_sigmoid_loss_args;', h).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = [n for decl in body.split(';') for n in re.findall(r'(\w+)\s*(?:,|$)', decl.replace('*', ' ').strip())]
    assert names == [f[0] for f in _lib.SigmoidLossArgs._fields_], names
