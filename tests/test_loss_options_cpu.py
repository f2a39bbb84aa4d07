"""The reference's loss options -- decoupled contrastive learning, the extra (CLOOB) latent
projection, image multiview (ct_clip/ct_clip.py:663-675, 780-790, 845-899) -- on the CPU:

  * ``general_loss`` below is a fresh fp32 torch restatement of the general loss; it is pinned to
    the reference by tests/golden/golden_loss_options.safetensors (the reference's own CTCLIP at
    the tiny configuration, tests/golden/make_golden_loss_options.py): losses and the projection /
    temperature gradients.  The GPU tests (test_gpu_loss_options.py) check the HIP kernel against
    this restatement;
  * the constructor / forward validation of ``ctclip_mi355x.CTCLIP``;
  * the distributed layout of ``functional.ClipLossExFn`` under gloo (world 2), with the
    restatement as ``impl=``.
"""
import os
import socket
import types

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from oracle import ctclip_oracle as O
from oracle import weights as W

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'golden_loss_options.safetensors')
# tag -> (decoupled, extra projection, augmented image views), as the fixture's generator
CASES = {'plain': (False, False, 0), 'dcl': (True, False, 0), 'extra': (False, True, 0), 'all': (True, True, 2)}
MV_WEIGHT = 0.1          # CTCLIP's default multiview_loss_weight (ct_clip.py:447)


# ------------------------------------------------------------------------------ restatement
def general_loss(t_raw, i_raw, log_temp, t_extra=None, i_extra=None, decoupled=False, w_main=1.0, w_multiview=0.0):
    """Raw latent view stacks t_raw [Vt, B, D], i_raw [Vi, B, D] (view 0 = the un-augmented batch),
    optionally a second pair for the image -> text direction.  Every latent is scaled to unit length
    (norm floor 1e-12).  For each (text view m, image view n), in the order m-major:
      text -> image logits  L[x, y] = exp(log_temp) <t_m[x], i_n[y]>,
      image -> text logits  M[y, x] = L[x, y], or exp(log_temp) <i'_n[y], t'_m[x]> with the extra pair;
      per direction and row: -log(exp(own logit) + 1e-20) + log(sum of exp over the row + 1e-20),
      the own (diagonal) term left out of that sum when ``decoupled``; no max is subtracted;
      pair loss = half the sum of the two directions' row means.
    Returns (w_main * loss of pair 0 + w_multiview * mean of the remaining pairs, pair losses)."""
    temp = log_temp.reshape(()).exp()
    unit = lambda x: x / x.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    t, i = unit(t_raw), unit(i_raw)
    tx, ix = (unit(t_extra), unit(i_extra)) if t_extra is not None else (t, i)
    B = t.shape[1]
    off_diag = 1.0 - torch.eye(B, dtype=t.dtype, device=t.device)

    def direction(logits):                      # rows = queries, columns = candidates
        e = logits.exp()
        own = e.diagonal()
        total = (e * off_diag).sum(1) if decoupled else e.sum(1)
        return (torch.log(total + 1e-20) - torch.log(own + 1e-20)).mean()

    pair = []
    for m in range(t.shape[0]):
        for n in range(i.shape[0]):
            t2i = temp * t[m] @ i[n].t()
            i2t = temp * ix[n] @ tx[m].t()
            pair.append(0.5 * (direction(t2i) + direction(i2t)))
    pair = torch.stack(pair)
    loss = w_main * pair[0]
    if pair.numel() > 1:
        loss = loss + w_multiview * pair[1:].mean()
    return loss, pair


def loss_and_grads(t_raw, i_raw, log_temp, t_extra=None, i_extra=None, decoupled=False, w_main=1.0, w_multiview=0.0):
    """``general_loss`` with the outputs of kernels.clip_loss_ex: (loss [1], dt, di, dt_extra,
    di_extra, dlt [1], pair losses) -- the ``impl=`` of functional.ClipLossExFn."""
    leaf = lambda x: None if x is None else x.detach().clone().requires_grad_(True)
    t, i, tx, ix, lt = leaf(t_raw), leaf(i_raw), leaf(t_extra), leaf(i_extra), leaf(log_temp)
    with torch.enable_grad():                   # called inside an autograd.Function forward
        loss, pair = general_loss(t, i, lt, tx, ix, decoupled, w_main, w_multiview)
        loss.backward()
    return (loss.detach().reshape(1), t.grad, i.grad, None if tx is None else tx.grad, None if ix is None else ix.grad,
            lt.grad.reshape(1), pair.detach())


# ------------------------------------------------------------------------------ fixture pin
def _close(a, b, tol):      # as tests/test_oracle_golden.py
    a, b = a.double(), b.double()
    err = (a - b).abs().max().item()
    scale = max(1.0, b.abs().max().item())
    assert err <= tol * scale, f'max err {err} (scale {scale})'


@pytest.fixture(scope='module')
def golden():
    from safetensors.torch import load_file
    return load_file(GOLDEN)


def _weights(tag):
    dcl, extra, naug = CASES[tag]
    return dcl, extra, naug + 1, (1.0 - MV_WEIGHT if naug else 1.0), (MV_WEIGHT if naug else 0.0)


@pytest.mark.parametrize('tag', list(CASES))
def test_restatement_reproduces_reference_loss(golden, tag):
    """The fixture's (unit) latents through the restatement give the reference's loss, to the 1e-5
    of the tiny loss in test_oracle_golden.py."""
    dcl, extra, nv, w_main, w_mv = _weights(tag)
    lat = {n: golden[f'{tag}.latents.{n}'] for n in ('text', 'image')}
    B, D = lat['text'].shape
    assert lat['image'].shape == (nv * B, D)
    tx = golden[f'{tag}.latents.text_extra'].view(1, B, D) if extra else None
    ix = golden[f'{tag}.latents.image_extra'].view(nv, B, D) if extra else None
    assert (f'{tag}.latents.text_extra' in golden) == extra
    loss, pair = general_loss(lat['text'].view(1, B, D), lat['image'].view(nv, B, D), torch.tensor(1.0), tx, ix, dcl,
                              w_main, w_mv)
    _close(loss.reshape(1), golden[f'{tag}.loss'], 1e-5)
    assert pair.shape == (nv,)


@pytest.mark.parametrize('tag', list(CASES))
def test_restatement_reproduces_reference_gradients(golden, tag):
    """Raw latents rebuilt from the recorded projection inputs and the recipe weights; the
    restatement's gradients of the four projection weights and the temperature against the
    reference's (2e-4, the gradient tolerance of test_oracle_golden.py), and the scores."""
    dcl, extra, nv, w_main, w_mv = _weights(tag)
    sd = W.make_state_dict(O.TINY)
    names = ['to_text_latent.weight', 'to_visual_latent.weight', 'temperature']
    if extra:
        names += ['to_text_latent_extra.weight', 'to_visual_latent_extra.weight']
    p = {n: sd[n].clone().requires_grad_(True) for n in names}
    cls, pooled = golden['in.cls'], golden['in.pooled']
    B = cls.shape[0]
    pooled = pooled[:nv * B]
    proj = lambda x, n, v: F.linear(x, p[n]).view(v, B, -1)
    t, i = proj(cls, 'to_text_latent.weight', 1), proj(pooled, 'to_visual_latent.weight', nv)
    tx = proj(cls, 'to_text_latent_extra.weight', 1) if extra else None
    ix = proj(pooled, 'to_visual_latent_extra.weight', nv) if extra else None
    _close(F.normalize(i.detach().reshape(nv * B, -1), dim=-1), golden[f'{tag}.latents.image'], 1e-5)
    loss, _ = general_loss(t, i, p['temperature'], tx, ix, dcl, w_main, w_mv)
    _close(loss.detach().reshape(1), golden[f'{tag}.loss'], 1e-5)
    loss.backward()
    for n in names:
        _close(p[n].grad, golden[f'{tag}.grad.{n}'], 2e-4)
    assert (f'{tag}.grad.to_text_latent_extra.weight' in golden) == extra
    # eval scores (ct_clip.py:805-807): the extra latents when text_to_image is False
    un = lambda x: F.normalize(x.detach()[0], dim=-1)
    temp = sd['temperature'].exp()
    _close((un(t) * un(i)).sum(-1) * temp, golden[f'{tag}.scores.t2i'], 1e-5)
    i2t = (un(tx) * un(ix)).sum(-1) * temp if extra else (un(t) * un(i)).sum(-1) * temp
    _close(i2t, golden[f'{tag}.scores.i2t'], 1e-5)
    if extra:
        assert not torch.allclose(golden[f'{tag}.scores.t2i'], golden[f'{tag}.scores.i2t'])


def test_restatement_plain_is_oracle_infonce():
    g = torch.Generator().manual_seed(3)
    t, i = torch.randn(1, 5, 16, generator=g), torch.randn(1, 5, 16, generator=g)
    lt = torch.tensor(1.3)
    loss, _ = general_loss(t, i, lt)
    ref = O.infonce(F.normalize(t[0], dim=-1), F.normalize(i[0], dim=-1), lt)
    assert abs(loss.item() - ref.item()) < 1e-6


# ------------------------------------------------------------------------------ validation
class _Stop(Exception):
    pass


class _Tower(torch.nn.Module):
    """Stands in for both encoders: reaching it means forward's validation let the call through."""

    def forward(self, *a, **k):
        raise _Stop

    def encode_pooled(self, *a, **k):
        raise _Stop


def _model(**kw):
    from ctclip_mi355x.ct_clip import CTCLIP
    return CTCLIP(image_encoder=_Tower(), text_encoder=_Tower(), dim_text=8, dim_image=8, dim_latent=4, **kw)


def test_constructor_accepts_the_loss_options():
    m = _model(decoupled_contrastive_learning=True, extra_latent_projection=True)
    assert m.decoupled_contrastive_learning and m.extra_latent_projection
    assert {'to_text_latent_extra.weight', 'to_visual_latent_extra.weight'} <= set(m.state_dict())
    for opt in ('use_all_token_embeds', 'use_mlm', 'use_visual_ssl', 'text_causal_mask', 'downsample_image_embeds'):
        with pytest.raises(NotImplementedError, match='outside the contrastive hot path'):
            _model(**{opt: True})


def test_forward_validation():
    text = types.SimpleNamespace(input_ids=torch.zeros(2, 4, dtype=torch.long), attention_mask=torch.ones(2, 4))
    image = torch.zeros(2, 1, 4, 8, 8)
    m = _model()
    with pytest.raises(AssertionError, match='do not pass in augmented'):
        m(text, image, aug_image=image.clone())                    # no views without return_loss
    with pytest.raises(AssertionError, match='multiview loss weight cannot be 0'):
        _model(multiview_loss_weight=0)(text, image, return_loss=True, aug_image=(image.clone(),))
    with pytest.raises(AssertionError, match='shape'):
        m(text, image, return_loss=True, aug_image=image[:1].clone())
    with pytest.raises(NotImplementedError, match='multiview augmentation is off'):
        m(text, image, return_loss=True, aug_text=text)
    with pytest.raises(_Stop):                                     # a valid multiview call reaches the towers
        m(text, image, return_loss=True, aug_image=(image.clone(), image.clone()))


# ------------------------------------------------------------------------------ gloo, world 2
WORLD, B, DIN, DL, VI = 2, 3, 16, 8, 2


def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


def _problem():
    g = torch.Generator().manual_seed(17)
    r = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).float()
    x = dict(xt=r(WORLD * B, DIN), xi=r(VI, WORLD * B, DIN))
    w = {n: r(DIN, DL) for n in ('wt', 'wi', 'wtx', 'wix')}
    return x, w


def _loss_fn(x, w, lt, rows, apply):
    """DCL + extra projection + one augmented view on the rows ``rows`` of the global batch."""
    xt, xi = x['xt'][rows], x['xi'][:, rows]
    return apply((xt @ w['wt'])[None], xi @ w['wi'], (xt @ w['wtx'])[None], xi @ w['wix'], lt)


def _single_process():
    x, w = _problem()
    w = {n: v.requires_grad_(True) for n, v in w.items()}
    lt = torch.tensor(1.0, requires_grad=True)
    loss = _loss_fn(x, w, lt, slice(None),
                    lambda t, i, tx, ix, l: general_loss(t, i, l, tx, ix, True, 1.0 - MV_WEIGHT, MV_WEIGHT)[0])
    loss.backward()
    return loss.detach(), {n: v.grad for n, v in w.items()}, lt.grad


def _worker(rank, port, out_dir):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=WORLD)
    try:
        from ctclip_mi355x import dist_sync
        from ctclip_mi355x.functional import ClipLossExFn
        x, w0 = _problem()
        ref_loss, ref_g, ref_glt = _single_process()
        rows = slice(rank * B, (rank + 1) * B)
        for early in (False, True):
            w = {n: torch.nn.Parameter(v.clone()) for n, v in w0.items()}
            lt = torch.nn.Parameter(torch.tensor(1.0))

            def apply(t, i, tx, ix, l):
                # early: the text sets' gather started ahead of the loss (CTCLIP.encode), both on one collective
                h = dist_sync.start_gather_stacks([t, tx]) if early else None
                return ClipLossExFn.apply(t, i, tx, ix, l, True, 1.0 - MV_WEIGHT, MV_WEIGHT, loss_and_grads, h)
            loss = _loss_fn(x, w, lt, rows, apply)
            loss.backward()
            assert torch.allclose(loss.detach(), ref_loss, rtol=1e-6, atol=1e-6), (loss.item(), ref_loss.item())
            # every rank back-propagated its own rows of the global loss: the SUM is the global gradient
            for n, prm in list(w.items()) + [('lt', lt)]:
                dist.all_reduce(prm.grad)
                torch.testing.assert_close(prm.grad, ref_glt if n == 'lt' else ref_g[n], rtol=1e-5, atol=1e-6)
        # gathered stacks keep the view axis; within a view the rows arrive in rank order
        a = torch.full((2, B, DL), float(rank)) + torch.tensor([0.0, 100.0]).view(2, 1, 1)
        (ga,), (gb,) = dist_sync.gather_stacks([a], [a[:1] + 10.0])
        ranks = torch.arange(WORLD).repeat_interleave(B).float()
        assert ga.shape == (2, WORLD * B, DL) and gb.shape == (1, WORLD * B, DL)
        assert torch.equal(ga[0, :, 0], ranks) and torch.equal(ga[1, :, 0], ranks + 100) and torch.equal(gb[0, :, 0], ranks + 10)
        assert torch.equal(dist_sync.local_view_rows(ga, B), a)
        open(os.path.join(out_dir, f'ok{rank}'), 'w').close()
    finally:
        dist.destroy_process_group()


def test_two_rank_general_loss(tmp_path):
    """DCL + extra + one augmented view: the two-rank loss and the summed local-row gradients equal
    the one-process result on the concatenated batch (negatives span the global batch per view)."""
    mp.spawn(_worker, args=(_free_port(), str(tmp_path)), nprocs=WORLD, join=True)
    assert all((tmp_path / f'ok{r}').exists() for r in range(WORLD))


def test_single_process_function_matches_restatement():
    from ctclip_mi355x.functional import ClipLossExFn
    x, w0 = _problem()
    w = {n: v.clone().requires_grad_(True) for n, v in w0.items()}
    lt = torch.tensor(1.0, requires_grad=True)
    loss = _loss_fn(x, w, lt, slice(None), lambda t, i, tx, ix, l: ClipLossExFn.apply(
        t, i, tx, ix, l, True, 1.0 - MV_WEIGHT, MV_WEIGHT, loss_and_grads))
    (3.0 * loss).backward()
    ref_loss, ref_g, ref_glt = _single_process()
    assert torch.allclose(loss.detach(), ref_loss)
    for n in w:
        torch.testing.assert_close(w[n].grad, 3.0 * ref_g[n])
    torch.testing.assert_close(lt.grad, 3.0 * ref_glt)
