"""The multi-positive InfoNCE loss without a GPU: the torch restatement of
multipos_loss_common.py against a hand-written double loop, finite differences, plain InfoNCE and the
all-equal closed form; ``MultiPosLossFn``'s exchange logic under gloo with the restatement standing in for
the kernel; CTCLIP's constructor option and refusals; the id hash restatement; and the C header / ctypes
table entries of the new entry points."""
import math
import os
import re
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from multipos_loss_common import LOG_TEMPS, loss_and_grads, mix, multipos_loss, positive_count, report_id

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORLD, B, DIN, DL = 2, 3, 16, 8
F64 = torch.float64


def _latents(Bg, Dl, seed, dtype=F64):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(Bg, Dl, generator=g, dtype=dtype), torch.randn(Bg, Dl, generator=g, dtype=dtype)


# ------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize('lt', LOG_TEMPS)
def test_restatement_against_double_loop(lt):
    """Bg = 3, ids (7, 7, 9): every pair by hand in Python floats (f64), log(sum exp) written out."""
    t, i = _latents(3, 5, 1)
    ids = [7, 7, 9]
    loss = multipos_loss(t, i, torch.tensor(ids), torch.tensor(lt, dtype=F64)).item()
    tl, il = t.tolist(), i.tolist()
    norm = lambda v: max(math.sqrt(sum(x * x for x in v)), 1e-12)
    x = [[math.exp(lt) * sum(p * q for p, q in zip(tl[a], il[c])) / (norm(tl[a]) * norm(il[c])) for c in range(3)]
         for a in range(3)]
    tot = 0.0
    for a in range(3):
        pos = [c for c in range(3) if ids[c] == ids[a]]
        tot += math.log(sum(math.exp(x[a][c]) for c in range(3))) - sum(x[a][c] for c in pos) / len(pos)
        tot += math.log(sum(math.exp(x[c][a]) for c in range(3))) - sum(x[c][a] for c in pos) / len(pos)
    assert abs(loss - tot / 6) < 1e-12 * max(1.0, abs(tot / 6))
    assert positive_count(torch.tensor(ids)) == 2


@pytest.mark.parametrize('lt', LOG_TEMPS)
def test_restatement_gradients_against_finite_differences(lt):
    """Central differences in f64, step 1e-6: truncation ~1e-12 |f'''|, rounding ~1e-16 |f| / 1e-6 = 1e-10,
    against gradients of order 1e-3 .. 1: 1e-6 relative per tensor."""
    t, i = _latents(4, 6, 2)
    ids = torch.tensor([3, 5, 3, 8])
    ltt = torch.tensor([lt], dtype=F64)
    _, dt, di, dlt, npos = loss_and_grads(t, i, ids, ltt)
    assert npos.item() == 2
    args = [t, i, ltt]
    h = 1e-6
    f = lambda a: multipos_loss(a[0], a[1], ids, a[2])
    for k, g in enumerate((dt, di, dlt)):
        fd = torch.zeros_like(args[k])
        for e in range(args[k].numel()):
            hi = [a.clone() for a in args]
            lo = [a.clone() for a in args]
            hi[k].view(-1)[e] += h
            lo[k].view(-1)[e] -= h
            fd.view(-1)[e] = (f(hi) - f(lo)) / (2 * h)
        assert ((fd - g).norm() / g.norm()).item() < 1e-6, k


def test_restatement_gradient_formulas():
    """The closed forms the kernel evaluates: g = 1/2Bg [p_row + p_col - [same] (1/n_i + 1/n_j)],
    dlt = sum g x, dt^ = temp g i^ followed by the l2norm backward."""
    t, i = _latents(5, 7, 3)
    ids = torch.tensor([1, 2, 1, 1, 9])
    lt = torch.tensor([0.7], dtype=F64)
    _, dt, di, dlt, _ = loss_and_grads(t, i, ids, lt)
    tn, inn = torch.nn.functional.normalize(t, dim=-1), torch.nn.functional.normalize(i, dim=-1)
    x = lt.exp() * tn @ inn.t()
    same = (ids[:, None] == ids[None, :]).double()
    n = same.sum(1)
    g = (torch.softmax(x, 1) + torch.softmax(x, 0) - same * (1 / n[:, None] + 1 / n[None, :])) / 10
    assert abs(dlt.item() - (g * x).sum().item()) < 1e-14
    for grad, gm, self_n, other_n, raw in ((dt, g, tn, inn, t), (di, g.t(), inn, tn, i)):
        dn = lt.exp() * gm @ other_n
        ref = (dn - self_n * (dn * self_n).sum(-1, keepdim=True)) / raw.norm(dim=-1, keepdim=True)
        assert ((grad - ref).norm() / ref.norm()).item() < 1e-13


@pytest.mark.parametrize('lt', LOG_TEMPS)
def test_all_ids_distinct_is_plain_infonce(lt):
    """Against ``test_loss_options_cpu.general_loss``'s plain case, in f64.  The two forms differ by the 1e-20
    inside the reference's logs: per row and direction log(S + 1e-20) - log(e_own + 1e-20) against
    log S - log e_own, and 0 <= log(1 + 1e-20 / y) <= 1e-20 / y with y >= exp(-temp) (|x_ij| <= temp), so the
    losses differ by at most 1e-20 exp(temp).  On top, f64 rounding of the two evaluation orders: each of the
    2 Bg row terms is a difference of two numbers of size <= temp + log Bg, a few ulp each -- 32 eps of that
    size covers the exp / sum / log chains of both forms at Bg = 6."""
    from test_loss_options_cpu import general_loss
    Bg = 6
    t, i = _latents(Bg, 9, 4)
    ltt = torch.tensor(lt, dtype=F64)
    ours = multipos_loss(t, i, torch.arange(Bg) * 3 + 1, ltt).item()
    ref = general_loss(t[None], i[None], ltt)[0].item()
    temp = math.exp(lt)
    bound = 1e-20 * math.exp(temp) + 32 * 2.0 ** -52 * (temp + math.log(Bg))
    assert abs(ours - ref) <= bound, (ours, ref, bound)
    assert positive_count(torch.arange(Bg)) == 0


def test_all_ids_equal_closed_form():
    """One group: every row's and column's term is logsumexp - mean."""
    Bg = 5
    t, i = _latents(Bg, 4, 5)
    lt = torch.tensor(1.3, dtype=F64)
    loss = multipos_loss(t, i, torch.full((Bg,), 11), lt)
    x = lt.exp() * torch.nn.functional.normalize(t, dim=-1) @ torch.nn.functional.normalize(i, dim=-1).t()
    ref = 0.5 * ((torch.logsumexp(x, 1) - x.mean(1)).mean() + (torch.logsumexp(x, 0) - x.mean(0)).mean())
    assert abs(loss.item() - ref.item()) < 1e-14
    assert positive_count(torch.full((Bg,), 11)) == Bg * (Bg - 1)


def test_restatement_is_finite_at_temperature_100():
    t, i = _latents(4, 3, 6, dtype=torch.float32)
    i[1] = -t[1]                                 # a positive cosine of -1 ...
    i[0] = t[1]                                  # ... beside a negative cosine of +1
    out = loss_and_grads(t, i, torch.arange(4), torch.tensor([math.log(100.0)]))
    assert all(torch.isfinite(x).all() for x in out[:4])


# ------------------------------------------------------------------------------ the id hash
def test_report_id_rule():
    assert mix(0) == 0 and mix(1) == 0xb456bcfc34c2cb2c      # the splitmix64 finaliser (murmur3 fmix64)
    from ctclip_mi355x.augment import mix64
    assert all(mix(v) == mix64(v, 0) for v in (1, 2, 12345, (1 << 64) - 1))
    a = report_id([5, 6, 7, 0], [1, 1, 1, 0])
    assert a == report_id([5, 6, 7, 99], [1, 1, 1, 0])       # behind the mask
    assert a == report_id([5, 99, 6, 7], [1, 0, 1, 1])       # the kept tokens are the same sequence
    assert a != report_id([5, 6, 8, 0], [1, 1, 1, 0])        # one kept token
    assert a != report_id([5, 7, 6, 0], [1, 1, 1, 0])        # position
    assert a != report_id([5, 6, 7, 0], [1, 1, 1, 1])        # length
    assert a != report_id([5, 6, 0, 0], [1, 1, 0, 0])
    assert -(1 << 63) <= a < (1 << 63)
    assert report_id([3, 4], [0, 0]) == mix(0) == 0           # nothing kept: defined


# ------------------------------------------------------------------------------ exchange under gloo
def _free_port():
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        return s.getsockname()[1]


# rows 1 (rank 0) and 4 (rank 1) are one group: the duplicate spans the two ranks
IDS = torch.tensor([10, 77, 12, 13, 77, 15], dtype=torch.int64)


def _problem():
    g = torch.Generator().manual_seed(17)
    r = lambda *s: torch.randn(*s, generator=g, dtype=F64).float()
    return r(WORLD * B, DIN), r(WORLD * B, DIN), r(DIN, DL), r(DIN, DL)


def _single_process():
    xt, xi, wt, wi = _problem()
    prm = [wt.requires_grad_(True), wi.requires_grad_(True), torch.tensor(1.2, requires_grad=True)]
    t, i = xt @ prm[0], xi @ prm[1]
    t.retain_grad()
    i.retain_grad()
    loss = 3.0 * multipos_loss(t, i, IDS, prm[2])
    loss.backward()
    return loss.detach() / 3.0, t.grad, i.grad, [p.grad for p in prm]


def _worker(rank, port, out_dir):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=WORLD)
    try:
        from ctclip_mi355x import dist_sync
        from ctclip_mi355x.functional import MultiPosLossFn
        xt, xi, wt0, wi0 = _problem()
        ref_loss, ref_dt, ref_di, ref_g = _single_process()
        rows = slice(rank * B, (rank + 1) * B)
        for early in (False, True):
            prm = [torch.nn.Parameter(wt0.clone()), torch.nn.Parameter(wi0.clone()),
                   torch.nn.Parameter(torch.tensor(1.2))]
            t, i = xt[rows] @ prm[0], xi[rows] @ prm[1]
            t.retain_grad()
            i.retain_grad()
            h = dist_sync.start_gather(t) if early else None      # the gather CTCLIP.encode starts early
            loss, npos = MultiPosLossFn.apply(t, i, IDS[rows].clone(), prm[2], loss_and_grads, h)
            (3.0 * loss).backward()                               # a non-unit upstream gradient
            # every rank holds the same global loss and count; its own rows' gradients are the global batch's
            assert npos.item() == 2 and not npos.requires_grad
            assert torch.allclose(loss.detach(), ref_loss, rtol=1e-6, atol=1e-6), (loss.item(), ref_loss.item())
            torch.testing.assert_close(t.grad, ref_dt[rows], rtol=1e-5, atol=1e-7)
            torch.testing.assert_close(i.grad, ref_di[rows], rtol=1e-5, atol=1e-7)
            # dlt is the full value scaled by 1 / world: the SUM all-reduce gives it once
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
    from ctclip_mi355x.functional import MultiPosLossFn
    xt, xi, wt0, wi0 = _problem()
    prm = [wt0.clone().requires_grad_(True), wi0.clone().requires_grad_(True), torch.tensor(1.2, requires_grad=True)]
    loss, npos = MultiPosLossFn.apply(xt @ prm[0], xi @ prm[1], IDS, prm[2], loss_and_grads)
    (3.0 * loss).backward()
    ref_loss, _, _, ref_g = _single_process()
    assert torch.allclose(loss.detach(), ref_loss) and npos.item() == 2
    for p, r in zip(prm, ref_g):
        torch.testing.assert_close(p.grad, r, rtol=1e-5, atol=1e-6)
    with pytest.raises(ValueError, match='int64'):
        MultiPosLossFn.apply(xt @ prm[0], xi @ prm[1], IDS.int(), prm[2], loss_and_grads)
    with pytest.raises(ValueError, match='int64'):
        MultiPosLossFn.apply(xt @ prm[0], xi @ prm[1], IDS[:5], prm[2], loss_and_grads)


# ------------------------------------------------------------------------------ constructor
def _ctclip(**kw):
    from ctclip_mi355x.ct_clip import CTCLIP
    enc = torch.nn.Linear(4, 4)
    enc.dim = 4
    return CTCLIP(image_encoder=enc, text_encoder=torch.nn.Linear(4, 4), dim_text=4, dim_image=4, dim_latent=4, **kw)


def test_constructor_option_adds_no_parameter_and_no_key():
    """Fails on the parent commit: the keyword is swallowed by **kwargs there and the attribute is absent."""
    plain = _ctclip()
    assert plain.multi_positive is False and not hasattr(plain, 'last_positive_count')
    m = _ctclip(multi_positive=True)
    assert m.multi_positive is True and m.last_positive_count is None
    assert list(m.state_dict()) == list(plain.state_dict())
    assert [n for n, _ in m.named_parameters()] == [n for n, _ in plain.named_parameters()]
    assert [n for n, _ in m.named_buffers()] == [n for n, _ in plain.named_buffers()]
    assert m.temperature.item() == 1.0


@pytest.mark.parametrize('name', ['sigmoid_loss', 'decoupled_contrastive_learning', 'extra_latent_projection',
                                  'use_all_token_embeds'])
def test_refused_combinations_raise_by_name(name):
    with pytest.raises(NotImplementedError, match=f'multi_positive with {name}'):
        _ctclip(multi_positive=True, **{name: True})


def test_visual_ssl_head_is_refused_by_name():
    from ctclip_mi355x.visual_ssl import VisualSSLHead
    with pytest.raises(NotImplementedError, match='multi_positive with visual_ssl'):
        _ctclip(multi_positive=True, visual_ssl=VisualSSLHead(4))


def test_aug_image_is_refused_by_name():
    m = _ctclip(multi_positive=True)
    x = torch.zeros(2, 4)
    with pytest.raises(NotImplementedError, match='multi_positive with aug_image'):
        m(None, x, return_loss=True, aug_image=x)


def test_pair_ids_without_the_option_raise():
    x = torch.zeros(2, 4)
    with pytest.raises(ValueError, match='pair_ids without multi_positive'):
        _ctclip()(None, x, return_loss=True, pair_ids=torch.zeros(2, dtype=torch.int64))
    import inspect
    from ctclip_mi355x.ct_clip import CTCLIP
    assert list(inspect.signature(CTCLIP.forward).parameters)[-1] == 'pair_ids'      # placed last


# ------------------------------------------------------------------------------ C-ABI
def test_header_and_ctypes_table_declare_the_entry_points():
    from ctclip_mi355x import _lib
    h = open(os.path.join(REPO, 'include', 'ctclip_hip.h')).read()
    assert re.search(r'int ctclip_multipos_loss\(const ctclip_multipos_loss_args\* a, void\* stream\);', h)
    assert re.search(r'int64_t ctclip_multipos_loss_ws_bytes\(const ctclip_multipos_loss_args\* a\);', h)
    assert re.search(r'int ctclip_report_ids\(const int64_t\* input_ids, const int64_t\* attention_mask, int32_t B, '
                     r'int32_t L, int64_t\* out,\s*void\* stream\);', h)
    assert all(n in _lib._SIGS for n in ('ctclip_multipos_loss', 'ctclip_multipos_loss_ws_bytes', 'ctclip_report_ids'))
    assert len(_lib._SIGS['ctclip_report_ids']) == 6
    assert _lib._RESTYPES['ctclip_multipos_loss_ws_bytes'] is _lib.c_i64
    assert _lib.ABI_VERSION == 2
    assert re.search(r'#define CTCLIP_ABI_VERSION 2\b', h)
    # the struct mirrors the header field for field
    body = re.search(r'typedef struct \{([^}]*)\} ctclip_multipos_loss_args;', h).group(1)
    body = re.sub(r'/\*.*?\*/', '', body, flags=re.S)
    names = [n for decl in body.split(';') for n in re.findall(r'(\w+)\s*(?:,|$)', decl.replace('*', ' ').strip())]
    assert names == [f[0] for f in _lib.MultiposLossArgs._fields_], names
