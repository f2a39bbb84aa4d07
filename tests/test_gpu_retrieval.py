"""Retrieval evaluation on the GPU: ctclip_retrieval_ranks / ctclip_retrieval_topk (csrc/retrieval.hip),
their custom ops, RetrievalEvaluator and CTClipTrainer.validate_retrieval.

Reference: the float64 restatement of test_retrieval_cpu (the same normalisation, the header's rank
formula, a stable descending sort).

Exact-arithmetic inputs: rows of exactly 16 entries of +-1 have norm 4, normalised entries +-0.25 and
dot products that are multiples of 1/16 -- exact in f32 in any summation order -- so ranks, top-k
indices and top-k scores must EQUAL the reference, ties included (bit-identical gallery rows, a zero
row, a zero query).

Random inputs: an f32 fma chain over Dl products of unit vectors is within Dl 2^-24 of the exact dot
product (|partial sums| <= 1 by Cauchy-Schwarz, one rounding per step), rounding the two normalised
vectors moves it by at most Dl 2^-24 more to first order, and the two norm / division roundings by
8 2^-24: the bound (2 Dl + 8) 2^-24.  A rank can differ from the reference only for a query with some
score within that distance of its own; the test leaves out queries with a float64 gap below 1e-6 and
fails if they are more than 1 %."""
import types

import pytest
import torch

from oracle import ctclip_oracle as O
from oracle import weights as W
from test_retrieval_cpu import ref_ranks, ref_scores, ref_topk

pytestmark = pytest.mark.gpu


def _K():
    from ctclip_mi355x import kernels as K
    return K


# ------------------------------------------------------------------------------------ exact inputs
def _unit_rows(n, Dl, g):
    x = torch.zeros(n, Dl)
    for r in range(n):
        pos = torch.randperm(Dl, generator=g)[:16]
        x[r, pos] = torch.randint(0, 2, (16,), generator=g).float() * 2 - 1
    return x


def exact_case(N, M, Dl, seed=0):
    """q [N, Dl], g [M, Dl] with 16 entries of +-1 per row, pair [N] (not the identity).  Gallery rows
    0, M // 2 and M - 1 are bit-identical; row 1 is zero (M >= 4).  Query 0's positive is the lowest
    duplicate, query 1's the highest; query 2 is zero; queries 3, 4, 5 have their positives at gallery
    rows 63, 64 and M - 1 (M > 64).  Every other even query is its positive with i % 5 signs flipped
    (score 1 - (i % 5) / 8), the odd ones are unrelated rows."""
    gen = torch.Generator().manual_seed(seed)
    g = _unit_rows(M, Dl, gen)
    g[M // 2] = g[0]
    g[M - 1] = g[0]
    if M >= 4:
        g[1] = 0
    q = _unit_rows(N, Dl, gen)
    pair = torch.randint(0, M, (N,), generator=gen)
    fixed = {0: 0, 1: M - 1}
    if M > 64:
        fixed.update({3: 63, 4: 64, 5: M - 1})
    for i, p in fixed.items():
        if i < N:
            pair[i] = p
    for i in range(N):
        if i in fixed or i % 2 == 0:
            q[i] = g[pair[i]]
            if i not in fixed:
                nz = q[i].nonzero().flatten()[:i % 5]
                q[i, nz] = -q[i, nz]
    if N >= 3:
        q[2] = 0
    assert int(((q != 0).sum(1) % 16 != 0).sum()) == 0 and int(((g != 0).sum(1) % 16 != 0).sum()) == 0
    return q, g, pair.int()


def _ks(M):
    return sorted({1, min(5, M), min(M, 128)})


def _cross_check(rank, idx, pair, k):
    """Whenever rank_i < k, the rank-th entry of the top-k list is the positive: no tolerance."""
    rank, idx, pair = rank.cpu().long(), idx.cpu().long(), pair.cpu().long()
    rows = (rank < k).nonzero().flatten()
    assert torch.equal(idx[rows, rank[rows]], pair[rows])


# (1, 1, 16) ... (130, 257, 258): the issue's shapes; (6, 130, 32): positives on the tile edges with
# few rows; (70, 1100, 24): more column tiles than column chunks, so a workgroup walks several tiles
EXACT_SHAPES = [(1, 1, 16), (3, 2, 20), (63, 65, 64), (64, 64, 100), (65, 129, 127), (130, 257, 258), (6, 130, 32),
                (70, 1100, 24)]


@pytest.mark.parametrize('shape', EXACT_SHAPES)
def test_exact_inputs_equal_the_reference(shape):
    K = _K()
    N, M, Dl = shape
    q, g, pair = exact_case(N, M, Dl, seed=N + M)
    S = ref_scores(q, g)
    assert torch.equal(S * 16, (S * 16).round())                    # the construction is exact
    want = ref_ranks(S, pair)
    if M >= 3 and N >= 2:
        assert int(want[0]) == 0 and int(want[1]) == 2              # behind the two lower duplicates
    qd, gd, pd = q.cuda(), g.cuda(), pair.cuda()
    rank = K.retrieval_ranks(qd, gd, pd)
    assert rank.dtype == torch.int32 and rank.shape == (N,)
    assert torch.equal(rank.cpu(), want)
    assert torch.equal(K.retrieval_ranks(qd, gd, pd.long()).cpu(), want)
    if N == M:
        ident = torch.arange(N, dtype=torch.int32)
        assert torch.equal(K.retrieval_ranks(qd, gd).cpu(), ref_ranks(S, ident))
    for k in _ks(M):
        score, idx = K.retrieval_topk(qd, gd, k)
        assert score.shape == idx.shape == (N, k) and score.dtype == torch.float32 and idx.dtype == torch.int32
        rs, ri = ref_topk(S, k)
        assert torch.equal(idx.cpu(), ri)
        assert torch.equal(score.cpu().double(), rs)
        _cross_check(rank, idx, pair, k)
        s2, i2 = K.retrieval_topk(qd, gd, k)                        # bit reproducible
        assert torch.equal(s2, score) and torch.equal(i2, idx)
    assert torch.equal(K.retrieval_ranks(qd, gd, pd), rank)


# ----------------------------------------------------------------------------------- random inputs
# w: own score ~ w / sqrt(1 + c w^2) against a noise of 1 / sqrt(Dl) (c queries share a gallery row)
RANDOM_CASES = [((300, 300, 512), 0, 0.07), ((65, 130, 100), 1, 0.13), ((257, 64, 64), 2, 0.2)]


def random_case(shape, seed, w):
    N, M, Dl = shape
    gen = torch.Generator().manual_seed(seed)
    q = torch.randn(N, Dl, generator=gen)
    g = torch.randn(M, Dl, generator=gen)
    pair = torch.randperm(M, generator=gen)[:N] if N <= M else torch.randint(0, M, (N,), generator=gen)
    g.index_add_(0, pair, w * q)
    return q, g, pair.int()


@pytest.mark.parametrize('shape,seed,w', RANDOM_CASES)
def test_random_inputs(shape, seed, w):
    K = _K()
    N, M, Dl = shape
    q, g, pair = random_case(shape, seed, w)
    S = ref_scores(q, g)
    want = ref_ranks(S, pair)
    med = want.double().median().item()
    print(f'{shape}: reference median rank {med}, M / 4 = {M / 4}')
    assert 0 < med < M / 4
    qd, gd, pd = q.cuda(), g.cuda(), pair.cuda()
    rank = K.retrieval_ranks(qd, gd, pd)
    own = S.gather(1, pair.long()[:, None])
    gap = (S - own).abs()
    gap.scatter_(1, pair.long()[:, None], float('inf'))
    keep = gap.min(1).values >= 1e-6
    left_out = int((~keep).sum())
    wrong = int((rank.cpu()[keep] != want[keep]).sum())
    print(f'{shape}: {left_out} of {N} queries left out (gap < 1e-6), {wrong} disagreements outside them')
    assert left_out <= N // 100
    assert wrong == 0
    bound = (2 * Dl + 8) * 2.0 ** -24
    for k in _ks(M):
        score, idx = K.retrieval_topk(qd, gd, k)
        rs, ri = ref_topk(S, k)
        err = (score.cpu().double() - rs).abs().max().item()
        print(f'{shape} k = {k}: max |score - float64| {err:.3e}, bound {bound:.3e}')
        assert err <= bound
        v = torch.sort(S, dim=1, descending=True, stable=True).values
        clear = (v[:, k - 1] - v[:, k] > bound) if k < M else torch.ones(N, dtype=torch.bool)
        assert int(clear.sum()) > N // 2
        assert torch.equal(torch.sort(idx.cpu()[clear], dim=1).values, torch.sort(ri[clear], dim=1).values)
        _cross_check(rank, idx, pair, k)
        s2, i2 = K.retrieval_topk(qd, gd, k)
        assert torch.equal(s2, score) and torch.equal(i2, idx)
    assert torch.equal(K.retrieval_ranks(qd, gd, pd), rank)


# ---------------------------------------------------------------------------------------- refusals
def test_refusals():
    K = _K()
    from ctclip_mi355x._lib import KernelError
    q, g = torch.randn(6, 32, device='cuda'), torch.randn(9, 32, device='cuda')
    for k in (0, 10, 129):                                          # k = 0, k > M, k > 128
        with pytest.raises(KernelError, match='1003'):
            K.retrieval_topk(q, g, k)
    with pytest.raises(KernelError, match='1003'):
        K.retrieval_topk(q, torch.randn(200, 32, device='cuda'), 129)
    e = torch.empty(6, 0, device='cuda')
    with pytest.raises(KernelError, match='1003'):                  # Dl = 0
        K.retrieval_topk(e, e, 1)
    with pytest.raises(KernelError, match='1003'):
        K.retrieval_ranks(e, e)
    big = torch.zeros(65537, 4, device='cuda')
    with pytest.raises(KernelError, match='1003'):                  # N = 65,537
        K.retrieval_ranks(big, g[:, :4].contiguous(), torch.zeros(65537, dtype=torch.int32, device='cuda'))
    with pytest.raises(KernelError, match='1003'):
        K.retrieval_topk(big, g[:, :4].contiguous(), 1)
    with pytest.raises(KernelError, match='1003'):                  # M = 65,537
        K.retrieval_topk(g[:, :4].contiguous(), big, 1)
    with pytest.raises(ValueError):
        K.retrieval_ranks(q.half(), g.half(), torch.zeros(6, dtype=torch.int32, device='cuda'))
    with pytest.raises(ValueError):
        K.retrieval_topk(q.double(), g.double(), 1)
    with pytest.raises(ValueError):
        K.retrieval_topk(q.cpu(), g, 1)                             # a host tensor
    with pytest.raises(ValueError):
        K.retrieval_ranks(q, g.cpu(), torch.zeros(6, dtype=torch.int32, device='cuda'))
    for bad in (-1, 9):                                             # pair outside [0, M)
        pair = torch.zeros(6, dtype=torch.int32, device='cuda')
        pair[3] = bad
        with pytest.raises(ValueError, match=r'\[0, 9\)'):
            K.retrieval_ranks(q, g, pair)
    torch.cuda.synchronize()


# -------------------------------------------------------------------------------------- custom ops
def test_custom_ops():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from ctclip_mi355x import ops  # noqa: F401
    K = _K()
    q, g, pair = (x.cuda() for x in exact_case(20, 70, 40, seed=5))
    rank = torch.ops.ctclip.retrieval_ranks(q, g, pair)
    score, idx = torch.ops.ctclip.retrieval_topk(q, g, 7)
    assert torch.equal(rank, K.retrieval_ranks(q, g, pair))
    ks, ki = K.retrieval_topk(q, g, 7)
    assert torch.equal(score, ks) and torch.equal(idx, ki)
    utils = ('test_schema', 'test_faketensor', 'test_autograd_registration')
    torch.library.opcheck(torch.ops.ctclip.retrieval_ranks, (q, g, pair), test_utils=utils)
    torch.library.opcheck(torch.ops.ctclip.retrieval_ranks, (g, g, None), test_utils=utils)
    torch.library.opcheck(torch.ops.ctclip.retrieval_topk, (q, g, 7), test_utils=utils)
    with FakeTensorMode():
        fq, fg = torch.empty(300, 512, device='cuda'), torch.empty(1000, 512, device='cuda')
        fr = torch.ops.ctclip.retrieval_ranks(fq, fg, torch.empty(300, dtype=torch.int32, device='cuda'))
        assert fr.shape == (300,) and fr.dtype == torch.int32
        fs, fi = torch.ops.ctclip.retrieval_topk(fq, fg, 100)
        assert fs.shape == fi.shape == (300, 100) and fs.dtype == torch.float32 and fi.dtype == torch.int32
    assert not rank.requires_grad and not score.requires_grad


# --------------------------------------------------------------------------- evaluator and trainer
@pytest.fixture(scope='module')
def tiny():
    from test_gpu_model import build, cfg_small
    K = _K()
    torch.manual_seed(0)
    cfg = cfg_small()
    model = build(cfg)
    ids, mask = W.make_text(6, 32, cfg.bert.vocab_size, seed=7, ragged=True)
    text = types.SimpleNamespace(input_ids=ids.cuda(), attention_mask=mask.cuda())
    video = O.normalize_hu(W.make_hu(6, cfg.vit)).cuda()
    K.reset_ln_status()
    return cfg, model, text, video


def _consistent(d, ranks_ref, ks):
    from ctclip_mi355x.retrieval import mean_reciprocal_rank, median_rank, recall_at_k
    assert torch.equal(d['ranks'].cpu(), ranks_ref)
    assert torch.equal(d['recall'].cpu(), recall_at_k(ranks_ref, ks))
    for c, k in enumerate(ks):
        assert d['recall'][c].item() == int((ranks_ref < k).sum()) / ranks_ref.numel()
    assert d['median_rank'] == median_rank(ranks_ref) and d['mrr'] == mean_reciprocal_rank(ranks_ref)


def test_evaluator(tiny):
    from ctclip_mi355x.retrieval import RetrievalEvaluator
    cfg, model, text, video = tiny
    ks = (1, 2, 5, 10)
    ev = RetrievalEvaluator(model)
    res = ev.evaluate(video, text, ks=ks, n_boot=20, topk=3, batch_size=4)
    t, v = res['text_latents'], res['image_latents']
    assert t.shape == v.shape == (6, cfg.dim_latent)
    ident = torch.arange(6)
    _consistent(res['report_to_volume'], ref_ranks(ref_scores(t, v), ident), ks)
    _consistent(res['volume_to_report'], ref_ranks(ref_scores(v, t), ident), ks)
    for name in ('report_to_volume', 'volume_to_report'):
        d = res[name]
        assert d['ci'].shape == (3, len(ks)) and d['ci'].dtype == torch.float64
        assert d['idx'].shape == d['score'].shape == (6, 3)
        _cross_check(d['ranks'], d['idx'], ident, 3)
    # several reports per volume: reports 0..5 belong to volumes 0, 0, 1, 3, 3, 3 (2, 4, 5 have none)
    pair = torch.tensor([0, 0, 1, 3, 3, 3])
    res2 = ev.evaluate([video[:4], video[4:]], text, pair=pair, ks=ks, batch_size=4)
    assert torch.equal(res2['image_latents'], v) and res2['report_to_volume']['ci'] is None
    assert 'idx' not in res2['report_to_volume']
    _consistent(res2['report_to_volume'], ref_ranks(ref_scores(t, v), pair), ks)
    Sv = ref_scores(v, t)
    best = torch.full((6,), -1, dtype=torch.int32)
    for vol in (0, 1, 3):
        best[vol] = min(int(ref_ranks(Sv[vol:vol + 1], [r])) for r in range(6) if int(pair[r]) == vol)
    assert torch.equal(res2['volume_to_report']['ranks'].cpu(), best)
    from ctclip_mi355x.retrieval import recall_at_k
    assert torch.equal(res2['volume_to_report']['recall'].cpu(), recall_at_k(best[best >= 0], ks))


def test_validate_retrieval_keeps_the_training_state(tiny):
    K = _K()
    from ctclip_mi355x.trainer import CTClipTrainer, EvalGuardError
    cfg, model, text, video = tiny
    two = types.SimpleNamespace(input_ids=text.input_ids[:2], attention_mask=text.attention_mask[:2])
    K.reset_ln_status()
    model.train()
    tr = CTClipTrainer(model, lr=1e-3)
    tr.train_step(two, video[:2])
    tr.flush()
    word = K.status_word(video.device)
    snap = word.clone()
    codebook = model.visual_transformer.vq._codebook.embed.clone()
    assert model.training
    res = tr.validate_retrieval(video, text, ks=(1, 5), n_boot=4, batch_size=3)
    assert model.training and torch.equal(word, snap)
    assert torch.equal(model.visual_transformer.vq._codebook.embed, codebook)      # no EMA from the pass
    ident = torch.arange(6)
    assert torch.equal(res['report_to_volume']['ranks'].cpu(),
                       ref_ranks(ref_scores(res['text_latents'], res['image_latents']), ident))
    assert res['volume_to_report']['ci'].shape == (3, 2)
    bad = video.clone()
    bad[1, 0, 17, 33, 71] = float('nan')
    with pytest.raises(EvalGuardError) as ei:
        tr.validate_retrieval(bad, text)
    assert ei.value.bits != 0 and model.training and torch.equal(word, snap)
    before = tr.flat.data.clone()
    loss = tr.train_step(two, video[:2])
    tr.check()
    assert torch.isfinite(loss) and not torch.equal(before, tr.flat.data)
    model.eval()
    tr.validate_retrieval(video[:2], two)
    assert not model.training
    model.train()
