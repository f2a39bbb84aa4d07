"""Host side of the retrieval evaluation (ctclip_mi355x/retrieval.py): Recall@K, median rank, MRR and
the bootstrap table on hand-made rank vectors with known answers, and the refusals the wrappers raise
before the library is touched.

``ref_ranks`` / ``ref_topk`` restate the two kernels in float64 torch (the same normalisation, the rank
formula of include/ctclip_hip.h, a stable descending sort); the GPU tests compare against them."""
import numpy as np
import pytest
import torch


def ref_scores(q, g):
    """float64 cosine scores [N, M]: x / max(|x|, 1e-12) per row (a zero row stays zero), q^ g^T."""
    q, g = q.detach().cpu().double(), g.detach().cpu().double()
    qn = q / q.norm(dim=1, keepdim=True).clamp_min(1e-12)
    gn = g / g.norm(dim=1, keepdim=True).clamp_min(1e-12)
    return qn @ gn.t()


def ref_ranks(S, pair):
    """rank_i = #{ j != pair_i : S_ij > S_i,pair_i or (S_ij == S_i,pair_i and j < pair_i) }."""
    pair = torch.as_tensor(pair).long().cpu()
    own = S.gather(1, pair[:, None])
    j = torch.arange(S.shape[1])[None, :]
    above = (S > own) | ((S == own) & (j < pair[:, None]))
    return (above & (j != pair[:, None])).sum(1).int()


def ref_topk(S, k):
    """(score, idx) [N, k]: descending score, ties by ascending index (a stable descending sort)."""
    v, i = torch.sort(S, dim=1, descending=True, stable=True)
    return v[:, :k], i[:, :k].int()


def test_reference_rank_is_the_place_in_a_stable_sort():
    g = torch.Generator().manual_seed(0)
    S = torch.randint(0, 4, (7, 9), generator=g).double()          # many ties
    pair = torch.tensor([0, 8, 3, 3, 5, 1, 7])
    order = torch.sort(S, dim=1, descending=True, stable=True).indices
    place = (order == pair[:, None]).int().argmax(1).int()
    assert torch.equal(ref_ranks(S, pair), place)


def test_recall_at_k():
    from ctclip_mi355x.retrieval import recall_at_k
    ranks = torch.tensor([0, 0, 1, 4, 4, 5, 9, 49, 99, 100], dtype=torch.int32)
    got = recall_at_k(ranks)                                        # K = 1, 5, 10, 50, 100
    assert got.dtype == torch.float64
    assert got.tolist() == [0.2, 0.5, 0.7, 0.8, 0.9]
    assert recall_at_k(ranks, ks=(1000,)).tolist() == [1.0]         # K beyond every rank
    assert recall_at_k(ranks, ks=(5, 6, 101)).tolist() == [0.5, 0.6, 1.0]
    assert recall_at_k(ranks, ks=()).shape == (0,)
    assert recall_at_k(ranks.numpy(), ks=[1]).tolist() == [0.2]     # anything as_tensor takes
    assert recall_at_k(torch.tensor([3]), ks=(3, 4)).tolist() == [0.0, 1.0]
    with pytest.raises(ValueError):
        recall_at_k(torch.zeros(0, dtype=torch.int32))
    with pytest.raises(ValueError):
        recall_at_k(torch.zeros(3))                                  # floating ranks
    with pytest.raises(ValueError):
        recall_at_k(torch.zeros(2, 2, dtype=torch.int32))


def test_median_rank_and_mrr():
    from ctclip_mi355x.retrieval import mean_reciprocal_rank, median_rank
    assert median_rank(torch.tensor([4, 0, 2])) == 3.0               # 1-based: 1, 3, 5
    assert median_rank(torch.tensor([0, 1, 2, 9])) == 2.5            # the two middle ones: 2, 3
    assert median_rank(torch.tensor([7])) == 8.0
    assert median_rank(torch.tensor([0, 0, 0, 0])) == 1.0
    assert mean_reciprocal_rank(torch.tensor([0, 1, 3])) == pytest.approx((1 + 0.5 + 0.25) / 3, abs=1e-15)
    assert mean_reciprocal_rank(torch.tensor([0, 0])) == 1.0


def test_bootstrap_recall_applies_the_reference_resamples():
    from ctclip_mi355x.evaluate import bootstrap_indices, compute_cis
    from ctclip_mi355x.retrieval import bootstrap_recall, recall_at_k
    g = torch.Generator().manual_seed(3)
    ranks = torch.randint(0, 40, (23,), generator=g, dtype=torch.int32)
    ks = (1, 5, 10, 64)
    S = 12
    table = bootstrap_recall(ranks, ks, S)
    assert table.shape == (S, len(ks)) and table.dtype == torch.float64
    rows = bootstrap_indices(23, S)
    for s in range(S):
        drawn = ranks.numpy()[rows[s]]
        for c, k in enumerate(ks):
            assert table[s, c].item() == np.mean(drawn < k)
        assert torch.equal(table[s], recall_at_k(torch.from_numpy(drawn), ks))
    assert bool((table[:, 3] == 1.0).all())                          # K beyond every rank
    ci = compute_cis(table)
    assert ci.shape == (3, len(ks))
    assert np.array_equal(ci[0].numpy(), np.round(table.numpy().mean(0), 4))
    assert bootstrap_recall(ranks, (), 4).shape == (4, 0)


def test_wrappers_refuse_before_the_library():
    from ctclip_mi355x import kernels as K
    q, g = torch.zeros(5, 8), torch.zeros(4, 8)
    with pytest.raises(ValueError, match='pair=None'):
        K.retrieval_ranks(q, g)                                      # N != M without pairs
    with pytest.raises(ValueError, match=r'\[N, Dl\]'):
        K.retrieval_ranks(q, torch.zeros(4, 9), torch.zeros(5, dtype=torch.int32))
    with pytest.raises(ValueError, match=r'\[N, Dl\]'):
        K.retrieval_ranks(torch.zeros(5), g, torch.zeros(5, dtype=torch.int32))
    with pytest.raises(ValueError, match='pair must be'):
        K.retrieval_ranks(q, g, torch.zeros(4, dtype=torch.int32))   # one entry per query
    with pytest.raises(ValueError, match='pair must be'):
        K.retrieval_ranks(q, g, torch.zeros(5))                      # floating indices
    with pytest.raises(ValueError, match='device tensor'):
        K.retrieval_ranks(q, g, torch.zeros(5, dtype=torch.int32))   # host tensors
    with pytest.raises(ValueError, match=r'\[N, Dl\]'):
        K.retrieval_topk(q, torch.zeros(4, 9), 2)
    with pytest.raises(ValueError, match=r'\[N, Dl\]'):
        K.retrieval_topk(q, torch.zeros(4, 8, 1), 2)
    with pytest.raises(ValueError, match='device tensor'):
        K.retrieval_topk(q, g, 2)


def test_evaluator_needs_pairs_when_counts_differ():
    from ctclip_mi355x.retrieval import RetrievalEvaluator
    ev = RetrievalEvaluator(model=None)
    ev.text_latents = lambda text, batch_size=8: torch.zeros(5, 8)
    ev.image_latents = lambda volumes, batch_size=8: torch.zeros(4, 8)
    with pytest.raises(ValueError, match='pair=None'):
        ev.evaluate(None, None)
