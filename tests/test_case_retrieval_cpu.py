"""Host side of the case retrieval evaluation: the float64 restatement of ctclip_case_retrieval
(case_retrieval_common.py) on hand-worked cases -- it defines what the GPU tests call right --, and
``retrieval.pack_labels`` / ``map_at_k`` / ``precision_at_k`` / ``mean_jaccard_at_k`` / ``bootstrap_case`` and
the refusals ``kernels.case_retrieval`` raises before the library is touched."""
import types

import numpy as np
import pytest
import torch

import case_retrieval_common as C


def _lab(*words):
    return torch.tensor(words, dtype=torch.int64)


# one query along e0 and a gallery whose scores fall in the order 0, 1, 2, 3 (cosines 0.995, 0.707, 0.0995, -1)
Q4 = torch.tensor([[1.0, 0.0]])
G4 = torch.tensor([[1.0, 0.1], [1.0, 1.0], [0.1, 1.0], [-1.0, 0.0]])


def test_four_row_gallery_worked_by_hand():
    """Query labels {0, 1} = 0b011; the gallery in list order has 0b100, 0b001, 0b011, 0b010.

    any:  relevant by place 0 1 1 1, R = 3; h_r at the relevant places 2, 3, 4 is 1, 2, 3, so
          AP@1 = 0 / 1, AP@2 = (1/2) / 2, AP@3 = (1/2 + 2/3) / 3, AP@4 = (1/2 + 2/3 + 3/4) / 3;
          hits 0 1 2 3.
    exact: only place 3 (0b011) is relevant, R = 1: AP@1 = AP@2 = 0, AP@3 = AP@4 = (1/3) / min(K, 1) = 1/3;
          hits 0 0 1 1.
    Jaccard by place: 0/3, 1/2, 2/2, 1/2 -> gain 0, 0.5, 1.5, 2.0 in both modes."""
    ks = (1, 2, 3, 4)
    qlab, glab = _lab(0b011), _lab(0b100, 0b001, 0b011, 0b010)
    r = C.reference(Q4, G4, qlab, glab, ks=ks, rel='any')
    assert r.idx.tolist() == [[0, 1, 2, 3]] and r.filled.tolist() == [4] and r.nrel.tolist() == [3]
    assert r.hits.tolist() == [[0, 1, 2, 3]]
    assert r.ap.tolist() == [[0.0, (1 / 2) / 2, (1 / 2 + 2 / 3) / 3, (1 / 2 + 2 / 3 + 3 / 4) / 3]]
    assert r.gain.tolist() == [[0.0, 0.5, 1.5, 2.0]]
    e = C.reference(Q4, G4, qlab, glab, ks=ks, rel='exact')
    assert e.nrel.tolist() == [1] and e.hits.tolist() == [[0, 0, 1, 1]]
    assert e.ap.tolist() == [[0.0, 0.0, 1 / 3, 1 / 3]]
    assert e.gain.tolist() == [[0.0, 0.5, 1.5, 2.0]]
    assert torch.equal(r.idx, e.idx)                                 # the mode changes no list


def test_exclusion_and_ties():
    """Groups: query group 7 hides gallery rows 0 and 2 (R and the list are taken over rows 1, 3 only); a
    negative query group hides nothing.  Bit-equal gallery rows tie and keep the ascending index."""
    glab = _lab(0b100, 0b001, 0b011, 0b010)
    qgrp, ggrp = torch.tensor([7], dtype=torch.int32), torch.tensor([7, 1, 7, 2], dtype=torch.int32)
    r = C.reference(Q4, G4, _lab(0b011), glab, qgrp, ggrp, ks=(1, 3), rel='any')
    assert r.idx.tolist() == [[1, 3, -1]] and r.score[0, 2].item() == 0.0
    assert r.filled.tolist() == [2] and r.nrel.tolist() == [2]
    assert r.hits.tolist() == [[1, 2]] and r.ap.tolist() == [[1.0, (1.0 + 1.0) / 2]]
    assert r.gain.tolist() == [[0.5, 1.0]]
    free = C.reference(Q4, G4, _lab(0b011), glab, torch.tensor([-1], dtype=torch.int32), ggrp, ks=(1, 3))
    assert free.idx.tolist() == [[0, 1, 2]] and free.nrel.tolist() == [3]
    whole = C.reference(Q4, G4, _lab(0b011), glab, qgrp, torch.full((4,), 7, dtype=torch.int32), ks=(1, 3))
    assert whole.filled.tolist() == [0] and whole.idx.tolist() == [[-1, -1, -1]]
    assert whole.ap.tolist() == [[-1.0, -1.0]] and whole.gain.tolist() == [[0.0, 0.0]]
    g = torch.stack([G4[1], G4[0], G4[1], G4[1]])
    tie = C.reference(Q4, g, _lab(1), _lab(1, 1, 1, 1), ks=(4,))
    assert tie.idx.tolist() == [[1, 0, 2, 3]]


def test_no_relevant_row_small_gallery_and_empty_label_sets():
    glab = _lab(0b100, 0b100, 0, 0b1000)
    r = C.reference(Q4, G4, _lab(0b011), glab, ks=(1, 5, 10))         # R = 0; the gallery is smaller than K
    assert r.nrel.tolist() == [0] and r.filled.tolist() == [4]
    assert r.ap.tolist() == [[-1.0, -1.0, -1.0]] and r.hits.tolist() == [[0, 0, 0]]
    assert r.idx.tolist() == [[0, 1, 2, 3] + [-1] * 6] and r.score[0, 4:].abs().sum().item() == 0.0
    assert r.gain.tolist() == [[0.0, 0.0, 0.0]]
    # a query without labels: under 'any' (and 'exact') exactly the rows without labels are relevant, J = 1 there
    for rel in ('any', 'exact'):
        e = C.reference(Q4, G4, _lab(0), glab, ks=(1, 5, 10), rel=rel)
        assert e.nrel.tolist() == [1] and e.hits.tolist() == [[0, 1, 1]]
        assert e.ap.tolist() == [[0.0, (1 / 3) / 1, (1 / 3) / 1]]        # the one relevant row is at place 3
        assert e.gain.tolist() == [[0.0, 1.0, 1.0]]


def test_all_64_bits_and_exact_versus_any():
    assert C.popcount(-1) == 64 and C.jaccard(-1, -1) == 1.0 and C.jaccard(-1, 1) == 1 / 64
    assert C.jaccard(-1, 0) == 0.0 and C.jaccard(1 << 63, -1) == 1 / 64 and C.jaccard(0, 0) == 1.0
    assert C.relevant(-1, 1 << 63, 'any') and not C.relevant(-1, 1 << 63, 'exact') and C.relevant(-1, -1, 'exact')
    assert C.relevant(0, 0, 'any') and not C.relevant(0, 1, 'any') and not C.relevant(0b01, 0b10, 'any')
    glab = _lab(-1, -(1 << 63), 0b1, 0)                              # all 64 bits, bit 63 alone, bit 0, none
    a = C.reference(Q4, G4, _lab(-1), glab, ks=(2, 4), rel='any')
    assert a.nrel.tolist() == [3] and a.hits.tolist() == [[2, 3]]
    assert a.ap.tolist() == [[(1.0 + 1.0) / 2, (1.0 + 1.0 + 1.0) / 3]]
    assert a.gain.tolist() == [[1.0 + 1 / 64, 1.0 + 1 / 64 + 1 / 64 + 0.0]]
    e = C.reference(Q4, G4, _lab(-1), glab, ks=(2, 4), rel='exact')
    assert e.nrel.tolist() == [1] and e.hits.tolist() == [[1, 1]] and e.ap.tolist() == [[1.0, 1.0]]
    assert torch.equal(e.gain, a.gain)


def test_metrics_on_lists_takes_any_list():
    """The restatement applied to a list that is not the reference's (the GPU tests apply it to the kernel's)."""
    hits, ap, gain = C.metrics_on_lists([[3, 0, -1]], _lab(0b011), _lab(0b100, 0b001, 0b011, 0b010), [3], (1, 2, 3),
                                        'any')
    assert hits.tolist() == [[1, 1, 1]] and ap.tolist() == [[1.0, 0.5, 1 / 3]] and gain.tolist() == [[0.5, 0.5, 0.5]]


# -------------------------------------------------------------------------------------- pack_labels
def test_pack_labels():
    from ctclip_mi355x.retrieval import pack_labels
    y = torch.tensor([[1, 0, 1], [0, 0, 0], [0, 1, 0]])
    for t in (y, y.bool(), y.float(), y.double(), y.to(torch.uint8), y.int(), y.numpy()):
        got = pack_labels(t)
        assert got.dtype == torch.int64 and got.tolist() == [0b101, 0, 0b010]
    full = torch.ones(2, 64, dtype=torch.int8)
    full[1, 63] = 0
    assert pack_labels(full).tolist() == [-1, (1 << 63) - 1]
    only63 = torch.zeros(1, 64)
    only63[0, 63] = 1
    assert pack_labels(only63).tolist() == [-(1 << 63)]
    gen = torch.Generator().manual_seed(0)
    r = torch.randint(0, 2, (40, 18), generator=gen)
    words = pack_labels(r)
    assert torch.equal((words[:, None] >> torch.arange(18)[None, :]) & 1, r)       # round trip
    assert pack_labels(torch.zeros(0, 5)).shape == (0,) and pack_labels(torch.zeros(3, 0)).tolist() == [0, 0, 0]
    for bad in (torch.tensor([[0, 2]]), torch.tensor([[0.5, 1.0]]), torch.tensor([[-1, 0]]),
                torch.tensor([[float('nan'), 0.0]])):
        with pytest.raises(ValueError, match='0 or 1'):
            pack_labels(bad)
    with pytest.raises(ValueError, match='C <= 64'):
        pack_labels(torch.zeros(2, 65))
    with pytest.raises(ValueError, match=r'\[N, C\]'):
        pack_labels(torch.zeros(5))


# ----------------------------------------------------------------------------------- metric helpers
def test_metric_helpers_on_hand_made_outputs():
    from ctclip_mi355x.retrieval import map_at_k, mean_jaccard_at_k, precision_at_k
    ks = (1, 5)
    ap = torch.tensor([[1.0, 0.5], [-1.0, -1.0], [0.0, 0.25], [-1.0, -1.0], [1.0, 0.75]], dtype=torch.float64)
    m, n = map_at_k(ap)
    assert n == 3 and m.dtype == torch.float64 and m.tolist() == [2.0 / 3, 1.5 / 3]
    m0, n0 = map_at_k(ap[[1, 3]])
    assert n0 == 0 and bool(torch.isnan(m0).all()) and m0.shape == (2,)
    hits = torch.tensor([[1, 3], [0, 0], [0, 2], [1, 1], [1, 4]], dtype=torch.int32)
    filled = torch.tensor([5, 0, 5, 2, 5], dtype=torch.int32)        # places up to K: 1 0 1 1 1 / 5 0 5 2 5
    p = precision_at_k(hits, filled, ks)
    assert p.dtype == torch.float64 and p.tolist() == [3 / 4, 10 / 17]
    gain = torch.tensor([[1.0, 2.5], [0.0, 0.0], [0.25, 1.0], [0.5, 0.5], [1.0, 4.5]], dtype=torch.float64)
    j = mean_jaccard_at_k(gain, filled, ks)
    assert j.tolist() == [2.75 / 4, 8.5 / 17]
    assert bool(torch.isnan(precision_at_k(hits[1:2], filled[1:2], ks)).all())     # no list has a place
    with pytest.raises(ValueError):
        map_at_k(torch.zeros(0, 2, dtype=torch.float64))
    with pytest.raises(ValueError):
        map_at_k(hits)                                               # an integer table
    with pytest.raises(ValueError):
        precision_at_k(gain, filled, ks)                             # a floating table
    with pytest.raises(ValueError):
        precision_at_k(hits, filled[:4], ks)


def test_bootstrap_case_applies_the_reference_resamples():
    from ctclip_mi355x.evaluate import bootstrap_indices, compute_cis
    from ctclip_mi355x.retrieval import bootstrap_case, map_at_k, mean_jaccard_at_k, precision_at_k
    gen = torch.Generator().manual_seed(4)
    N, ks, S = 19, (1, 5, 10), 9
    ap = torch.rand(N, 3, generator=gen, dtype=torch.float64)
    ap[[2, 7, 11]] = -1.0
    filled = torch.randint(0, 11, (N,), generator=gen, dtype=torch.int32)
    places = torch.minimum(filled.long()[:, None], torch.tensor(ks)[None, :])
    hits = (torch.rand(N, 3, generator=gen) * (places + 1)).long().clamp(max=places).int()
    gain = torch.rand(N, 3, generator=gen, dtype=torch.float64) * places
    rows = bootstrap_indices(N, S)
    t_ap, t_hits, t_gain = bootstrap_case(ap, S), bootstrap_case(hits, S, places), bootstrap_case(gain, S, places)
    for t in (t_ap, t_hits, t_gain):
        assert t.shape == (S, 3) and t.dtype == torch.float64
    for s in range(S):
        drawn = torch.from_numpy(rows[s]).long()
        want, n = map_at_k(ap[drawn])
        assert n == int((ap[drawn, 0] != -1).sum())
        np.testing.assert_allclose(t_ap[s].numpy(), want.numpy(), rtol=1e-14, atol=0)
        kept = ap[drawn][ap[drawn, 0] != -1]
        np.testing.assert_allclose(t_ap[s].numpy(), kept.numpy().mean(0), rtol=1e-14, atol=0)
        assert torch.equal(t_hits[s], precision_at_k(hits[drawn], filled[drawn], ks))
        np.testing.assert_allclose(t_gain[s].numpy(), mean_jaccard_at_k(gain[drawn], filled[drawn], ks).numpy(),
                                   rtol=1e-14, atol=0)
    assert compute_cis(t_ap).shape == (3, 3)
    none = bootstrap_case(torch.full((4, 2), -1.0, dtype=torch.float64), 3)
    assert none.shape == (3, 2) and bool(torch.isnan(none).all())
    with pytest.raises(ValueError):
        bootstrap_case(hits, S, places[:, :2])


# ---------------------------------------------------------------------------------------- refusals
def test_wrapper_refuses_before_the_library(monkeypatch):
    from ctclip_mi355x import _lib
    from ctclip_mi355x import kernels as K

    def touched():
        raise AssertionError('the library was touched')
    monkeypatch.setattr(_lib, 'lib', touched)
    q, g = torch.zeros(5, 8), torch.zeros(4, 8)
    ql, gl = torch.zeros(5, dtype=torch.int64), torch.zeros(4, dtype=torch.int64)
    qg, gg = torch.zeros(5, dtype=torch.int32), torch.zeros(4, dtype=torch.int32)

    def refused(match, *a, **kw):
        with pytest.raises(ValueError, match=match):
            K.case_retrieval(*a, **kw)
    refused(r'\[N, Dl\]', q, torch.zeros(4, 9), ql, gl)                # shapes
    refused(r'\[N, Dl\]', torch.zeros(5), g, ql, gl)
    refused(r'\[N, Dl\]', torch.zeros(0, 8), g, ql[:0], gl)
    refused('float32', q.double(), g.double(), ql, gl)               # dtype
    refused('float32', q, g.half(), ql, gl)
    refused('qlab', q, g, ql.int(), gl)
    refused('glab', q, g, ql, gl[:3])
    refused('glab', q, g, ql, torch.zeros(4, 18, dtype=torch.int64))
    refused('come together', q, g, ql, gl, qg, None)                 # one group vector without the other
    refused('come together', q, g, ql, gl, None, gg)
    refused('qgrp', q, g, ql, gl, qg.long(), gg)
    refused('ggrp', q, g, ql, gl, qg, gg[:2])
    for ks in ((), (0, 5), (5, 5), (5, 1), (1, 129), tuple(range(1, 10)), 5):      # ks
        refused('ks must be', q, g, ql, gl, ks=ks)
    refused('K above 128', q, g, ql, gl, ks=(1, 200))
    refused("'any' or 'exact'", q, g, ql, gl, rel='jaccard')          # rel
    refused('nDCG', q, g, ql, gl, rel='ndcg')
    refused('queries must be contiguous', torch.zeros(8, 5).t(), g, ql, gl)        # contiguity
    refused('glab must be contiguous', q, g, ql, torch.zeros(8, dtype=torch.int64)[::2])
    refused('device tensor', q, g, ql, gl)                           # host tensors
    refused('device tensor', q, g, ql, gl, qg, gg, ks=(1, 2), rel='exact')


def test_evaluator_refusals():
    from ctclip_mi355x.retrieval import CaseRetrievalEvaluator
    with pytest.raises(NotImplementedError, match='CaseRetrievalEvaluator with CTCLIP\\(use_all_token_embeds=True\\)'):
        CaseRetrievalEvaluator(types.SimpleNamespace(use_all_token_embeds=True))
    ev = CaseRetrievalEvaluator(model=None)
    ev.image_latents = lambda volumes, batch_size=8: torch.zeros(5 if volumes == 'q' else 4, 8)
    y5, y4 = torch.zeros(5, 3), torch.zeros(4, 3)
    with pytest.raises(ValueError, match='without gallery_volumes'):
        ev.evaluate('q', y5, gallery_labels=y4)
    with pytest.raises(ValueError, match='without gallery_volumes'):
        ev.evaluate('q', y5, gallery_groups=torch.arange(4))
    with pytest.raises(ValueError, match='needs gallery_labels'):
        ev.evaluate('q', y5, gallery_volumes='g')
    with pytest.raises(ValueError, match='come together'):
        ev.evaluate('q', y5, groups=torch.arange(5), gallery_volumes='g', gallery_labels=y4)
    with pytest.raises(ValueError, match='labels must be'):
        ev.evaluate('q', y4)                                         # four label rows for five volumes
    with pytest.raises(ValueError, match='0 or 1'):
        ev.evaluate('q', y5 + 2)
    with pytest.raises(ValueError, match='groups must be'):
        ev.evaluate('q', y5, groups=torch.zeros(5))
    with pytest.raises(ValueError, match='device tensor'):           # everything passed on: the wrapper's refusal
        ev.evaluate('q', y5, gallery_volumes='g', gallery_labels=y4, groups=torch.arange(5),
                    gallery_groups=torch.arange(4))
