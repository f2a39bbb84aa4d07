"""The float64 restatement of ctclip_case_retrieval (include/ctclip_hip.h has the definitions) and the
exact-arithmetic input builder; test_case_retrieval_cpu.py checks the restatement on hand-worked cases,
test_gpu_case_retrieval.py compares the kernel against it.

Scores are ``test_retrieval_cpu.ref_scores`` (float64, the kernel's normalisation); excluded columns are
masked, the list is a stable descending sort, and hits / ap / gain follow the header's formulas in the stated
order, in Python floats (IEEE doubles: one correctly rounded operation per step, as the kernel's f64)."""
import types

import numpy as np
import torch

from test_retrieval_cpu import ref_scores

MASK64 = (1 << 64) - 1


def _word(x):
    return int(x) & MASK64


def popcount(x):
    return bin(_word(x)).count('1')


def relevant(a, b, rel):
    a, b = _word(a), _word(b)
    if rel == 'exact':
        return a == b
    assert rel == 'any'
    return (a & b) != 0 or (a == 0 and b == 0)


def jaccard(a, b):
    a, b = _word(a), _word(b)
    return 1.0 if (a | b) == 0 else popcount(a & b) / popcount(a | b)


def visible_mask(N, M, qgrp, ggrp):
    """[N, M] bool: row j is invisible to query i iff groups are given, qgrp[i] >= 0 and ggrp[j] == qgrp[i]."""
    if qgrp is None:
        assert ggrp is None
        return torch.ones(N, M, dtype=torch.bool)
    qg, gg = torch.as_tensor(qgrp).long().cpu(), torch.as_tensor(ggrp).long().cpu()
    return ~((qg[:, None] >= 0) & (gg[None, :] == qg[:, None]))


def ref_lists(S, visible, kmax):
    """(idx [N, kmax] int32, score [N, kmax] f64, filled [N] int32, order [N, M], sorted scores [N, M]): the
    first min(kmax, visible_i) visible rows by descending score, ties by ascending index; -1 / 0 behind."""
    N, M = S.shape
    Sm = S.clone()
    Sm[~visible] = -float('inf')                                     # every real score is >= -1
    v, order = torch.sort(Sm, dim=1, descending=True, stable=True)
    filled = visible.sum(1).clamp(max=kmax).int()
    idx = torch.full((N, kmax), -1, dtype=torch.int32)
    score = torch.zeros(N, kmax, dtype=torch.float64)
    c = min(M, kmax)
    idx[:, :c], score[:, :c] = order[:, :c].int(), v[:, :c]
    behind = torch.arange(kmax)[None, :] >= filled[:, None]
    idx[behind], score[behind] = -1, 0.0
    return idx, score, filled, order, v


def ref_nrel(qlab, glab, visible, rel):
    """[N] int32: the relevant rows among all visible gallery rows (``relevant``, on whole int64 tensors)."""
    a, b = torch.as_tensor(qlab).long().cpu()[:, None], torch.as_tensor(glab).long().cpu()[None, :]
    r = (a == b) if rel == 'exact' else (((a & b) != 0) | ((a == 0) & (b == 0)))
    assert rel in ('any', 'exact')
    return (r & visible).sum(1).int()


def metrics_on_lists(idx, qlab, glab, nrel, ks, rel):
    """(hits [N, nK] int32, ap [N, nK] f64, gain [N, nK] f64) of the lists ``idx`` (-1 = unfilled), with
    m = min(K, n_i), h_r the relevant among the first r:
    ap = (sum_{r <= m, rel_r} h_r / r) / min(K, R_i) in ascending r, -1 when R_i == 0 or n_i == 0;
    gain = sum_{r <= m} J_r in ascending r."""
    idx = torch.as_tensor(idx).cpu().tolist()
    qlab, glab = [int(x) for x in qlab], [int(x) for x in glab]
    nrel = [int(x) for x in nrel]
    N, nK = len(idx), len(ks)
    hits = np.zeros((N, nK), dtype=np.int32)
    ap = np.zeros((N, nK), dtype=np.float64)
    gain = np.zeros((N, nK), dtype=np.float64)
    for i in range(N):
        row = [j for j in idx[i] if j >= 0]
        assert row == idx[i][:len(row)]                              # unfilled places only at the end
        n, R = len(row), nrel[i]
        for c, k in enumerate(ks):
            h, s, gsum = 0, 0.0, 0.0
            for r in range(1, min(k, n) + 1):
                b = glab[row[r - 1]]
                if relevant(qlab[i], b, rel):
                    h += 1
                    s += float(h) / float(r)
                gsum += jaccard(qlab[i], b)
            hits[i, c], gain[i, c] = h, gsum
            ap[i, c] = -1.0 if (R == 0 or n == 0) else s / float(min(k, R))
    return torch.from_numpy(hits), torch.from_numpy(ap), torch.from_numpy(gain)


def reference(q, g, qlab, glab, qgrp=None, ggrp=None, ks=(1, 5, 10, 50), rel='any'):
    """Every output of the kernel in float64, plus ``S`` (the scores), ``visible`` and ``sorted`` (each
    query's visible scores in list order, -inf behind them)."""
    S = ref_scores(q, g)
    vis = visible_mask(S.shape[0], S.shape[1], qgrp, ggrp)
    idx, score, filled, _, v = ref_lists(S, vis, ks[-1])
    nrel = ref_nrel(qlab, glab, vis, rel)
    hits, ap, gain = metrics_on_lists(idx, qlab, glab, nrel, ks, rel)
    return types.SimpleNamespace(idx=idx, score=score, filled=filled, nrel=nrel, hits=hits, ap=ap, gain=gain, S=S,
                                 visible=vis, sorted=v)


# ------------------------------------------------------------------------------------ exact inputs
def _unit_rows(n, Dl, gen):
    x = torch.zeros(n, Dl)
    for r in range(n):
        pos = torch.randperm(Dl, generator=gen)[:16]
        x[r, pos] = torch.randint(0, 2, (16,), generator=gen).float() * 2 - 1
    return x


def random_labels(n, gen, bits=18, p=0.12):
    """[n] int64 bitmasks over ``bits`` labels, each present with probability p."""
    y = (torch.rand(n, bits, generator=gen) < p).long()
    return (y << torch.arange(bits)[None, :]).sum(1)


def exact_case(N, M, Dl, seed=0, groups='none'):
    """Inputs whose scores are exact in f32 in any summation order: rows of exactly 16 entries of +-1 have
    norm 4 and dot products that are multiples of 1/16.  Returns a namespace q, g, qlab, glab, qgrp, ggrp.

    Gallery rows 0, M // 2 and M - 1 are bit-identical, row 1 is zero (M >= 4).  Labels are drawn over 18
    bits; gallery rows 2 and 3 (M >= 4) have none, row M - 1 has all 64 bits.

    groups = 'none': q [N, Dl] of related and unrelated rows, query 0 the duplicated row, query 2 zero, query
      1 without labels, query 3 with all 64 bits; no group vectors.
    groups = 'self': the gallery queries itself (q IS g, N = M rows) with qgrp = ggrp = arange: query M // 2
      is the MIDDLE duplicate, so its own row is not the first of its ties (rows 0 and M - 1 remain).
    groups = 'groups': the queries of 'none'; the gallery falls into runs of 1 - 5 rows with one id each (a
      gallery of at most 5 rows is one group), query i gets the id of a random gallery row, every third query
      -1 (sees everything), and query 0 the id of gallery row 0: with M <= 5 its group is the whole gallery."""
    gen = torch.Generator().manual_seed(seed)
    g = _unit_rows(M, Dl, gen)
    g[M // 2] = g[0]
    g[M - 1] = g[0]
    if M >= 4:
        g[1] = 0
    glab = random_labels(M, gen)
    if M >= 4:
        glab[2] = 0
        glab[3] = 0
    glab[M - 1] = -1                                                 # all 64 bits
    if groups == 'self':
        ar = torch.arange(M, dtype=torch.int32)
        return types.SimpleNamespace(q=g, g=g, qlab=glab, glab=glab, qgrp=ar, ggrp=ar)
    q = _unit_rows(N, Dl, gen)
    src = torch.randint(0, M, (N,), generator=gen)
    for i in range(0, N, 2):                                         # even queries: a gallery row, i % 5 signs flipped
        q[i] = g[src[i]]
        nz = q[i].nonzero().flatten()[:i % 5]
        q[i, nz] = -q[i, nz]
    q[0] = g[0]
    if N >= 3:
        q[2] = 0
    qlab = random_labels(N, gen)
    for i in range(4, N, 4):                                         # some queries carry a gallery row's labels
        qlab[i] = glab[src[i]]
    if N >= 2:
        qlab[1] = 0
    if N >= 4:
        qlab[3] = -1
    assert int(((q != 0).sum(1) % 16 != 0).sum()) == 0 and int(((g != 0).sum(1) % 16 != 0).sum()) == 0
    qgrp = ggrp = None
    if groups == 'groups':
        ggrp = torch.zeros(M, dtype=torch.int32)
        j, gid = 0, 0
        while j < M:
            run = M if M <= 5 else int(torch.randint(1, 6, (1,), generator=gen))
            ggrp[j:j + run] = 100 + gid
            j, gid = j + run, gid + 1
        qgrp = ggrp[torch.randint(0, M, (N,), generator=gen)].clone()
        qgrp[1::3] = -1
        qgrp[0] = ggrp[0]
    else:
        assert groups == 'none'
    return types.SimpleNamespace(q=q, g=g, qlab=qlab, glab=glab, qgrp=qgrp, ggrp=ggrp)


# ----------------------------------------------------------------------------------- random inputs
def random_case(N, M, Dl, seed):
    """Latents of rank 3 plus noise (cosines spread over [-1, 1] rather than bunched within 1 / sqrt(Dl), so
    few adjacent list places are closer than 1e-6), random 18-bit labels, self-exclusion by arange groups."""
    gen = torch.Generator().manual_seed(seed)
    B = torch.randn(3, Dl, generator=gen)
    q = torch.randn(N, 3, generator=gen) @ B + 0.3 * torch.randn(N, Dl, generator=gen)
    g = torch.randn(M, 3, generator=gen) @ B + 0.3 * torch.randn(M, Dl, generator=gen)
    return types.SimpleNamespace(q=q, g=g, qlab=random_labels(N, gen), glab=random_labels(M, gen),
                                 qgrp=torch.arange(N, dtype=torch.int32), ggrp=torch.arange(M, dtype=torch.int32))


def clear_queries(ref, kmax, gap=1e-6):
    """[N] bool: the queries whose smallest float64 gap between adjacent list places, and between place
    K_max and K_max + 1, is at least ``gap`` (only among visible rows: -inf places give infinite gaps)."""
    v = ref.sorted[:, :kmax + 1]
    d = v[:, :-1] - v[:, 1:]
    d = torch.where(torch.isnan(d), torch.full_like(d, float('inf')), d)       # -inf - -inf
    return d.min(1).values >= gap if d.shape[1] else torch.ones(v.shape[0], dtype=torch.bool)
