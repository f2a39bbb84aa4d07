#!/usr/bin/env python3
"""Time the fused case retrieval pass (ctclip_case_retrieval: each volume's 50 best other volumes and their
label-graded hits@K / AP@K / Jaccard gain@K, the N x M scores never written) with the gallery querying itself
under self-exclusion, Dl = 512, ks = (1, 5, 10, 50), 18 labels, at

    N = M = 3,039    CT-RATE's validation volumes
    N = M = 16,384

against (a) a torch f32 restatement on the same device -- normalise, ``matmul``, mask the diagonal, ``topk``,
gather the labels, the metrics, and the relevant-row count as a second (label) product; it writes the N x M
matrix and has no tie rule -- and (b) ``ctclip_retrieval_topk`` with k = 50 alone: the cost of the list without
exclusion, counts or metrics.

Per version: HIP events around one call (the C-ABI call itself for the two kernels, outputs and workspace
allocated beforehand), --warmup calls, then --reps; the median and min - max are reported.  The floor is one
product, 2 N M Dl flop, at the f32 matrix rate (157.3 TF spec).  Not a test; sets no threshold.  Prints one
JSON line per case; --log also appends them to a file.

    python tools/case_retrieval_bench.py [--reps 11 --warmup 3 --log profiles/case_retrieval_bench.log]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'ctpa-clip_amd'))

MFMA_F32 = 157.3e12          # flop / s, spec
KS = (1, 5, 10, 50)
LABELS = 18


def torch_case(x, Y, ks):
    """The plain restatement ('any' relevance), S [N, N] in memory.  Y [N, C] f32 0 / 1."""
    N = x.shape[0]
    xn = F.normalize(x, dim=1, eps=1e-12)
    S = xn @ xn.t()
    S.fill_diagonal_(-float('inf'))
    score, idx = torch.topk(S, ks[-1], dim=1)
    inter = Y @ Y.t()                                                # |a & b|
    cnt = Y.sum(1)
    empty = cnt == 0
    rel_all = (inter > 0) | (empty[:, None] & empty[None, :])
    rel_all.fill_diagonal_(False)
    nrel = rel_all.sum(1)
    ii = inter.gather(1, idx)
    union = cnt[:, None] + cnt[idx] - ii
    jac = torch.where(union > 0, ii / union.clamp_min(1), torch.ones_like(ii)).double()
    rel = rel_all.gather(1, idx)
    h = rel.cumsum(1)
    r = torch.arange(1, ks[-1] + 1, device=x.device)
    prec = torch.where(rel, h.double() / r, torch.zeros((), dtype=torch.float64, device=x.device)).cumsum(1)
    gain = jac.cumsum(1)
    kk = torch.tensor(ks, device=x.device)
    ap = prec[:, kk - 1] / torch.minimum(kk[None, :], nrel[:, None]).clamp_min(1)
    ap = torch.where(nrel[:, None] > 0, ap, torch.full_like(ap, -1.0))
    return idx, score, nrel, h[:, kk - 1], ap, gain[:, kk - 1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', type=int, nargs='+', default=[3039, 16384])
    ap.add_argument('--Dl', type=int, default=512)
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--log', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('case_retrieval_bench: needs the GPU (a timing taken elsewhere says nothing)')
    from ctclip_mi355x import _lib
    from ctclip_mi355x._lib import call, ptr, stream_ptr
    from ctclip_mi355x.retrieval import pack_labels
    i32, f64 = torch.int32, torch.float64
    kmax, nK = KS[-1], len(KS)
    ks_arr = (_lib.c_i32 * nK)(*KS)

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e)             # ms

    for N in a.sizes:
        gen = torch.Generator().manual_seed(0)
        # rank 16 plus noise: neighbours exist, as among real volumes
        x = (torch.randn(N, 16, generator=gen) @ torch.randn(16, a.Dl, generator=gen)
             + torch.randn(N, a.Dl, generator=gen)).cuda()
        Yh = (torch.rand(N, LABELS, generator=gen) < 0.12)
        Y, lab = Yh.float().cuda(), pack_labels(Yh).cuda()
        grp = torch.arange(N, dtype=i32, device='cuda')
        dev = dict(device='cuda')
        o = dict(idx=torch.empty(N, kmax, dtype=i32, **dev), score=torch.empty(N, kmax, **dev),
                 filled=torch.empty(N, dtype=i32, **dev), nrel=torch.empty(N, dtype=i32, **dev),
                 hits=torch.empty(N, nK, dtype=i32, **dev), ap=torch.empty(N, nK, dtype=f64, **dev),
                 gain=torch.empty(N, nK, dtype=f64, **dev))
        nb_case = _lib.lib().ctclip_case_retrieval_ws_bytes(N, N, a.Dl, kmax)
        nb_topk = _lib.lib().ctclip_retrieval_topk_ws_bytes(N, N, a.Dl, kmax)
        ws = torch.empty(max(nb_case, nb_topk) // 4, **dev)
        ts, ti = torch.empty(N, kmax, **dev), torch.empty(N, kmax, dtype=i32, **dev)

        def kernel():
            call('ctclip_case_retrieval', ptr(x), ptr(x), ptr(lab), ptr(lab), ptr(grp), ptr(grp), N, N, a.Dl, ks_arr,
                 nK, 0, ptr(o['idx']), ptr(o['score']), ptr(o['filled']), ptr(o['nrel']), ptr(o['hits']),
                 ptr(o['ap']), ptr(o['gain']), ptr(ws), nb_case, stream_ptr())

        def topk_alone():
            call('ctclip_retrieval_topk', ptr(x), ptr(x), N, N, a.Dl, kmax, ptr(ts), ptr(ti), ptr(ws), nb_topk,
                 stream_ptr())

        fns = dict(kernel=kernel, torch_f32=lambda: torch_case(x, Y, KS), retrieval_topk=topk_alone)
        # same numbers first: faster and different is not faster
        kernel()
        t_idx, t_score, t_nrel, t_hits, t_ap, t_gain = torch_case(x, Y, KS)
        same_list = (t_idx == o['idx']).all(1)
        agree = dict(score=float((t_score - o['score']).abs().max()), nrel_equal=bool((t_nrel == o['nrel']).all()),
                     lists_equal=round(float(same_list.float().mean()), 4),
                     ap_where_lists_equal=float((t_ap - o['ap'])[same_list].abs().max()),
                     gain_where_lists_equal=float((t_gain - o['gain'])[same_list].abs().max()),
                     hits_where_lists_equal=bool((t_hits == o['hits'])[same_list].all()),
                     map_at_k=[round(float(v), 4) for v in o['ap'][o['ap'][:, 0] != -1].mean(0)])
        del t_idx, t_score, t_nrel, t_hits, t_ap, t_gain
        for _ in range(a.warmup):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in fns}
        for _ in range(a.reps):
            for k, fn in fns.items():
                t[k].append(timed(fn))
        flop = 2.0 * N * N * a.Dl
        res = dict(tool='case_retrieval_bench', N=N, M=N, Dl=a.Dl, ks=list(KS), labels=LABELS, reps=a.reps,
                   warmup=a.warmup)
        mk = statistics.median(t['kernel'])
        for k in fns:
            res[k + '_ms'] = round(statistics.median(t[k]), 3)
            res[k + '_min_ms'], res[k + '_max_ms'] = round(min(t[k]), 3), round(max(t[k]), 3)
            if k != 'kernel':
                res['kernel_time_over_' + k] = round(mk / statistics.median(t[k]), 3)
        res.update(one_product_gflop=round(flop / 1e9, 2), floor_ms=round(flop / MFMA_F32 * 1e3, 3),
                   fraction_of_floor=round(flop / MFMA_F32 * 1e3 / mk, 3), workspace_mib=round(nb_case / 2 ** 20, 1),
                   scores_bytes_not_written=4 * N * N, agree=agree, device=torch.cuda.get_device_name(0))
        line = json.dumps(res)
        print(line, flush=True)
        if a.log:
            os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
            with open(a.log, 'a') as fh:
                fh.write(line + '\n')
        del x, Y, lab, grp, o, ws, ts, ti, fns
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
