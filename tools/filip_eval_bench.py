#!/usr/bin/env python3
"""Time the rectangular token-wise score kernel (ctclip_filip_scores: A and C of R reports x V volumes from ONE
product, forward only, the R x V x T x I scores never written) at the two evaluation shapes, I = 576, Dl = 512:

    zero-shot block   R = 36 prompts with 12 kept of 512 tokens, V = 8
    retrieval block   R = V = 64 with 128 kept of 512 tokens

against (a) a torch f32 restatement on the same device that materialises S, forward only -- once over all T
tokens with the mask applied (``torch_full``), once with the text cut to the kept prefix beforehand
(``torch_kept``, the cheapest torch can be: the masks here are prefixes) -- and (b), on the square retrieval
block only, ``kernels.filip_loss(want_logits=True)``, the only other way to get these numbers.

Per call: HIP events around one call, warm, median of --reps (the versions alternate inside one loop); the
whole measurement is repeated --repeats times and the spread of the medians is reported.  The floor is one
product of the kept scores, 2 R V Tu I Dl flop, at the f32 matrix rate (157.3 TF spec).  Not a test; sets no
threshold.  Prints one JSON line per case; --log also appends them to a file.

    python tools/filip_eval_bench.py [--reps 30 --repeats 3 --log profiles/filip_eval_bench.log]
"""
import argparse
import json
import math
import os
import statistics
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'ctpa-clip_amd'))

MFMA_F32 = 157.3e12          # flop / s, spec
CASES = (('zero_shot_block', 36, 8, 12), ('retrieval_block', 64, 64, 128))      # name, R, V, kept tokens


def torch_scores(t_raw, i_raw, mask, log_temp):
    """The plain restatement, S [R, V, T, I] in memory."""
    m = mask.bool()
    S = log_temp.exp() * torch.einsum('xtd,yid->xyti', F.normalize(t_raw, dim=-1), F.normalize(i_raw, dim=-1))
    mf = m.float()
    A = (S.amax(3) * mf[:, None, :]).sum(2) / mf.sum(1).clamp_min(1e-6)[:, None]
    C = S.masked_fill(~m[:, None, :, None], -torch.finfo(S.dtype).max).amax(2).mean(2)
    return A, C


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--T', type=int, default=512)
    ap.add_argument('--I', type=int, default=576)
    ap.add_argument('--Dl', type=int, default=512)
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--log', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('filip_eval_bench: needs the GPU (a timing taken elsewhere says nothing)')
    from ctclip_mi355x import kernels as K
    lt = torch.tensor([math.log(1 / 0.07)]).cuda()

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) * 1e3          # us

    for name, R, V, tu in CASES:
        g = torch.Generator().manual_seed(0)
        t = torch.randn(R, a.T, a.Dl, generator=g).cuda()
        i = torch.randn(V, a.I, a.Dl, generator=g).cuda()
        mask = torch.zeros(R, a.T, dtype=torch.uint8)
        mask[:, :tu] = 1
        mask = mask.cuda()
        t_kept, mask_kept = t[:, :tu].contiguous(), mask[:, :tu].contiguous()
        fns = dict(kernel=lambda: K.filip_scores(t, i, mask, lt),
                   torch_full=lambda: torch_scores(t, i, mask, lt),
                   torch_kept=lambda: torch_scores(t_kept, i, mask_kept, lt))
        if R == V:
            fns['filip_loss'] = lambda: K.filip_loss(t, i, mask, lt, want_logits=True)
        # same numbers first: faster and different is not faster
        out = fns['kernel']()
        agree = {}
        for k in fns:
            if k == 'kernel':
                continue
            o = fns[k]()
            A, C = (o['A'], o['C']) if isinstance(o, dict) else o
            agree[k] = dict(A=float((out['A'] - A).abs().max()), C=float((out['C'] - C).abs().max()))
            del o, A, C
        medians = {k: [] for k in fns}
        lo, hi = {k: math.inf for k in fns}, {k: 0.0 for k in fns}
        for _ in range(a.repeats):
            for _ in range(a.warmup):
                for fn in fns.values():
                    fn()
            torch.cuda.synchronize()
            ts = {k: [] for k in fns}
            for _ in range(a.reps):
                for k, fn in fns.items():
                    ts[k].append(timed(fn))
            for k in fns:
                medians[k].append(statistics.median(ts[k]))
                lo[k], hi[k] = min(lo[k], min(ts[k])), max(hi[k], max(ts[k]))
        flop = 2.0 * R * V * tu * a.I * a.Dl
        mk = statistics.median(medians['kernel'])
        res = dict(tool='filip_eval_bench', case=name, R=R, V=V, T=a.T, kept=tu, I=a.I, Dl=a.Dl, reps=a.reps,
                   repeats=a.repeats)
        for k in fns:
            res[k + '_us'] = round(statistics.median(medians[k]), 1)
            res[k + '_medians_us'] = [round(x, 1) for x in medians[k]]
            res[k + '_spread_us'] = round(max(medians[k]) - min(medians[k]), 1)
            res[k + '_min_us'], res[k + '_max_us'] = round(lo[k], 1), round(hi[k], 1)
            if k != 'kernel':
                # the slowest kernel median against the fastest median of the other: the ratio that survives the spread
                res['speedup_vs_' + k] = round(statistics.median(medians[k]) / mk, 3)
                res['worst_case_speedup_vs_' + k] = round(min(medians[k]) / max(medians['kernel']), 3)
        res.update(one_product_gflop=round(flop / 1e9, 2), floor_us=round(flop / MFMA_F32 * 1e6, 1),
                   fraction_of_floor=round(flop / MFMA_F32 * 1e6 / mk, 3),
                   scores_bytes_not_written=4 * R * V * a.T * a.I, agree=agree, device=torch.cuda.get_device_name(0))
        line = json.dumps(res)
        print(line)
        if a.log:
            os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
            with open(a.log, 'a') as fh:
                fh.write(line + '\n')
        del t, i, mask, t_kept, mask_kept, fns, out
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
