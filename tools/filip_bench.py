#!/usr/bin/env python3
"""Time the fine-grained (FILIP) loss kernel (ctclip_filip_loss: loss and every gradient from one call, the
Bg x Bg x T x I scores never written) against a torch restatement of the same loss and gradient on the same
device (f32, the scores materialised, autograd through amax), at the base configuration: Bg = 8, T = 512,
I = 576, Dl = 512, once with 128 unmasked text tokens per report and once with all 512.

Per call: HIP events around one step, warm, median of --reps (the two versions alternate inside one loop).
The floor is ONE product of the unmasked scores, 2 Bg^2 Tu I Dl flop, at the f32 matrix rate (157.3 TF spec);
the kernel forms that product twice (once per argmax direction), so half of the floor rate is its own ceiling.
Not a test; sets no threshold.  Prints one JSON line per case; --log also appends them to a file.

    python tools/filip_bench.py [--Bg 8 --T 512 --I 576 --Dl 512 --reps 30 --log profiles/filip_bench.log]
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


def torch_step(t_raw, i_raw, mask, log_temp):
    """The plain restatement: loss and gradients through autograd, S [Bg, Bg, T, I] in memory."""
    t, i, lt = (x.detach().clone().requires_grad_(True) for x in (t_raw, i_raw, log_temp))
    m = mask.bool()
    S = lt.exp() * torch.einsum('xtd,yid->xyti', F.normalize(t, dim=-1), F.normalize(i, dim=-1))
    mf = m.float()
    A = (S.amax(3) * mf[:, None, :]).sum(2) / mf.sum(1).clamp_min(1e-6)[:, None]
    C = S.masked_fill(~m[:, None, :, None], -torch.finfo(S.dtype).max).amax(2).mean(2)

    def direction(M):
        e = M.exp()
        return (torch.log(e.sum(1) + 1e-20) - torch.log(e.diagonal() + 1e-20)).mean()

    loss = 0.5 * (direction(A) + direction(C))
    loss.backward()
    return loss.detach(), t.grad, i.grad, lt.grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--Bg', type=int, default=8)
    ap.add_argument('--T', type=int, default=512)
    ap.add_argument('--I', type=int, default=576)
    ap.add_argument('--Dl', type=int, default=512)
    ap.add_argument('--unmasked', type=int, nargs='+', default=[128, 512])
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--log', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('filip_bench: needs the GPU (a timing taken elsewhere says nothing)')
    from ctclip_mi355x import kernels as K
    g = torch.Generator().manual_seed(0)
    t = torch.randn(a.Bg, a.T, a.Dl, generator=g).cuda()
    i = torch.randn(a.Bg, a.I, a.Dl, generator=g).cuda()
    lt = torch.tensor([math.log(1 / 0.07)]).cuda()

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) * 1e3          # us

    for tu in a.unmasked:
        mask = torch.zeros(a.Bg, a.T, dtype=torch.uint8)
        mask[:, :tu] = 1
        mask = mask.cuda()
        fused = lambda: K.filip_loss(t, i, mask, lt)
        plain = lambda: torch_step(t, i, mask, lt)
        # same numbers first: faster and different is not faster
        f, (pl, pdt, pdi, pdl) = fused(), plain()
        rel = lambda x, y: float((x.double() - y.double()).norm() / y.double().norm())
        agree = dict(loss=abs(float(f['loss']) - float(pl)), dt=rel(f['dt'], pdt), di=rel(f['di'], pdi),
                     dlt=rel(f['dlt'], pdl.reshape(1)))
        for _ in range(a.warmup):
            fused()
            plain()
        torch.cuda.synchronize()
        tf, tp = [], []
        for _ in range(a.reps):
            tf.append(timed(fused))
            tp.append(timed(plain))
        flop = 2.0 * a.Bg * a.Bg * min(tu, a.T) * a.I * a.Dl
        mf, mp = statistics.median(tf), statistics.median(tp)
        res = dict(tool='filip_bench', Bg=a.Bg, T=a.T, I=a.I, Dl=a.Dl, unmasked=tu, reps=a.reps,
                   fused_us=round(mf, 1), fused_min_us=round(min(tf), 1), fused_max_us=round(max(tf), 1),
                   torch_us=round(mp, 1), torch_min_us=round(min(tp), 1), torch_max_us=round(max(tp), 1),
                   speedup=round(mp / mf, 3), one_product_gflop=round(flop / 1e9, 2),
                   floor_us=round(flop / MFMA_F32 * 1e6, 1), fraction_of_floor=round(flop / MFMA_F32 * 1e6 / mf, 3),
                   scores_bytes_not_written=4 * a.Bg * a.Bg * a.T * a.I, agree=agree,
                   device=torch.cuda.get_device_name(0))
        line = json.dumps(res)
        print(line)
        if a.log:
            os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
            with open(a.log, 'a') as fh:
                fh.write(line + '\n')


if __name__ == '__main__':
    main()
