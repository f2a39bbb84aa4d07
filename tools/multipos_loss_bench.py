#!/usr/bin/env python3
"""Time the multi-positive InfoNCE loss kernels (ctclip_multipos_loss: loss and every gradient from one call) at
(Bg, Dl) = (8, 512), (128, 512), (1024, 512), (8192, 512), about a quarter of the rows in duplicate groups, against
  * the InfoNCE kernels ``ClipLossFn`` takes at the same shape (the one-workgroup ctclip_clip_loss up to 128
    rows, the tiled ctclip_clip_loss_tiled above) on the same latents -- recorded, not gated: the extra work
    is the maximum pass and the mask terms;
  * a torch restatement of the same loss and gradient on the same device (f32, autograd).

Per call: HIP events around one call, warm, median of --reps (the three versions alternate inside one loop).
The kernel forms three f32-MFMA products of 2 Bg^2 Dl flop each (the logits, G . I^ and G^T . T^); the floor is
those 6 Bg^2 Dl flop at the f32 matrix rate (157.3 TF spec).  Not a test; sets no threshold.  Prints one JSON
line per shape; --log also appends them to a file.

    python tools/multipos_loss_bench.py [--shapes 8x512 128x512 1024x512 8192x512 --reps 30 --log FILE]
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


def torch_step(t_raw, i_raw, ids, log_temp):
    """The plain restatement: loss and gradients through autograd."""
    t, i, lt = (x.detach().clone().requires_grad_(True) for x in (t_raw, i_raw, log_temp))
    x = lt.exp() * (F.normalize(t, dim=-1) @ F.normalize(i, dim=-1).t())
    same = (ids[:, None] == ids[None, :]).to(x.dtype)
    n = same.sum(1)
    loss = 0.5 * ((torch.logsumexp(x, 1) - (x * same).sum(1) / n).mean()
                  + (torch.logsumexp(x, 0) - (x * same).sum(0) / n).mean())
    loss.backward()
    return loss.detach(), t.grad, i.grad, lt.grad, (same.sum() - ids.numel()).to(torch.int32)


def quarter_duplicates(Bg, g):
    """Group ids with about a quarter of the rows in duplicate groups (pairs and triples at random rows)."""
    ids = torch.arange(Bg, dtype=torch.int64) * 2654435761 + 17
    perm = torch.randperm(Bg, generator=g)[:Bg // 4]
    k = 0
    while k + 1 < len(perm):
        size = 3 if (k // 2) % 4 == 3 and k + 2 < len(perm) else 2
        ids[perm[k + 1:k + size]] = ids[perm[k]].item()
        k += size
    return ids


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', nargs='+', default=['8x512', '128x512', '1024x512', '8192x512'])
    ap.add_argument('--reps', type=int, default=30)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--log', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('multipos_loss_bench: needs the GPU (a timing taken elsewhere says nothing)')
    from ctclip_mi355x import functional as Fn
    from ctclip_mi355x import kernels as K
    lt = torch.tensor([math.log(10.0)]).cuda()

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) * 1e3          # us

    for shape in a.shapes:
        Bg, Dl = (int(v) for v in shape.split('x'))
        g = torch.Generator().manual_seed(0)
        t = torch.randn(Bg, Dl, generator=g).cuda()
        i = torch.randn(Bg, Dl, generator=g).cuda()
        ids = quarter_duplicates(Bg, g).cuda()
        fused = lambda: K.multipos_loss(t, i, ids, lt)
        if Fn.loss_uses_tiled(Bg):
            infonce, which = (lambda: K.clip_loss_tiled(t[None], i[None], lt)), 'clip_loss_tiled'
        else:
            infonce, which = (lambda: K.clip_loss(t, i, lt)), 'clip_loss'
        plain = lambda: torch_step(t, i, ids, lt)
        # same numbers first: faster and different is not faster
        f, p = fused(), plain()
        rel = lambda x, y: float((x.double() - y.double()).norm() / y.double().norm())
        agree = dict(loss=abs(float(f[0]) - float(p[0])) / max(1.0, abs(float(p[0]))), dt=rel(f[1], p[1]),
                     di=rel(f[2], p[2]), dlt=rel(f[3], p[3].reshape(1)), npos=[int(f[4]), int(p[4])])
        del f, p
        for _ in range(a.warmup):
            fused()
            infonce()
            plain()
        torch.cuda.synchronize()
        tf, tn, tp = [], [], []
        for _ in range(a.reps):
            tf.append(timed(fused))
            tn.append(timed(infonce))
            tp.append(timed(plain))
        flop = 6.0 * Bg * Bg * Dl
        mf, mn, mp = statistics.median(tf), statistics.median(tn), statistics.median(tp)
        res = dict(tool='multipos_loss_bench', Bg=Bg, Dl=Dl, reps=a.reps, launches=6,
                   multipos_us=round(mf, 1), multipos_min_us=round(min(tf), 1), multipos_max_us=round(max(tf), 1),
                   infonce_kernel=which, infonce_us=round(mn, 1), infonce_min_us=round(min(tn), 1),
                   infonce_max_us=round(max(tn), 1),
                   torch_us=round(mp, 1), torch_min_us=round(min(tp), 1), torch_max_us=round(max(tp), 1),
                   speedup_vs_torch=round(mp / mf, 3), ratio_to_infonce=round(mf / mn, 3),
                   mfma_products=3, gflop=round(flop / 1e9, 3), floor_us=round(flop / MFMA_F32 * 1e6, 2),
                   fraction_of_floor=round(flop / MFMA_F32 * 1e6 / mf, 4), agree=agree,
                   device=torch.cuda.get_device_name(0))
        line = json.dumps(res)
        print(line, flush=True)
        if a.log:
            os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
            with open(a.log, 'a') as fh:
                fh.write(line + '\n')


if __name__ == '__main__':
    main()
