#!/usr/bin/env python3
"""Time the SimSiam visual self-supervision head (``VisualSSLHead`` forward + backward on csrc/ssl.hip) at
B = 8 and 16 volumes per view, dim_latent 512, the default widths (hidden 4096, projection 256), against
  * the same head's f32 torch ``nn.Sequential`` restatement (the CPU path's code) on the same device;
  * the floor of streaming the head's f32 weights once in the forward and twice in the backward (dX and dW
    each read or write every weight) at the HBM rate DESIGN.md uses, 6.29 TB/s.

Per call: HIP events around one forward + backward, warm, median of --reps with the two versions alternating
inside one loop.  Not a test; sets no threshold.  Prints one JSON line per batch size; --log appends them.

    python tools/visual_ssl_bench.py [--batches 8 16 --reps 20 --log FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'ctpa-clip_amd'))

HBM = 6.29e12                # bytes / s


def torch_forward(head, views):
    """The restatement path of VisualSSLHead.forward on device tensors."""
    from ctclip_mi355x.visual_ssl import simsiam_loss_rows
    z = [head.projector(views[g]) for g in range(2)]
    p = [head.predictor(z[g]) for g in range(2)]
    return (simsiam_loss_rows(p[0], z[1].detach()) + simsiam_loss_rows(p[1], z[0].detach())).mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batches', nargs='+', type=int, default=[8, 16])
    ap.add_argument('--dim', type=int, default=512)
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--log', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('visual_ssl_bench: needs the GPU (a timing taken elsewhere says nothing)')
    from ctclip_mi355x.visual_ssl import VisualSSLHead
    torch.manual_seed(0)
    head = VisualSSLHead(a.dim).cuda().train()
    wbytes = 4 * sum(p.numel() for p in head.parameters() if p.ndim == 2)
    floor_us = 3 * wbytes / HBM * 1e6

    def step(fn, views):
        leaf = views.detach().clone().requires_grad_(True)
        for p in head.parameters():
            p.grad = None
        loss = fn(leaf)
        loss.backward()
        return loss.detach(), leaf.grad

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) * 1e3          # us

    for B in a.batches:
        g = torch.Generator().manual_seed(B)
        views = torch.randn(2, B, a.dim, generator=g).cuda()
        fused = lambda: step(head, views)
        plain = lambda: step(lambda v: torch_forward(head, v), views)
        # same numbers first: faster and different is not faster
        f, p = fused(), plain()
        agree = dict(loss=abs(float(f[0]) - float(p[0])) / max(1.0, abs(float(p[0]))),
                     dviews=float((f[1].double() - p[1].double()).norm() / p[1].double().norm()))
        for _ in range(a.warmup):
            fused()
            plain()
        torch.cuda.synchronize()
        tf, tp = [], []
        for _ in range(a.reps):
            tf.append(timed(fused))
            tp.append(timed(plain))
        mf, mp = statistics.median(tf), statistics.median(tp)
        res = dict(tool='visual_ssl_bench', B=B, dim=a.dim, hidden=head.projection_hidden_size,
                   projection=head.projection_size, reps=a.reps,
                   hip_us=round(mf, 1), hip_min_us=round(min(tf), 1), hip_max_us=round(max(tf), 1),
                   torch_us=round(mp, 1), torch_min_us=round(min(tp), 1), torch_max_us=round(max(tp), 1),
                   speedup_vs_torch=round(mp / mf, 3), weight_mbytes=round(wbytes / 1e6, 2),
                   floor_us=round(floor_us, 2), fraction_of_floor=round(floor_us / mf, 4), agree=agree,
                   device=torch.cuda.get_device_name(0))
        line = json.dumps(res)
        print(line, flush=True)
        if a.log:
            os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
            with open(a.log, 'a') as fh:
                fh.write(line + '\n')


if __name__ == '__main__':
    main()
