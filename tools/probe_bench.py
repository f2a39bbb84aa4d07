#!/usr/bin/env python3
"""Time one linear-probe step (ctclip_probe_step: loss, dW, db in one pass over the latents) against what a
user would write in torch on the same device -- two matmuls plus the elementwise BCE-with-logits -- at the
order of a CT-RATE training split: M = 50,000 latents, D = 512, P = 18.

Per call: HIP events around one step, warm, median of --reps (the two versions alternate inside one loop).
The floor is one read of the latents, M * D * 4 bytes, at the HBM rate (8.0 TB/s spec and the 6.29 TB/s a
float4 copy measures).  Not a test; sets no threshold.  Prints one JSON line; --log also appends it to a file.

    python tools/probe_bench.py [--M 50000 --D 512 --P 18 --reps 50 --log profiles/probe_bench.log]
"""
import argparse
import json
import os
import statistics
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, 'ctpa-clip_amd'))

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12          # bytes / s


def torch_step(X, W, b, Yf, pw):
    """The plain restatement: logits, stable BCE-with-logits with pos_weight (mean), gradient by hand."""
    Z = torch.addmm(b, X, W.t())
    L = 1 + (pw - 1) * Yf
    loss = ((1 - Yf) * Z + L * (torch.clamp(-Z, min=0) + torch.log1p(torch.exp(-Z.abs())))).mean()
    r = ((1 - Yf) - L * torch.sigmoid(-Z)) / Z.numel()
    return loss, r.t() @ X, r.sum(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--M', type=int, default=50000)
    ap.add_argument('--D', type=int, default=512)
    ap.add_argument('--P', type=int, default=18)
    ap.add_argument('--reps', type=int, default=50)
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--log', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('probe_bench: needs the GPU (a timing taken elsewhere says nothing)')
    from ctclip_mi355x import kernels as K
    g = torch.Generator().manual_seed(0)
    X = torch.randn(a.M, a.D, generator=g)
    X = (X / X.norm(dim=1, keepdim=True)).cuda()
    W = (torch.randn(a.P, a.D, generator=g) * 0.5).cuda()
    b = (torch.randn(a.P, generator=g) * 0.1).cuda()
    Y = (torch.rand(a.M, a.P, generator=g) < 0.3).to(torch.uint8).cuda()
    Yf = Y.float()
    pw = (torch.rand(a.P, generator=g) * 3 + 0.25).cuda()
    out = dict(loss=torch.empty(1, device='cuda'), dW=torch.empty(a.P, a.D, device='cuda'),
               db=torch.empty(a.P, device='cuda'))

    def fused():
        return K.probe_step(X, W, b, Y, pos_weight=pw, out=out)

    def plain():
        return torch_step(X, W, b, Yf, pw)

    # same numbers first: faster and different is not faster
    f, (pl, pdw, pdb) = fused(), plain()
    rel = lambda x, y: float((x.double() - y.double()).norm() / y.double().norm())
    agree = dict(loss=abs(float(f['loss']) - float(pl)), dW=rel(f['dW'], pdw), db=rel(f['db'], pdb))

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e) * 1e3          # us

    for _ in range(a.warmup):
        fused()
        plain()
    torch.cuda.synchronize()
    tf, tp = [], []
    for _ in range(a.reps):
        tf.append(timed(fused))
        tp.append(timed(plain))
    nbytes = a.M * a.D * 4
    mf, mp = statistics.median(tf), statistics.median(tp)
    res = dict(tool='probe_bench', M=a.M, D=a.D, P=a.P, reps=a.reps,
               fused_us=round(mf, 2), fused_min_us=round(min(tf), 2), fused_max_us=round(max(tf), 2),
               torch_us=round(mp, 2), torch_min_us=round(min(tp), 2), torch_max_us=round(max(tp), 2),
               speedup=round(mp / mf, 3),
               floor_bytes=nbytes, floor_us_spec=round(nbytes / HBM_SPEC * 1e6, 2),
               floor_us_copy=round(nbytes / HBM_COPY * 1e6, 2),
               fraction_of_floor_spec=round(nbytes / HBM_SPEC * 1e6 / mf, 3),
               fraction_of_floor_copy=round(nbytes / HBM_COPY * 1e6 / mf, 3),
               agree=agree, device=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, 'a') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
