"""GPU micro-benchmark of the curve-metric kernel (DESIGN.md "Operating points and PR-AUC"):
ctclip_curve_boot beside ctclip_auroc_boot on the same device buffers at P = 18, S = 1000,
N = 2000 and N = 8192 (continuous scores, 30 % prevalence, the reference's resamples), and the host
loop the kernel replaces at N = 2000: per (resample, label) one ``roc_curve`` and one
``precision_recall_curve`` (--host-resamples of the S resamples timed, scaled to S; skipped
without sklearn).

HIP events around single launches, 3 warm-up launches, --reps timed ones, the two kernels
interleaved; median and min - max.  python tools/curve_bench.py [--reps 11] [--host-resamples 50]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'ctpa-clip_amd'))
from ctclip_mi355x import evaluate as E  # noqa: E402
from ctclip_mi355x._lib import call, ptr, stream_ptr  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=11)
    ap.add_argument('--host-resamples', type=int, default=50)
    a = ap.parse_args()
    P, S = 18, 1000
    for N in (2000, 8192):
        g = np.random.default_rng(N)
        probs = g.random((N, P)).astype(np.float32)
        labels = (g.random((N, P)) < 0.3).astype(np.uint8)
        s, y, order = E._sorted_scores(torch.from_numpy(probs).cuda(), torch.from_numpy(labels))
        rows_h = E.bootstrap_indices(N, S)
        rows = torch.from_numpy(rows_h).cuda()
        outs = {'ctclip_auroc_boot': torch.empty(S, P, device='cuda', dtype=torch.float64),
                'ctclip_curve_boot': torch.empty(S, P, 5, device='cuda', dtype=torch.float64)}
        times = {k: [] for k in outs}
        for rep in range(3 + a.reps):
            for sym, out in outs.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                call(sym, ptr(s), ptr(y), ptr(order), ptr(rows), N, P, S, ptr(out), stream_ptr())
                t1.record()
                torch.cuda.synchronize()
                if rep >= 3:
                    times[sym].append(t0.elapsed_time(t1) * 1e3)
        med = {}
        for sym, t in times.items():
            med[sym] = float(np.median(t))
            print(f'N = {N}, P = {P}, S = {S}: {sym} {med[sym]:8.1f} us ({min(t):.1f} - {max(t):.1f}), {len(t)} launches',
                  flush=True)
        print(f'N = {N}: curve / auroc = {med["ctclip_curve_boot"] / med["ctclip_auroc_boot"]:.2f}', flush=True)
        if N != 2000:
            continue
        try:
            from sklearn.metrics import precision_recall_curve, roc_curve
        except ImportError:
            print('host loop: sklearn is not installed, skipped')
            continue
        hs = min(a.host_resamples, S)
        yd = labels.astype(np.float64)
        t0 = time.perf_counter()
        for i in range(hs):
            r = rows_h[i]
            for j in range(P):
                roc_curve(yd[r, j], probs[r, j])
                precision_recall_curve(yd[r, j], probs[r, j])
        ms = (time.perf_counter() - t0) * 1e3 * S / hs
        print(f'N = {N}: host loop, {S} x {P} roc_curve + precision_recall_curve: {ms:9.1f} ms '
              f'({hs} resamples timed, scaled) = {ms * 1e3 / med["ctclip_curve_boot"]:.0f} x the kernel', flush=True)


if __name__ == '__main__':
    main()
