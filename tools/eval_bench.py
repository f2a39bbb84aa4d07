"""GPU micro-benchmark of the validation loop's two kernels (DESIGN.md "Zero-shot evaluation"):

  * the evaluation loader (ctclip_eval_volume) at full size: a stored (240, 480, 480) scan, f32 and
    f64, into the (1, 240, 480, 480) f32 tensor -- 221 MB (f64: 442 MB) read + 221 MB written;
    prints us per launch, GB/s and the fraction of the 8.0 TB/s HBM peak; and a typical smaller scan
    (mostly padding: the write stream alone);
  * the bootstrap AUROC (ctclip_auroc_boot) at N = 100 and N = 3000, P = 18, S = 1000: the kernel
    alone (order and resample indices on the device), the whole ``bootstrap_auroc`` call (index
    generation with numpy, upload, sort, kernel), and the same table from a numpy restatement on
    this machine's host (--host-resamples of the S resamples, scaled to S).

HIP events around --reps launches each.  python tools/eval_bench.py [--reps 20] [--host-resamples 100]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'ctpa-clip_amd'))
from ctclip_mi355x import evaluate as E  # noqa: E402
from ctclip_mi355x.preprocess import eval_volume_to_tensor  # noqa: E402
from ctclip_mi355x._lib import call, ptr, stream_ptr  # noqa: E402

HBM_PEAK = 8.0e12


def timeit(fn, reps):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1000 / reps


def host_auroc(scores, labels, mult):
    """Tie-aware Mann-Whitney AUROC of one label in numpy (the restatement of tests/test_eval_cpu.py)."""
    order = np.argsort(scores, kind='stable')
    s, pos, neg = scores[order], (labels * mult)[order], ((1 - labels) * mult)[order]
    starts = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]]))
    pos_g, neg_g = np.add.reduceat(pos, starts), np.add.reduceat(neg, starts)
    count = int((pos_g * (2 * (np.cumsum(neg_g) - neg_g) + neg_g)).sum())
    den = 2 * int(pos.sum()) * int(neg.sum())
    return count / den if den else float('nan')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--host-resamples', type=int, default=100)
    a = ap.parse_args()
    torch.manual_seed(0)
    out = torch.empty(1, 240, 480, 480, device='cuda')
    for shape, dt in (((240, 480, 480), torch.float32), ((240, 480, 480), torch.float64),
                      ((200, 400, 400), torch.float32), ((300, 512, 512), torch.float32)):
        scan = (torch.rand(shape, device='cuda', dtype=torch.float32) * 1.8 - 1.3).to(dt)
        us = timeit(lambda: eval_volume_to_tensor(scan, out=out), a.reps)
        used = [min(n, t) for n, t in zip(shape, (240, 480, 480))]
        nbytes = used[0] * used[1] * used[2] * scan.element_size() + out.numel() * 4
        print(f'loader {tuple(shape)} {str(dt)[6:]}: {us:8.1f} us, {nbytes / 1e6:6.1f} MB moved, '
              f'{nbytes / us / 1e3:7.1f} GB/s = {nbytes / (us * 1e-6) / HBM_PEAK:.1%} of HBM peak', flush=True)
    P, S = 18, 1000
    for N in (100, 3000):
        g = np.random.default_rng(N)
        probs = g.random((N, P)).astype(np.float32)
        labels = (g.random((N, P)) < 0.3).astype(np.uint8)
        dp, dl = torch.from_numpy(probs).cuda(), torch.from_numpy(labels).cuda()
        rows_h = E.bootstrap_indices(N, S)
        rows = torch.from_numpy(rows_h).cuda()
        order = torch.sort(dp.t().contiguous(), dim=1).indices.to(torch.int32).contiguous()
        res = torch.empty(S, P, device='cuda', dtype=torch.float64)
        us_k = timeit(lambda: call('ctclip_auroc_boot', ptr(dp), ptr(dl), ptr(order), ptr(rows), N, P, S, ptr(res),
                                   stream_ptr()), a.reps)
        t0 = time.perf_counter()
        full = E.bootstrap_auroc(dp, dl, S)
        torch.cuda.synchronize()
        ms_full = (time.perf_counter() - t0) * 1e3
        hs = min(a.host_resamples, S)
        t0 = time.perf_counter()
        ref = np.empty((hs, P))
        l64 = labels.astype(np.int64)
        for i in range(hs):
            mult = np.bincount(rows_h[i], minlength=N)
            for j in range(P):
                ref[i, j] = host_auroc(probs[:, j], l64[:, j], mult)
        ms_host = (time.perf_counter() - t0) * 1e3 * S / hs
        same = np.array_equal(np.nan_to_num(ref, nan=-1.0), np.nan_to_num(full[:hs].cpu().numpy(), nan=-1.0))
        print(f'bootstrap N = {N}, P = {P}, S = {S}: kernel {us_k:8.1f} us; bootstrap_auroc() end to end '
              f'{ms_full:7.2f} ms; numpy on the host {ms_host:9.1f} ms ({hs} resamples timed, scaled); '
              f'first {hs} rows equal: {same}', flush=True)


if __name__ == '__main__':
    main()
