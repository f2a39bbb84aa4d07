#!/usr/bin/env python3
"""Time the volume-augmentation kernel (ctclip_augment_volume: every view of every sample in one launch) at
B = 8, V = 1 and 2, (D, H, W) = (240, 480, 480), int16 HU and f32, against
  * its HBM floor: one read and one write of the volume per view at 6.29 TB/s (the achievable rate of
    MI355X_MICROARCH's HBM section);
  * a torch restatement on the same device: ``affine_grid`` / ``grid_sample(align_corners=True)`` on the 5-D
    tensor + gain / shift + ``randn`` noise + clip (int16: normalised first and rounded back to HU after), the
    whole batch per view, or one volume at a time if the batch's sampling grid does not fit.

Per call: HIP events around one call, warm, median of --reps (the two versions alternate inside one loop).  The
records are drawn once (CTAugment's default ranges) and already on the device, so the timed call is the launch
alone.  Not a test; sets no threshold.  Prints one JSON line per case; --log also appends them to a file.

    python tools/augment_bench.py [--batch 8 --views 1 2 --shape 240 480 480 --reps 20 --log FILE]
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

HBM = 6.29e12                # bytes / s, achievable


def theta_of(matrix, D, H, W):
    """[B, 3, 4] voxel-space inverse maps (axes d, h, w) -> affine_grid's theta: normalised coordinates
    (align_corners=True: n = (i - c) / c), axes (x, y, z) = (w, h, d)."""
    c = torch.tensor([(D - 1) / 2, (H - 1) / 2, (W - 1) / 2], dtype=torch.float64)
    th = matrix.clone()
    th[:, :, :3] = matrix[:, :, :3] * c[None, None, :] / c[None, :, None]
    th[:, :, 3] = matrix[:, :, 3] / c[None, :]
    return th.flip(1)[:, :, [2, 1, 0, 3]].float()


def torch_views(video, params, noise=True, per_volume=False):
    """The plain restatement, [V, B, 1, D, H, W]."""
    B, _, D, H, W = video.shape
    i16 = video.dtype == torch.int16
    out = torch.empty((params.gain.shape[0],) + tuple(video.shape), device=video.device, dtype=video.dtype)
    for v in range(out.shape[0]):
        theta = theta_of(params.matrix[v], D, H, W).to(video.device)
        gain, shift, sigma = (t[v].float().to(video.device).view(B, 1, 1, 1, 1) for t in
                              (params.gain, params.shift, params.sigma))
        for lo in range(0, B, 1 if per_volume else B):
            sl = slice(lo, lo + (1 if per_volume else B))
            x = video[sl].float().clamp(-1000, 1000) / 1000 if i16 else video[sl]
            grid = F.affine_grid(theta[sl], x.shape, align_corners=True)
            y = F.grid_sample(x + 1.0, grid, mode='bilinear', padding_mode='zeros', align_corners=True) - 1.0
            y = gain[sl] * y + shift[sl]
            if noise:
                y = y + sigma[sl] * torch.randn_like(y)
            y = y.clamp(-1.0, 1.0)
            out[v, sl] = torch.round(1000.0 * y).to(torch.int16) if i16 else y
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--views', type=int, nargs='+', default=[1, 2])
    ap.add_argument('--shape', type=int, nargs=3, default=[240, 480, 480])
    ap.add_argument('--dtypes', nargs='+', default=['int16', 'float32'])
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--torch-reps', type=int, default=5)
    ap.add_argument('--log', default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('augment_bench: needs the GPU (a timing taken elsewhere says nothing)')
    from ctclip_mi355x.augment import CTAugment, augment_volume

    def timed(fn):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        return s.elapsed_time(e)                # ms

    B, (D, H, W) = a.batch, a.shape
    for name in a.dtypes:
        dtype = getattr(torch, name)
        g = torch.Generator(device='cuda').manual_seed(0)
        if dtype == torch.int16:
            video = torch.randint(-1000, 1001, (B, 1, D, H, W), generator=g, device='cuda', dtype=torch.int16)
        else:
            video = torch.rand(B, 1, D, H, W, generator=g, device='cuda') * 2.0 - 1.0
        for V in a.views:
            params = CTAugment(seed=0).draw(step=0, B=B, n_views=V)
            rec = params.pack().cuda()
            fused = lambda: augment_volume(video, rec)
            per_volume = False
            try:
                torch_views(video, params)
            except torch.OutOfMemoryError:
                per_volume = True
                torch.cuda.empty_cache()
            plain = lambda: torch_views(video, params, per_volume=per_volume)
            # same numbers first (noise off: the two draw different noise): faster and different is not faster
            quiet = CTAugment(seed=0, noise_sigma=(0.0, 0.0)).draw(step=0, B=B, n_views=V)
            f = augment_volume(video[:1], quiet.pack()[:, :1].contiguous().cuda())
            quiet.matrix, quiet.gain, quiet.shift, quiet.sigma = (t[:, :1] for t in (quiet.matrix, quiet.gain,
                                                                                     quiet.shift, quiet.sigma))
            p = torch_views(video[:1], quiet, noise=False)
            diff = (f.double() - p.double()).abs()
            agree = dict(max_abs=float(diff.max()), mean_abs=float(diff.mean()), unit='HU' if dtype == torch.int16 else '1')
            del f, p, diff
            for _ in range(a.warmup):
                fused()
            plain()
            torch.cuda.synchronize()
            tf, tp = [], []
            for k in range(a.reps):
                tf.append(timed(fused))
                if k < a.torch_reps:
                    tp.append(timed(plain))
            nbytes = 2.0 * V * video.numel() * video.element_size()
            floor = nbytes / HBM * 1e3
            mf, mp = statistics.median(tf), statistics.median(tp)
            res = dict(tool='augment_bench', B=B, V=V, shape=[D, H, W], dtype=name, reps=a.reps, launches=1,
                       augment_ms=round(mf, 3), augment_min_ms=round(min(tf), 3), augment_max_ms=round(max(tf), 3),
                       gbytes=round(nbytes / 1e9, 3), floor_ms=round(floor, 3), fraction_of_floor=round(floor / mf, 4),
                       tb_per_s=round(nbytes / mf / 1e9, 3), gvoxel_per_s=round(V * video.numel() / mf / 1e6, 2),
                       torch_ms=round(mp, 2), torch_min_ms=round(min(tp), 2), torch_max_ms=round(max(tp), 2),
                       torch_reps=len(tp), torch_per_volume=per_volume, speedup_vs_torch=round(mp / mf, 2),
                       agree_noise_off=agree, device=torch.cuda.get_device_name(0))
            line = json.dumps(res)
            print(line, flush=True)
            if a.log:
                os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
                with open(a.log, 'a') as fh:
                    fh.write(line + '\n')
        del video
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
