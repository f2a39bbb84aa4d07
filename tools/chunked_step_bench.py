"""Throughput and peak memory of the chunked train step (CTClipTrainer.train_step_chunked, DESIGN.md
§21) at the base config on one GPU, beside the one-shot train_step of the same session:

  one-shot B = 16 | chunked Bg = 16 / chunk 8 | Bg = 64 / chunk 16 | Bg = 256 / chunk 16, the volumes in
  pinned host memory (one chunk on the device at a time)

Per case: --warmup untimed steps, then --steps steps timed one by one (synchronised before and after
each, flush() inside the timed region so a step's deferred work is counted), the median step time,
pairs/s, the ratio to the one-shot rate and torch's peak allocation over the timed steps.  One JSON
line per case.  python tools/chunked_step_bench.py [--steps 5] [--warmup 2] [--cases one16,c16x8,...]"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'ctpa-clip_amd'))

CASES = {            # name -> (Bg, chunk or None for the one-shot step, volumes on the host)
    'one16': (16, None, False),
    'c16x8': (16, 8, False),
    'c64x16': (64, 16, False),
    'c256x16host': (256, 16, True),
}


def inputs(Bg, L, dev, host, distinct=16, frames=240, size=480, vocab=30522):
    """Bg reports and volumes; the volumes repeat `distinct` random ones (the loss is not the point here)."""
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    n = min(Bg, distinct)
    base = torch.randint(-1200, 1201, (n, 1, frames, size, size), generator=g, device=dev,
                         dtype=torch.int32).to(torch.int16)
    if host:
        hu = torch.empty((Bg,) + tuple(base.shape[1:]), dtype=torch.int16, pin_memory=True)
    else:
        hu = torch.empty((Bg,) + tuple(base.shape[1:]), dtype=torch.int16, device=dev)
    for r in range(0, Bg, n):
        hu[r:r + n].copy_(base[:min(n, Bg - r)])
    g.manual_seed(4321)
    ids = torch.randint(5, vocab, (Bg, L), generator=g, device=dev)
    ids[:, 0], ids[:, -1] = 2, 3
    torch.cuda.synchronize()
    return hu, types.SimpleNamespace(input_ids=ids, attention_mask=torch.ones(Bg, L, dtype=torch.long, device=dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--text-len', type=int, default=128)
    ap.add_argument('--cases', default=','.join(CASES))
    a = ap.parse_args()
    from ctclip_mi355x.models import build_ctclip, set_finetune_trainable
    from ctclip_mi355x.trainer import CTClipTrainer
    dev = torch.device('cuda', 0)
    torch.cuda.set_device(dev)
    torch.manual_seed(0)
    model = set_finetune_trainable(build_ctclip()).to(dev)
    model.train()
    tr = CTClipTrainer(model)
    base_rate = None
    for name in a.cases.split(','):
        Bg, chunk, host = CASES[name]
        hu, text = inputs(Bg, a.text_len, dev, host)
        step = (lambda: tr.train_step(text, hu)) if chunk is None else (lambda: tr.train_step_chunked(text, hu, chunk))
        for _ in range(a.warmup):
            step()
        tr.flush()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        resting = torch.cuda.memory_allocated(dev)
        times = []
        for _ in range(a.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            loss = step()
            tr.flush()
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
        med = statistics.median(times)
        rate = Bg / med
        if chunk is None:
            base_rate = rate
        print(json.dumps({
            'case': name, 'Bg': Bg, 'chunk': chunk, 'volumes': 'pinned host' if host else 'device',
            'median_step_ms': round(med * 1e3, 2), 'min_step_ms': round(min(times) * 1e3, 2),
            'max_step_ms': round(max(times) * 1e3, 2), 'pairs_per_s': round(rate, 2),
            'vs_one_shot': round(rate / base_rate, 4) if base_rate else None,
            'peak_alloc_GiB': round(torch.cuda.max_memory_allocated(dev) / 2 ** 30, 2),
            'peak_above_resting_GiB': round((torch.cuda.max_memory_allocated(dev) - resting) / 2 ** 30, 2),
            'resting_GiB (weights, moments, inputs on the device)': round(resting / 2 ** 30, 2),
            'loss': float(loss.reshape(-1)[0].item()), 'steps': a.steps, 'warmup': a.warmup}), flush=True)
        del hu, text, step
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
