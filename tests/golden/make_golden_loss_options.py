"""Golden fixture for the reference's loss options: decoupled contrastive learning, the extra
(CLOOB) latent projection and image multiview (ct_clip/ct_clip.py:663-675, 780-790, 845-899).

Run in the build container only (needs the reference checkout, see make_golden.py):
    python tests/golden/make_golden_loss_options.py

The reference's own CTCLIP runs the tiny configuration (oracle.TINY, B = 4, 16 ragged tokens,
name-seeded recipe weights) four times -- plain, DCL, extra projection, DCL + extra + 2 augmented
image views (W.make_hu(seed=100 + k)) -- and this script records, per case: the loss, the latent
sets of return_latents (all views), the eval scores for both text_to_image values, and the
gradients of the projection weights and the temperature.  The inputs of the projections (BERT's
CLS rows, the pooled image tokens of all three views) are stored once: together with the recipe
weights they let a test rebuild the raw latents without running the towers.

The fixture is DATA (expected outputs); nothing of the reference's source is copied into it.
"""
from __future__ import annotations

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402  (sets up sys.path for oracle/)
import torch  # noqa: E402
from safetensors.torch import save_file  # noqa: E402

from oracle import ctclip_oracle as O  # noqa: E402
from oracle import weights as W  # noqa: E402

# tag, decoupled_contrastive_learning, extra_latent_projection, augmented image views
CASES = (('plain', False, False, 0), ('dcl', True, False, 0), ('extra', False, True, 0), ('all', True, True, 2))
PROJ = ('to_text_latent.weight', 'to_visual_latent.weight', 'to_text_latent_extra.weight',
        'to_visual_latent_extra.weight', 'temperature')
BATCH, TEXT_LEN = 4, 16


def main():
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    _, V, C = G.import_reference()
    cfg = O.TINY
    sd = W.make_state_dict(cfg)
    video = O.normalize_hu(W.make_hu(BATCH, cfg.vit))
    ids, mask = W.make_text(BATCH, TEXT_LEN, cfg.bert.vocab_size, ragged=True)
    text = G._Text(ids, mask)
    out, mv_weight = {}, None
    for tag, dcl, extra, naug in CASES:
        clip = G.build_reference(cfg, V, C)
        clip.load_state_dict(sd, strict=True)
        clip.decoupled_contrastive_learning = dcl
        clip.extra_latent_projection = extra
        mv_weight = float(clip.multiview_loss_weight)
        aug = tuple(O.normalize_hu(W.make_hu(BATCH, cfg.vit, seed=100 + k)) for k in range(naug)) or None
        cap = {}
        hooks = [clip.to_text_latent.register_forward_pre_hook(lambda m, i: cap.__setitem__('cls', i[0].detach().clone())),
                 clip.to_visual_latent.register_forward_pre_hook(
                     lambda m, i: cap.__setitem__('pooled', i[0].detach().clone()))]
        clip.train()
        loss = clip(text, video, device='cpu', return_loss=True, aug_image=aug)
        loss.backward()
        for h in hooks:
            h.remove()
        out[f'{tag}.loss'] = loss.detach().reshape(1)
        named = dict(clip.named_parameters())
        for n in PROJ:
            if named[n].grad is not None:
                out[f'{tag}.grad.{n}'] = named[n].grad.detach().clone()
        if naug == 2:
            out['in.cls'], out['in.pooled'] = cap['cls'], cap['pooled']     # pooled: view-major, 3 views
        elif 'in.cls' in out:
            assert torch.equal(out['in.cls'], cap['cls'])
        # latents of every view (train mode, codebook restored: the quantised values do not depend on it)
        clip.load_state_dict(sd, strict=True)
        with torch.no_grad():
            lat = clip(text, video, device='cpu', return_loss=True, return_latents=True, aug_image=aug)
        names = ('text', 'image', 'text_extra', 'image_extra') if extra else ('text', 'image')
        assert len(lat) == (4 if extra else 3)
        for n, t in zip(names, lat):
            out[f'{tag}.latents.{n}'] = t.detach().clone()
        clip.load_state_dict(sd, strict=True)
        clip.eval()
        with torch.no_grad():
            out[f'{tag}.scores.t2i'] = clip(text, video, device='cpu').detach().clone()
            out[f'{tag}.scores.i2t'] = clip(text, video, device='cpu', text_to_image=False).detach().clone()
        print(tag, 'loss', float(loss.detach()), 'keys', sum(k.startswith(tag) for k in out))
    path = os.path.join(HERE, 'golden_loss_options.safetensors')
    save_file({k: v.contiguous() for k, v in out.items()}, path,
              metadata={'batch': str(BATCH), 'text_len': str(TEXT_LEN), 'multiview_loss_weight': repr(mv_weight),
                        'generator': 'tests/golden/make_golden_loss_options.py',
                        'reference': 'sharonct/CTPA-CLIP @ 2025-06-20 (ct_clip/ct_clip.py:614-901)'})
    print('->', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
