"""Zero-shot attribution maps: where in the volume a pathology's log-odds come from.

After the VQ and the mean over t (``ct_clip/ct_clip.py:724,740``) the image latent is linear in the
quantised tokens -- ``to_visual_latent`` has no bias (``:767``) -- so the zero-shot log-odds of every
pathology (``:771,805-807``, ``ctclip_inference.py:305-315``) split over the (t, h, w) token grid
without remainder.  With C the codebook, idx the code indices of volume n, W = to_visual_latent.weight
([Dl, HW * D], flatten order (h, w, d)), u^ the l2-normalised prompt latents and tau = exp(temperature):

    v_n            = W . pooled_n,       pooled_n[hw] = (1/T) sum_t C[idx[n, t, hw]]
    logit(probs)   = score[n, j, 0] - score[n, j, 1] = tau (u^[j, 0] - u^[j, 1]) . v_n / ||v_n||
    V[j, hw, :]    = W[:, hw*D:(hw+1)*D]^T (u^[j, 0] - u^[j, 1])          (once per prompt set)
    map[n, j, t, hw] = tau / (T ||v_n||) V[j, hw, :] . C[idx[n, t, hw], :]
    sum_{t, hw} map[n, j, t, hw] = logit(probs[n, j])                      (completeness)

This is not a gradient heuristic: it is the same product, summed in another order.  The operands are the
ones the forward used -- the bf16 weight image the projection reads, the f32 codebook rows behind
``pooled``, the indices the VQ chose, the norm of the projected latent -- except that the projection
rounds ``pooled`` to bf16 and the map does not (DESIGN.md §24 has the measured gap).

Cost: one extra stream of the bf16 weight per prompt set (``ctclip_attr_weights``, cached like the prompt
latents) and per batch one gather-dot over data the forward already produced (``ctclip_attr_map``): the
image tower runs once per volume, there is no backward.
"""
from __future__ import annotations

import torch

from . import kernels as K
from . import precise
from . import zero_shot as Z
from .ct_clip import require_cls_latents

WHICH = ('log_odds', 'scores')


def directions(t_raw, which='log_odds'):
    """The direction rows in latent space, from raw prompt latents [2P, Dl]: 'log_odds' [P, Dl], the
    difference of each l2-normalised (present, not present) pair; 'scores' [2P, Dl], the normalised
    prompt latents themselves."""
    if which not in WHICH:
        raise ValueError(f"which: one of {WHICH}, got {which!r}")
    u = torch.nn.functional.normalize(t_raw.float(), dim=-1)
    return (u[0::2] - u[1::2]).contiguous() if which == 'log_odds' else u.contiguous()


def to_volume(maps, patch):
    """Expand token-grid maps [..., T, Hg, Wg] to the voxel grid [..., T*pt, Hg*p1, Wg*p2] by nearest
    neighbour, divided by pt * p1 * p2: the sum over voxels equals the sum over tokens.  ``patch``:
    (temporal_patch_size, patch_height, patch_width)."""
    pt, p1, p2 = (int(x) for x in patch)
    out = maps
    for dim, rep in ((-3, pt), (-2, p1), (-1, p2)):
        out = out.repeat_interleave(rep, dim=dim)
    return out / float(pt * p1 * p2)


class ZeroShotAttribution:
    """``maps(volumes)`` for a ``zero_shot.ZeroShotClassifier`` with its prompts set."""

    def __init__(self, classifier):
        require_cls_latents(classifier.model, 'ZeroShotAttribution')
        self.classifier = classifier
        self._cache = {}        # which -> (key, t_raw the key refers to, [V chunks])

    def _weights(self, W, Wb, HW, D, which):
        """V [R, HW, D] in chunks of at most ``kernels.ATTR_MAX_ROWS`` direction rows, cached until the
        projection weight (pointer, version, weights epoch: ``CTCLIP._visual_weight_bf16``'s key) or the
        classifier's prompt latents change."""
        t_raw = self.classifier._t_raw
        in_arena = getattr(W, '_ctclip_flat', None) is not None
        key = (W.data_ptr(), W._version, K.weights_epoch() if in_arena else -1, Wb.data_ptr(), t_raw._version)
        hit = self._cache.get(which)
        if hit is None or hit[0] != key or hit[1] is not t_raw:
            dirs = directions(t_raw, which)
            Vs = [K.attr_weights(dirs[i:i + K.ATTR_MAX_ROWS], Wb, HW, D)
                  for i in range(0, dirs.shape[0], K.ATTR_MAX_ROWS)]
            self._cache[which] = hit = (key, t_raw, Vs)
        return hit[2]

    def maps(self, volumes, batch_size=8, which='log_odds', normalize=True, text_to_image=True):
        """dict(maps, probs, scores).  ``maps``: [N, P, T, Hg, Wg] f32, the split of
        ``logit(probs) = scores[..., 0] - scores[..., 1]`` over the token grid; with ``which='scores'``
        [N, P, 2, T, Hg, Wg], the split of each score.  ``normalize=False``: the raw contributions
        V . C[idx] (their sum over the grid is T d . v_n: no temperature, no 1/T, no norm).  ``probs`` /
        ``scores``: what ``classifier.predict`` returns, from the same forward."""
        cl = self.classifier
        m = cl.model
        if which not in WHICH:
            raise ValueError(f"ZeroShotAttribution.maps: which is one of {WHICH}, got {which!r}")
        if cl._t_raw is None:
            raise RuntimeError('ZeroShotAttribution: the classifier has no prompts (pass tokenizer= or call '
                               'set_prompts)')
        if precise.vit_precision() != 'bf16':
            raise NotImplementedError('ZeroShotAttribution: the f32 image-tower modes project with the f32 weight; '
                                      'the maps decompose the bf16 projection only')
        if not text_to_image and getattr(m, 'extra_latent_projection', False):
            raise NotImplementedError('ZeroShotAttribution: text_to_image=False with extra_latent_projection scores '
                                      'the extra latents, which the classifier does not use')
        vt = m.visual_transformer
        log_temp = m.temperature.detach().reshape(1)
        P = len(cl.pathologies)
        out, probs, scores = [], [], []
        with torch.no_grad(), Z._eval(m):
            for i in range(0, volumes.shape[0], batch_size):
                pooled, pooled_b = vt.encode_pooled(volumes[i:i + batch_size])      # the image tower, once
                idx = vt.vq.state.last_indices
                W = m.to_visual_latent.weight
                Wb = m._visual_weight_bf16(W)
                i_raw = m._project(W, Wb, pooled, pooled_b)
                p, s = K.zero_shot(cl._t_raw, i_raw, log_temp)
                embed = vt._codebook_tensors()[0]
                cb = embed.view(-1, embed.shape[-1])
                B = pooled.shape[0]
                hg, wg = vt.patch_height_width
                HW, D = hg * wg, cb.shape[1]
                T = idx.numel() // (B * HW)
                norm = (i_raw.float().contiguous(), log_temp.float()) if normalize else (None, None)
                parts = [K.attr_map(V, idx, cb, B, T, HW, *norm) for V in self._weights(W, Wb, HW, D, which)]
                mp = parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)
                out.append(mp.view(B, P, T, hg, wg) if which == 'log_odds' else mp.view(B, P, 2, T, hg, wg))
                probs.append(p)
                scores.append(s)
        return dict(maps=torch.cat(out), probs=torch.cat(probs), scores=torch.cat(scores))
