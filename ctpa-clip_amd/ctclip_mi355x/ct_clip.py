"""CTCLIP (ct_clip/ct_clip.py:407-901) — drop-in constructor / forward signature and state_dict
layout, with the image tower, text tower, projections and InfoNCE running on HIP kernels.

Supported configuration = the one the reference trains (pretrained_model.py:31-42): external
image / text encoders, use_mlm=False, use_visual_ssl=False, use_all_token_embeds=False,
downsample_image_embeds=False -- plus the reference's three loss options that run with external
encoders: decoupled_contrastive_learning (ct_clip.py:865-867), extra_latent_projection (CLOOB,
:780-790,:848-849: the image -> text direction, ``text_to_image=False`` scores and the 4-tuple of
``return_latents`` use to_text_latent_extra / to_visual_latent_extra) and image multiview
(``aug_image=``, :663-675,:882-899).  The plain configuration runs ``functional.ClipLossFn`` on the
one-workgroup kernel as before; any of the three options switches the loss to
``functional.ClipLossExFn`` (one workgroup per view pair + a fixed-order reduction).
Above 128 gathered rows both Functions take the tiled MFMA loss (``functional.set_loss_tiled``).
``use_all_token_embeds`` (the fine-grained FILIP loss, :751-755,:829-843) takes a branch of its own,
``_forward_filip`` on ``functional.FilipLossFn`` (csrc/filip.hip): every report token
against every spatial image token, one view, no extra projection, one rank.
``sigmoid_loss=True`` (not in the reference) trains the pairwise sigmoid (SigLIP) loss instead of InfoNCE:
``functional.SigmoidLossFn`` on csrc/loss_sigmoid.hip with a learned scalar ``logit_bias``;
one text and one image view, no extra projection, no DCL, no token-wise loss -- those combinations raise.
``multi_positive=True`` (not in the reference) trains the duplicate-report-aware InfoNCE: the positives of a row
are all rows of the global batch with its id -- ``forward(pair_ids=...)`` or, by default, a hash of the report's
kept tokens made on the device (``kernels.report_ids``) -- on ``functional.MultiPosLossFn`` and
csrc/loss_multipos.hip; one text and one image view, no other loss option.
``visual_ssl=VisualSSLHead(dim_latent)`` adds the SimSiam loss of the last two image views' raw latents with
``image_ssl_loss_weight`` (visual_ssl.py, csrc/ssl.hip); ``use_visual_ssl=True`` without a head (the
reference's built-in 2-D SimSiam / SimCLR) raises.
``aug_text`` (the reference itself cannot run it: it calls ``.shape`` on a BatchEncoding) and
everything else raises.
"""
from __future__ import annotations

import copy
import os
from pathlib import Path

import torch
from torch import nn

from . import dist_sync
from . import functional as Fn
from . import streams
from .visual_ssl import VisualSSLHead


# queue BERT's forward before the image tower's (A/B switch, default: image tower first)
TEXT_FWD_FIRST = os.environ.get('CTCLIP_TEXT_FWD_FIRST', '0') != '0'
# BERT's forward (text stream) starts after the image tower's patch embedding instead of with it: the
# patch LayerNorm is HBM-bound (0.43 ms alone, ~1.1 ms beside BERT's first kernels in round 4) and BERT
# is hidden behind the 3D-ViT either way.  CTCLIP_TEXT_GATE=0: start together (A/B).
TEXT_GATE = os.environ.get('CTCLIP_TEXT_GATE', '1') != '0'
# where the training VQ's codebook EMA update is queued on the auxiliary stream (A/B): '0' right
# after the VQ (its ~0.34 ms of short workgroups then hold the CUs the projection's slab reduction
# waits for: 5 -> 321 us in step, r05f_seq.txt), '1' after the image projection (the loss kernel and
# the backward's first launches wait instead), '2' (default) after the optimizer step, beside the
# next step's forward -- only when CTClipTrainer owns the step (train_step sets ema_after_step,
# optimizer_step calls flush_ema; any codebook reader, the next VQ or state_dict, queues a pending
# update first); a plain model(...) call in train mode gets site '1', so the codebook read after it
# is the updated one, as the reference updates it inside forward.  Measured (r05m_ema_site_ab.log):
# '2' 204.30 vs '1' 203.70 pairs/s; '1' vs '0' within noise (r05g_ema_ab_env.log).  '3' (round 6): as
# '2', but the trainer leaves the update pending and the NEXT step's image tower queues it once its
# patch embedding is queued (ctvit.encode_tokens), so it runs beside the GEMM-bound first layer
# instead of beside the HBM-bound patch LayerNorm (any codebook reader still queues it first)
DEFER_EMA = os.environ.get('CTCLIP_DEFER_EMA', '2')


class _nullctx:
    def __enter__(self):
        return self

    def __exit__(self, *exc):
        return False


def l2norm(t):
    return nn.functional.normalize(t, dim=-1)


def require_cls_latents(model, who):
    """The evaluators (zero-shot, retrieval, attribution, linear probe) score ONE latent per report and
    volume: a ``use_all_token_embeds`` model, whose heads project tokens, is refused by name."""
    if getattr(model, 'use_all_token_embeds', False):
        raise NotImplementedError(f'{who} with CTCLIP(use_all_token_embeds=True): the model has no pooled latent '
                                  'pair (its projections act on tokens)')


class CTCLIP(nn.Module):
    def __init__(self, *, image_encoder=None, text_encoder=None, dim_text=512, dim_image=512, dim_latent=512,
                 num_text_tokens=28897, text_enc_depth=6, text_seq_len=256, text_heads=8, text_dim_head=64,
                 text_has_cls_token=False, text_pad_id=0, text_rotary_pos_emb=False, text_causal_mask=False,
                 text_eos_id=None, text_encode_without_mask=False, visual_enc_depth=6, visual_heads=8,
                 visual_dim_head=64, visual_image_size=256, visual_patch_size=32, visual_patch_dropout=0.5,
                 visual_has_cls_token=False, channels=3, use_all_token_embeds=False, downsample_image_embeds=False,
                 decoupled_contrastive_learning=False, extra_latent_projection=False, use_mlm=False,
                 text_ssl_loss_weight=0.05, use_visual_ssl=False, visual_ssl=None, visual_ssl_type='simsiam',
                 visual_ssl_hidden_layer=-1, simclr_temperature=0.1, image_ssl_loss_weight=0.05,
                 multiview_loss_weight=0.1, checkpoint_during_training=False, sigmoid_loss=False,
                 sigmoid_bias_init=-10.0, sigmoid_temperature_init=None, multi_positive=False, **kwargs):
        """``sigmoid_loss``: train the pairwise sigmoid loss (Zhai et al. 2023) instead of InfoNCE; the model
        then owns a scalar parameter ``logit_bias`` (``sigmoid_bias_init``), absent otherwise, so the default
        ``state_dict`` keys stay the reference's.  ``temperature`` (log scale) keeps its constructor value 1
        unless ``sigmoid_temperature_init`` is given; the paper initialises temperature = log 10, bias = -10.
        ``multi_positive``: InfoNCE whose positives are all pairs of one group (identical reports by default,
        ``forward(pair_ids=)`` otherwise); no parameter and no ``state_dict`` key is added."""
        super().__init__()
        if multi_positive:
            refused = dict(sigmoid_loss=sigmoid_loss, decoupled_contrastive_learning=decoupled_contrastive_learning,
                           extra_latent_projection=extra_latent_projection,
                           use_all_token_embeds=use_all_token_embeds,
                           visual_ssl=visual_ssl is not None)
            for name, on in refused.items():
                if on:
                    raise NotImplementedError(f'CTCLIP: multi_positive with {name} (the multi-positive loss has '
                                              'one latent pair and the plain softmax denominators)')
        if sigmoid_loss:
            refused = dict(decoupled_contrastive_learning=decoupled_contrastive_learning,
                           extra_latent_projection=extra_latent_projection,
                           use_all_token_embeds=use_all_token_embeds)
            for name, on in refused.items():
                if on:
                    raise NotImplementedError(f'CTCLIP: sigmoid_loss with {name} (the pairwise sigmoid loss has '
                                              'one latent pair and no softmax denominator)')
        # use_all_token_embeds projects ONE spatial token of the image tower: the tower has to state its token
        # width (``.dim``, as CTViT does) and ``dim_image`` has to be that width.  With the flattened width
        # (h w d, the CLS configuration's) the pooled volume would be taken for a single token without an error
        token_width = getattr(image_encoder, 'dim', None)
        no_tokens = bool(use_all_token_embeds) and (token_width is None or int(token_width) != int(dim_image))
        # visual self-supervision runs with a prebuilt VisualSSLHead only: the reference's built-in SimSiam /
        # SimCLR (use_visual_ssl=True without a head) and any other visual_ssl object wrap a 2-D tower
        head = visual_ssl if isinstance(visual_ssl, VisualSSLHead) else None
        unsupported = dict(use_all_token_embeds=no_tokens, downsample_image_embeds=downsample_image_embeds,
                           use_mlm=use_mlm,
                           use_visual_ssl=(use_visual_ssl or visual_ssl is not None) and head is None,
                           text_causal_mask=text_causal_mask)
        bad = [k for k, v in unsupported.items() if v]
        if bad:
            hint = (f' (use_all_token_embeds needs an image encoder whose token width ``.dim`` equals dim_image = '
                    f'{dim_image}, got {token_width}; models.build_ctclip sets it)') if no_tokens else ''
            raise NotImplementedError(f'CTCLIP options outside the contrastive hot path: {bad}{hint}')
        if image_encoder is None or text_encoder is None:
            raise NotImplementedError('the built-in VisionTransformer / TextTransformer are never used by the '
                                      'reference (pretrained_model.py:31-42); pass image_encoder and text_encoder')
        if use_all_token_embeds and extra_latent_projection:
            raise NotImplementedError('CTCLIP: use_all_token_embeds with extra_latent_projection (the fine-grained '
                                      'loss has one latent pair)')
        self.use_all_token_embeds = bool(use_all_token_embeds)
        # use_all_token_embeds: the image -> text denominator over the texts (the FILIP paper) instead of over
        # the images (the reference, inherited from x-clip); see functional.FilipLossFn
        self.filip_i2t_over_text = False
        self.dim_text = dim_text
        self.dim_image = dim_image
        self.dim_latent = dim_latent
        self.text_transformer = text_encoder
        self.visual_transformer = image_encoder
        self.to_text_latent = nn.Linear(dim_text, dim_latent, bias=False)
        self.to_visual_latent = nn.Linear(dim_image, dim_latent, bias=False)
        self.temperature = nn.Parameter(torch.tensor(1. if sigmoid_temperature_init is None or not sigmoid_loss
                                                     else float(sigmoid_temperature_init)))
        self.sigmoid_loss = bool(sigmoid_loss)
        if self.sigmoid_loss:
            self.logit_bias = nn.Parameter(torch.tensor(float(sigmoid_bias_init)))
        self.multi_positive = bool(multi_positive)
        if self.multi_positive:
            self.last_positive_count = None      # the detached [1] int32 npos of the last forward, for logging
        self.extra_latent_projection = extra_latent_projection
        self.decoupled_contrastive_learning = decoupled_contrastive_learning
        self.to_text_latent_extra = copy.deepcopy(self.to_text_latent)
        self.to_visual_latent_extra = copy.deepcopy(self.to_visual_latent)
        self.multiview_loss_weight = multiview_loss_weight
        self.visual_ssl = None
        if head is not None:
            for name, on in dict(sigmoid_loss=sigmoid_loss, use_all_token_embeds=use_all_token_embeds).items():
                if on:
                    raise NotImplementedError(f'CTCLIP: visual_ssl with {name} (no image views there for the '
                                              'self-supervised pair)')
            if int(head.dim) != int(dim_latent):
                raise ValueError(f'CTCLIP: the VisualSSLHead acts on the raw image latents, its dim {head.dim} '
                                 f'must equal dim_latent {dim_latent}')
            # registered only with a head, so the default state_dict keys stay the reference's.  The weight is
            # image_ssl_loss_weight as given (the reference zeroes it unless use_visual_ssl is set too)
            self.visual_ssl = head
            self.image_ssl_loss_weight = float(image_ssl_loss_weight)
            self.last_image_ssl_loss = None      # the detached [1] loss of the last forward, for logging
        self._wvis = {}                    # bf16 casts of the visual projections, a slot per weight
        self.defer_text_backward = False     # set by CTClipTrainer (see encode)
        self._deferred_text = None
        self._deferred_image = None
        self._deferred_text_extra = None     # the same for the extra (CLOOB) projections' latents
        self._deferred_image_extra = None
        self._extra_raw = (None, None)       # encode's raw extra latents (extra_latent_projection)
        self._t_gather = None
        self.ema_after_step = False          # set by CTClipTrainer.train_step (DEFER_EMA '2')

    # ------------------------------------------------------------------ checkpoint
    def load(self, path):
        """``CTCLIP.load`` (ct_clip/ct_clip.py:593-597): strict=False; weights-only safe loader."""
        path = Path(path)
        assert path.exists()
        pt = torch.load(str(path), map_location='cpu', weights_only=True)
        return self.load_state_dict(pt, strict=False)

    def state_dict(self, *args, **kwargs):
        """The reference key layout; a text-tower Adam the trainer deferred to the next step
        (CTClipTrainer(defer_text_adam=True)) is queued first, and the caller's stream is ordered
        after the text stream (BERT's Adam) and the auxiliary stream (the codebook EMA), so the
        tensors returned -- and any copy of them queued on the current stream, e.g. torch.save --
        hold the updated weights."""
        if self._vq_state() is not None:
            self._vq_state().flush_ema()
        for p in self.text_transformer.parameters():
            if p.is_cuda:
                streams.flush_text(p.device)
                streams.join_text(p.device)
                streams.join_aux(p.device)
            break
        return super().state_dict(*args, **kwargs)

    # ------------------------------------------------------------------ helpers
    def _vq_state(self):
        """The image tower's VQ cache (functional.VQState), or None for another image encoder."""
        return getattr(getattr(self.visual_transformer, 'vq', None), 'state', None)

    def flush_ema(self):
        """Queue a deferred codebook EMA update now (auxiliary stream; see DEFER_EMA)."""
        vqs = self._vq_state()
        if vqs is not None:
            vqs.flush_ema()

    def set_ema_mode(self, mode):
        """What a train-mode image tower does with the codebook EMA (functional.VQState.ema_mode):
        None updates it in every call, 'skip' withholds it, 'hold' adds the call's rows to held
        statistics that ``apply_held_ema`` turns into ONE update (``drop_held_ema`` forgets them).
        Returns the previous mode.  The chunked step's two passes (CTClipTrainer.train_step_chunked)."""
        if mode not in (None, 'skip', 'hold'):
            raise ValueError(f"CTCLIP.set_ema_mode: None, 'skip' or 'hold', got {mode!r}")
        vqs = self._vq_state()
        if vqs is None:
            return None
        old, vqs.ema_mode = vqs.ema_mode, mode
        return old

    def apply_held_ema(self):
        vqs = self._vq_state()
        if vqs is not None:
            vqs.apply_held_ema()

    def drop_held_ema(self):
        vqs = self._vq_state()
        if vqs is not None:
            vqs.drop_held_ema()

    def _visual_weight_bf16(self, W):
        """bf16 to_visual_latent (or to_visual_latent_extra) weight (151 M parameters): the Adam-kept
        shadow when W trains, else a cast cached until W changes (one cache slot per weight).  Frozen
        in the fine-tune configuration (fine_tuning_ctclip.py:6-14), so it is cast once, not every
        step (0.23 ms per recast)."""
        from . import kernels as K
        from . import functional as Fn
        sh = Fn.shadow_bf16(W)
        if sh is not None:
            return sh
        # only an optimizer arena member is written behind torch's version counter (raw pointers)
        in_arena = getattr(W, '_ctclip_flat', None) is not None
        key = (W.data_ptr(), W._version, K.weights_epoch() if in_arena else -1)
        slot = 'extra' if W is self.to_visual_latent_extra.weight else 'main'
        if self._wvis.get(slot, (None, None))[0] != key:
            self._wvis[slot] = (key, K.cast_bf16(W.detach().contiguous()))
        return self._wvis[slot][1]

    def _project(self, W, Wb, pooled, pooled_b):
        # (in the f32 image-tower mode ImageProjFn's forward is the exact-f32 product, precise.py)
        return Fn.ImageProjFn.apply(pooled, pooled_b, W, Wb)

    def encode(self, text, image, gather=False, stack=False):
        """Text + image towers and raw latents: (enc_text (B,L,768), pooled (B, h*w*d),
        text_raw (B, dl), image_raw (B, dl)).  ``gather``: the caller will compute the global-batch
        loss, so under torch.distributed the text latents' all-gather starts here (every rank makes
        the same call); other callers (scores, encodings) issue no collective.  ``stack``: that loss
        is ``ClipLossExFn``, whose gathers are view stacks (the extra text latents ride the same
        collective).  With ``extra_latent_projection`` the raw latents of to_text_latent_extra /
        to_visual_latent_extra are left in ``self._extra_raw``.  ``image`` may hold several views
        concatenated on the batch axis (forward's ``aug_image``)."""
        # The host queues the image tower first (its ~16 ms of GPU work keep this stream busy while
        # the host queues BERT's many small launches), BERT on the text stream (streams.py) ordered
        # only after an event taken before the image tower, so the two run side by side.
        dev = image.device
        ready = torch.cuda.current_stream(dev).record_event() if streams.text_stream(dev) else None
        if TEXT_FWD_FIRST:      # A/B: BERT's launches queued before the image tower's
            enc_text = self.text_transformer(text.input_ids, attention_mask=text.attention_mask, join=False,
                                             ready=ready)[0]
            pooled, pooled_b = self.visual_transformer.encode_pooled(image)
        else:
            vqs = self._vq_state()
            if vqs is not None:
                vqs.defer_ema = DEFER_EMA != '0' and self.visual_transformer.training
            try:
                pooled, pooled_b = self.visual_transformer.encode_pooled(image)
            finally:
                if vqs is not None:
                    vqs.defer_ema = False
            gate = getattr(self.visual_transformer, '_patch_done', None)
            if TEXT_GATE and ready is not None and gate is not None:
                ready = gate
            enc_text = self.text_transformer(text.input_ids, attention_mask=text.attention_mask, join=False,
                                             ready=ready)[0]
        ts = streams.text_stream(dev)
        with torch.cuda.stream(ts) if ts is not None else _nullctx():
            cls = enc_text[:, 0, :].contiguous()
            t_raw = Fn.TextProjFn.apply(cls, self.to_text_latent.weight)
            t_extra = Fn.TextProjFn.apply(cls, self.to_text_latent_extra.weight) if self.extra_latent_projection else None
            # N > 1: the text latents' all-gather goes out from the text stream now, beside the
            # 3D-ViT forward still running on the main stream (SURVEY 8(e) overlap)
            self._t_gather = None
            if gather and dist_sync.world_rank()[0] > 1:
                if stack:
                    sets = [t_raw[None]] + ([t_extra[None]] if t_extra is not None else [])
                    self._t_gather = dist_sync.start_gather_stacks(sets)
                else:
                    self._t_gather = dist_sync.start_gather(t_raw)
        streams.join_text(dev)
        if ts is not None:
            t_raw.record_stream(torch.cuda.current_stream(dev))
            if t_extra is not None:
                t_extra.record_stream(torch.cuda.current_stream(dev))
        self._deferred_text_extra = self._deferred_image_extra = None
        if self.defer_text_backward and torch.is_grad_enabled() and t_raw.requires_grad:
            # the trainer back-propagates the text tower AFTER the loss / 3D-ViT graph
            # (CTClipTrainer.forward_backward): the long ViT chain is queued first, and BERT's
            # backward, queued while the GPU still works through it, runs beside it on the text
            # stream -- ordered only after an event taken when the loss produced its gradient
            leaf = t_raw.detach().requires_grad_(True)
            d = self._deferred_text = [t_raw, leaf, None]
            if ts is not None:
                def mark(g):
                    d[2] = torch.cuda.current_stream(dev).record_event()
                leaf.register_hook(mark)
            t_raw = leaf
        if self.defer_text_backward and torch.is_grad_enabled() and t_extra is not None and t_extra.requires_grad:
            # the extra projection's latents are cut the same way; backward_deferred_text walks
            # BERT once from both
            xleaf = t_extra.detach().requires_grad_(True)
            dx = self._deferred_text_extra = [t_extra, xleaf, None]
            if ts is not None:
                def mark_x(g):
                    dx[2] = torch.cuda.current_stream(dev).record_event()
                xleaf.register_hook(mark_x)
            t_extra = xleaf
        W = self.to_visual_latent.weight
        i_raw = self._project(W, self._visual_weight_bf16(W), pooled, pooled_b)
        i_extra = None
        if self.extra_latent_projection:
            Wx = self.to_visual_latent_extra.weight
            i_extra = self._project(Wx, self._visual_weight_bf16(Wx), pooled, pooled_b)
        if DEFER_EMA == '1' or (DEFER_EMA in ('2', '3') and not self.ema_after_step):
            self.flush_ema()               # the codebook EMA, after the projection
        if self.defer_text_backward and torch.is_grad_enabled() and i_raw.requires_grad:
            # the image tower's backward is deferred too (CTClipTrainer.forward_backward): BERT's
            # backward -- and its gradient buckets' all-reduces -- are queued before the 3D-ViT's
            ileaf = i_raw.detach().requires_grad_(True)
            self._deferred_image = [i_raw, ileaf]
            i_raw = ileaf
        if self.defer_text_backward and torch.is_grad_enabled() and i_extra is not None and i_extra.requires_grad:
            xileaf = i_extra.detach().requires_grad_(True)
            self._deferred_image_extra = [i_extra, xileaf]
            i_extra = xileaf
        self._extra_raw = (t_extra, i_extra)
        return enc_text, pooled, t_raw, i_raw

    def forward(self, text, image, device=None, return_loss=False, return_encodings=False, return_latents=False,
                freeze_image_encoder=False, freeze_text_encoder=False, text_to_image=True, aug_text=None,
                aug_image=None, pair_ids=None):
        """``CTCLIP.forward`` (ct_clip/ct_clip.py:614-901).  ``aug_image``: a tensor or a tuple of
        tensors shaped like ``image`` (int16 HU or f32), extra views of the same volumes: all views go
        through the image tower in one call (the VQ EMA sees them all, as in the reference) and each
        view's contrastive loss is mixed in with ``multiview_loss_weight`` (:882-899).  ``pair_ids`` (a
        ``multi_positive`` model with ``return_loss``): int64 [B] group ids, on host or device, global in
        meaning -- every rank must agree on what an id names (a hash of an accession number, say); without
        them the ids are ``kernels.report_ids`` of the reports.  ``last_positive_count`` then holds the
        global number of ordered positive pairs off the diagonal ([1] int32, on the device)."""
        if aug_text is not None:
            raise NotImplementedError('multiview augmentation is off in the reference configuration')
        if pair_ids is not None and not self.multi_positive:
            raise ValueError('CTCLIP: pair_ids without multi_positive=True (the other losses take the diagonal '
                             'as the only positives)')
        if self.multi_positive and aug_image is not None:
            raise NotImplementedError('CTCLIP: multi_positive with aug_image (the multi-positive loss has one '
                                      'image view)')
        if self.use_all_token_embeds:
            if aug_image is not None:
                raise NotImplementedError('CTCLIP: use_all_token_embeds with aug_image (the fine-grained loss has '
                                          'one image view)')
            return self._forward_filip(text, image, return_loss, return_encodings, return_latents)
        if self.sigmoid_loss and aug_image is not None:
            raise NotImplementedError('CTCLIP: sigmoid_loss with aug_image (the pairwise sigmoid loss has one '
                                      'image view)')
        n_views = 1
        if aug_image is not None:
            aug = tuple(aug_image) if isinstance(aug_image, (tuple, list)) else (aug_image,)
            assert all(a.shape == image.shape and a.dtype == image.dtype for a in aug), \
                'every augmented view has the shape and dtype of image'
            n_views = len(aug) + 1
            image = torch.cat((image, *aug), dim=0)
        is_multiview = n_views > 1
        assert not (not return_loss and is_multiview), 'do not pass in augmented texts or images if not training'
        assert not (self.multiview_loss_weight == 0 and is_multiview), \
            'multiview loss weight cannot be 0 if augmented text or images passed in'
        extra = self.extra_latent_projection
        # visual self-supervision: the SimSiam head on the last two image views' raw latents
        use_ssl = self.visual_ssl is not None and return_loss and not (return_latents or return_encodings)
        if use_ssl:
            if not is_multiview:
                raise ValueError('CTCLIP: visual_ssl needs aug_image with return_loss (the self-supervised pair '
                                 'is the last two image views)')
            if dist_sync.world_rank()[0] > 1:
                raise NotImplementedError('CTCLIP: visual_ssl under torch.distributed with world size > 1 (the '
                                          'BatchNorm statistics and the 1 / world gradient scale are not defined)')
        if return_latents:
            enc_text = self.text_transformer(text.input_ids, attention_mask=text.attention_mask)[0]
            tokens = self.visual_transformer(image, return_encoded_tokens=True)
            pooled, pooled_b = self._pool_tokens(tokens)
            cls = enc_text[:, 0, :].contiguous()
            t_raw = Fn.TextProjFn.apply(cls, self.to_text_latent.weight)
            W = self.to_visual_latent.weight
            i_raw = self._project(W, self._visual_weight_bf16(W), pooled, pooled_b)
            if extra:      # ct_clip.py:789-790: the 4-tuple, no tokens
                Wx = self.to_visual_latent_extra.weight
                t_extra = Fn.TextProjFn.apply(cls, self.to_text_latent_extra.weight)
                i_extra = self._project(Wx, self._visual_weight_bf16(Wx), pooled, pooled_b)
                return l2norm(t_raw), l2norm(i_raw), l2norm(t_extra), l2norm(i_extra)
            return l2norm(t_raw), l2norm(i_raw), tokens
        self._t_gather = None
        # the plain configuration keeps the one-workgroup loss (ClipLossFn); any option takes ClipLossExFn
        general = extra or self.decoupled_contrastive_learning or is_multiview
        enc_text, pooled, t_raw, i_raw = self.encode(text, image, gather=return_loss and not return_encodings,
                                                     stack=general)
        (t_extra, i_extra), self._extra_raw = self._extra_raw, (None, None)
        if return_encodings:
            return enc_text, pooled
        if not return_loss:
            from . import kernels as K
            if extra and not text_to_image:     # ct_clip.py:806: the image -> text latents
                t_raw, i_raw = t_extra, i_extra
            scores = K.clip_scores(t_raw.contiguous(), i_raw.contiguous(), self.temperature.detach().reshape(1))
            # sigmoid_loss: the logits the loss trains (the bias cancels in the evaluators' softmax / ranks)
            return scores + self.logit_bias.detach() if self.sigmoid_loss else scores
        tg, self._t_gather = self._t_gather, None
        if self.sigmoid_loss:
            return Fn.SigmoidLossFn.apply(t_raw, i_raw, self.temperature, self.logit_bias, None, tg)
        if self.multi_positive:
            from . import kernels as K
            B = t_raw.shape[0]
            if pair_ids is None:
                ids = K.report_ids(text.input_ids, text.attention_mask)
            else:
                if not torch.is_tensor(pair_ids) or pair_ids.dtype != torch.int64 or pair_ids.shape != (B,):
                    raise ValueError(f'CTCLIP: pair_ids must be an int64 tensor [{B}]')
                ids = pair_ids.to(t_raw.device).contiguous()
            loss, npos = Fn.MultiPosLossFn.apply(t_raw, i_raw, ids, self.temperature, None, tg)
            self.last_positive_count = npos.detach()
            return loss
        if not general:
            return Fn.ClipLossFn.apply(t_raw, i_raw, self.temperature, None, tg)
        B, Dl = t_raw.shape
        w_mv = float(self.multiview_loss_weight) if is_multiview else 0.0   # ct_clip.py:886-890 (MLM weight 0)
        w_ssl = self.image_ssl_loss_weight if use_ssl else 0.0
        loss = Fn.ClipLossExFn.apply(t_raw.view(1, B, Dl), i_raw.view(n_views, B, Dl),
                                     t_extra.view(1, B, Dl) if extra else None,
                                     i_extra.view(n_views, B, Dl) if extra else None, self.temperature,
                                     bool(self.decoupled_contrastive_learning), 1.0 - w_mv - w_ssl, w_mv, None, tg)
        if use_ssl:
            # (image, aug_1) with one augmented view, (aug_1, aug_2) with two; the gradient reaches
            # to_visual_latent and the tower through i_raw (the leaf encode() makes under the trainer)
            ssl = self.visual_ssl(i_raw.view(n_views, B, Dl)[-2:])
            self.last_image_ssl_loss = ssl.detach().reshape(1)
            loss = loss + w_ssl * ssl                                        # ct_clip.py:892-894
        return loss

    def _forward_filip(self, text, image, return_loss, return_encodings, return_latents):
        """``use_all_token_embeds`` (ct_clip.py:751-755, 829-843): every report token against every spatial
        image token (the pooled volume viewed [B, h*w, d]), both projected token-wise, the fine-grained loss
        on ``functional.FilipLossFn``.  Plain autograd walks both towers (``defer_text_backward`` is not
        used); BERT is joined on the current stream.  Without ``return_loss`` the temperature-scaled token
        similarity [B, T, I] of each pair comes back (the intent of :803), with ``return_latents`` the
        l2-normalised token latents and the image tokens."""
        from . import kernels as K
        if dist_sync.world_rank()[0] > 1:
            raise NotImplementedError('CTCLIP: use_all_token_embeds under torch.distributed with world size > 1 '
                                      '(the token latents are not gathered)')
        vqs = self._vq_state()
        if vqs is not None:
            vqs.defer_ema = DEFER_EMA != '0' and self.visual_transformer.training
        try:
            pooled, _ = self.visual_transformer.encode_pooled(image)
        finally:
            if vqs is not None:
                vqs.defer_ema = False
        enc_text = self.text_transformer(text.input_ids, attention_mask=text.attention_mask)[0]
        if return_encodings:
            self._flush_ema_in_forward()
            return enc_text, pooled
        B, T, dt = enc_text.shape
        d = self.to_visual_latent.weight.shape[1]
        tokens = pooled.view(B, -1, d)
        I, Dl = tokens.shape[1], self.dim_latent
        t_raw = Fn.TextProjFn.apply(enc_text.reshape(B * T, dt).contiguous(), self.to_text_latent.weight).view(B, T, Dl)
        i_raw = Fn.TextProjFn.apply(tokens.reshape(B * I, d).contiguous(), self.to_visual_latent.weight).view(B, I, Dl)
        self._flush_ema_in_forward()
        if return_latents:
            return l2norm(t_raw), l2norm(i_raw), tokens
        if not return_loss:
            tn, inn = l2norm(t_raw.detach()), l2norm(i_raw.detach())
            sim = torch.stack([K.smm(tn[b].contiguous(), inn[b].t()) for b in range(B)])
            return sim * self.temperature.detach().exp()
        mask = text.attention_mask.to(torch.uint8).contiguous()
        return Fn.FilipLossFn.apply(t_raw, i_raw, mask, self.temperature, bool(self.decoupled_contrastive_learning),
                                    bool(self.filip_i2t_over_text))

    def _flush_ema_in_forward(self):
        # the codebook EMA at encode()'s site: after the projections, unless the trainer owns the step
        if DEFER_EMA == '1' or (DEFER_EMA in ('2', '3') and not self.ema_after_step):
            self.flush_ema()

    def backward_deferred_text(self):
        """Back-propagate the text tower whose graph ``encode`` detached (defer_text_backward).
        On the text stream, after the event the loss's backward recorded for its gradient: the
        autograd engine then sees producer and consumer on the same stream and adds no wait on the
        main stream (which would serialise BERT after the whole 3D-ViT backward).  With the extra
        projection both latent sets' gradients go back in one walk."""
        ds = (self._deferred_text, self._deferred_text_extra)
        self._deferred_text = self._deferred_text_extra = None
        ds = [d for d in ds if d is not None and d[1].grad is not None]
        if not ds:
            return
        roots, grads, evs = [d[0] for d in ds], [d[1].grad for d in ds], [d[2] for d in ds]
        ts = streams.text_stream(grads[0].device)
        if ts is None or any(ev is None for ev in evs):
            torch.autograd.backward(roots, grads)
            return
        for ev, g in zip(evs, grads):
            ts.wait_event(ev)
            g.record_stream(ts)
        with torch.cuda.stream(ts):
            torch.autograd.backward(roots, grads)

    def backward_deferred_image(self):
        """Back-propagate the image tower whose graph ``encode`` detached (after BERT's, see
        CTClipTrainer.forward_backward), on the current stream."""
        ds = (self._deferred_image, self._deferred_image_extra)
        self._deferred_image = self._deferred_image_extra = None
        ds = [d for d in ds if d is not None and d[1].grad is not None]
        if ds:
            torch.autograd.backward([d[0] for d in ds], [d[1].grad for d in ds])

    def grad_buckets(self, text_first=True):
        """Gradient all-reduce buckets in the order the backward finalises them (dist_sync): BERT's
        layer groups from the top down (its backward is queued first, CTClipTrainer.forward_backward),
        the 3D-ViT's temporal stack, spatial stack, the rest of the image tower (patch embed, CPB),
        then the CTCLIP-level heads (projections, temperature), launched last."""
        vt = self.visual_transformer
        tb = getattr(self.text_transformer, 'grad_buckets', None)
        text = tb() if tb is not None else [('text_0', list(self.text_transformer.parameters()))]
        vit = [('vit_temporal', list(vt.enc_temporal_transformer.parameters())),
               ('vit_spatial', list(vt.enc_spatial_transformer.parameters())),
               ('vit_rest', list(vt.parameters()))]
        # the scalar temperature last: the arena is packed, and a 1-element parameter ahead of the
        # projections would leave their bf16 shadows off the 16-byte alignment the skinny GEMM needs
        head = [('head', sorted(self.parameters(), key=lambda p: p.numel() % 8 != 0))]
        return text + vit + head if text_first else vit + text + head

    def _pool_tokens(self, tokens):
        """mean over t + flatten of already-quantised tokens (ct_clip.py:724,740)."""
        from . import kernels as K
        pooled = tokens.mean(dim=1).reshape(tokens.shape[0], -1)
        return pooled, K.cast_bf16(pooled.detach().contiguous())
