"""Contrastive train step (ct_clip/CTCLIPTrainer.py:316-354) without the host data loader:
forward -> backward -> gradient all-reduce (RCCL) -> clip_grad_norm_(max_norm) -> Adam -> zero_grad.

MI355X-native layout: every trainable parameter is a view into ONE flat f32 arena, and every
.grad a view into ONE flat f32 gradient arena, so the gradient all-reduce is a single large
RCCL collective, the norm is one reduction kernel and Adam is one fused kernel (which also
never syncs the host: the clip coefficient stays on the device).
"""
from __future__ import annotations

import collections
import os
from types import SimpleNamespace as _Rows

import torch


from . import checkpoint
from . import dist_sync
from . import streams
from . import kernels as K


def _ema_site():
    from . import ct_clip
    return ct_clip.DEFER_EMA


# the per-step status-word copy on its own stream (streams.status_stream); 0 = on the current stream
STATUS_COPY_STREAM = os.environ.get('CTCLIP_STATUS_COPY_STREAM', '1') != '0'


class FlatParams:
    """Every trainable parameter as a view of one f32 arena, its .grad a view of one f32 gradient
    arena, and a bf16 SHADOW arena with the same layout: the Adam kernel writes the bf16 copy of
    each updated weight as it writes the f32 one, so the forward's GEMMs read bf16 weights
    (``functional.bf``) without a cast launch per weight per step.  A shadow is trusted only while
    the parameter's torch version counter and storage are the ones recorded here (an in-place torch
    update, e.g. load_state_dict, falls back to a fresh cast until the next Adam step re-syncs)."""

    def __init__(self, params, device):
        self.params = [p for p in params if p.requires_grad]
        n = sum(p.numel() for p in self.params)
        self.numel = n
        self.data = torch.empty(n, device=device, dtype=torch.float32)
        # one element past the gradients: the step's status slot.  It rides the last gradient bucket's
        # SUM all-reduce (dist_sync.BucketedGradSync), so every rank sees the sum of the ranks'
        # LayerNorm-exchange status words and all skip (or apply) the step together.
        self.grad = torch.zeros(n + 1, device=device, dtype=torch.float32)
        self.status = self.grad[n:]
        # (shadows only on the GPU: the CPU arenas serve the gloo rehearsal tests of the sync logic)
        gpu = torch.device(device).type == 'cuda' and os.environ.get('CTCLIP_BF16_SHADOW', '1') != '0'
        self.bf16 = torch.empty(n, device=device, dtype=torch.bfloat16) if gpu else None
        # ... and its lo residual, bf16(p - bf16(p)): the text tower's GEMMs read W = hi + lo
        # (functional.bf_split, gemm.hip B2); 2 more bytes per parameter written by the same Adam pass
        self.bf16_lo = torch.empty(n, device=device, dtype=torch.bfloat16) if gpu else None
        self.views = []
        off = 0
        for p in self.params:
            k = p.numel()
            self.data[off:off + k].copy_(p.detach().reshape(-1))
            p.data = self.data[off:off + k].view_as(p)
            g = self.grad[off:off + k].view_as(p)
            p.grad = g
            if gpu:
                p._ctclip_bf16 = self.bf16[off:off + k].view_as(p)
                p._ctclip_bf16_lo = self.bf16_lo[off:off + k].view_as(p)
                p._ctclip_off = off
                p._ctclip_flat = self
            self.views.append((off, k, g))
            off += k
        if gpu and n:
            K.cast_bf16_split(self.data, hi=self.bf16, lo=self.bf16_lo)
            self.sync_shadows(0, n)

    def sync_shadows(self, lo, hi):
        """Mark the shadows of the parameters in [lo, hi) current (after the kernel that wrote them)."""
        if self.bf16 is None:
            return
        for p, (off, k, _) in zip(self.params, self.views):
            if lo <= off < hi:
                p._ctclip_ver = p._version
                p._ctclip_ptr = p.data_ptr()

    def rebind_grads(self, only=None):
        """Make sure every .grad is (still) the arena view; fold stray grads back in."""
        sel = None if only is None else {id(p) for p in only}
        for p, (off, k, g) in zip(self.params, self.views):
            if sel is not None and id(p) not in sel:
                continue
            if p.grad is None:
                p.grad = g
            elif p.grad.data_ptr() != g.data_ptr():
                g.copy_(p.grad)
                p.grad = g


class StepGuardError(RuntimeError):
    """A training step was flagged on the device and NOT applied: the summed step status words
    (include/ctclip_hip.h CT_STATUS_*) are the Adam kernels' skip guard, so no rank changed its
    parameters or moments (the gradients were cleared), and the codebook EMA of that step was dropped.
    ``bits`` holds the (rank-summed) status value.  The status word is sticky: later steps are skipped
    too until ``kernels.reset_ln_status()``."""

    def __init__(self, msg, bits=0):
        super().__init__(msg)
        self.bits = bits


class LayerNormExchangeError(StepGuardError):
    """A LayerNorm-fused GEMM (kernels.linear_residual_ln, gemm256.hip EP_LN_FWD / EP_LN_BWD) gave up waiting for
    its partner tile's row statistics: that step's LayerNorm outputs were wrong.  The step's Adam
    update was not applied (the status word is the Adam kernel's skip guard); later steps are not
    applied either until ``kernels.reset_ln_status()``."""


class NonFiniteStepError(StepGuardError):
    """The step's forward or gradients left the representable range: an fp16 operand copy saturated or
    was non-finite (CT_STATUS_F16_RANGE, the 16-bit image-tower forward), a token reached the vector
    quantiser without a finite score (CT_STATUS_VQ_NONFINITE), or the gradient norm was NaN / inf
    (CT_STATUS_NONFINITE_GRAD).  The reference's fp32 step would have propagated the NaN into every
    parameter; here no rank applied the step."""


class EvalGuardError(StepGuardError):
    """A validation pass (``CTClipTrainer.validate``) was flagged on the device: one of its eval
    forwards set status bits (``bits``; e.g. a non-finite validation volume), so its scores are not
    to be trusted.  Nothing was trained by it, and the sticky status word was put back to what it was
    before the pass: no later ``train_step`` is skipped or blamed for it."""


_STATUS_NAMES = ((1, 'LayerNorm exchange timeout'), (2, 'fp16 range (saturated / non-finite fp16 operand)'),
                 (4, 'non-finite gradient norm'), (8, 'non-finite VQ token'))


def describe_status(v):
    """Names of the status bits of a (single-rank) status value."""
    return ', '.join(n for b, n in _STATUS_NAMES if v & b) or 'none'


def raise_for_status(v, step):
    """Raise the StepGuardError of a step's skip word ``v`` (the ranks' summed status words, with the
    gradient-norm bit ORed in), if it is nonzero.  Every rank holds the same value, so every rank
    raises for the same step."""
    if v == 0:
        return
    if v == 1:
        raise LayerNormExchangeError(
            f'LayerNorm-fused GEMM exchange timed out (status word set by step {step} or earlier, on '
            'this rank or another: the ranks\' words are summed with the gradients): its LayerNorm '
            'outputs were wrong and the Adam update of that step was skipped on every rank; '
            'kernels.reset_ln_status() clears the word (CTCLIP_LN_FUSED=0 runs the unfused GEMM + '
            'LayerNorm pair instead)', bits=v)
    raise NonFiniteStepError(
        f'step {step} (or earlier) was flagged on the device, status {v} ({describe_status(v)}; summed '
        'over the ranks): its Adam update and codebook EMA were skipped on every rank, parameters and '
        'moments unchanged; kernels.reset_ln_status() clears the sticky word', bits=v)


# queue BERT's backward before the 3D-ViT's (CTCLIP_TEXT_FIRST=0: after it, the r02 order; A/B)
TEXT_FIRST = os.environ.get('CTCLIP_TEXT_FIRST', '1') != '0'


def grad_buckets(model):
    """[(tag, params)] with every parameter in exactly one bucket, in the model's readiness order
    (``model.grad_buckets()``, e.g. CTCLIP: BERT layer groups, vit_temporal, vit_spatial, vit_rest,
    head)."""
    if not hasattr(model, 'grad_buckets'):
        spec = [('all', list(model.parameters()))]
    else:
        try:
            spec = model.grad_buckets(text_first=TEXT_FIRST)
        except TypeError:
            spec = model.grad_buckets()
    seen, out = set(), []
    for tag, ps in spec:
        mine = []
        for p in ps:
            if id(p) not in seen:
                seen.add(id(p))
                mine.append(p)
        out.append((tag, mine))
    rest = [p for p in model.parameters() if id(p) not in seen]
    if rest:
        out[-1][1].extend(rest)
    return out


class CTClipTrainer:
    """Optimiser + step for a ``ctclip_mi355x.CTCLIP``.  Hyper-parameters default to the
    reference's (CTCLIPTrainer.py:203-205, optimizer.py:24: Adam lr 1.25e-6, betas (0.9, 0.99),
    eps 1e-8, wd 0, clip 0.5).

    ``wd`` restates ct_clip/optimizer.py:23-34.  wd == 0: torch.optim.Adam.  wd != 0:
    torch.optim.AdamW -- decoupled decay p *= 1 - lr wd ahead of the Adam update -- on the parameters
    with ndim >= 2 only (optimizer.py:3-8); biases, LayerNorm gains, q_scale / k_scale and the
    temperature are not decayed.  The Adam kernel decays every element of the slice it is given, so
    with wd != 0 every gradient bucket's parameters are stably partitioned, ndim >= 2 first (BERT's
    q / k / v weights stay adjacent, and so do their biases: functional.bf_cat / gsink_cat), and the
    bucket's Adam runs as two launches, the first slice with wd, the second with 0.  With wd == 0
    the arena order and the launches are the undivided ones."""

    def __init__(self, model, lr=1.25e-6, wd=0.0, max_grad_norm=0.5, betas=(0.9, 0.99), eps=1e-8,
                 overlap_grad_sync=True, defer_text_adam=False):
        self.model = model
        # the text bucket's Adam is queued by the NEXT step's text-tower forward (streams.defer_text);
        # call flush() after the last train_step before reading the parameters
        self.defer_text_adam = defer_text_adam
        dev = next(model.parameters()).device
        self.device = dev
        # arena order = gradient bucket order, so every bucket is one contiguous slice
        groups = grad_buckets(model) if overlap_grad_sync else [('all', list(model.parameters()))]
        if wd != 0:
            # decayed (ndim >= 2) parameters first in every bucket, each kind in its old order
            groups = [(tag, [p for p in ps if p.ndim >= 2] + [p for p in ps if p.ndim < 2]) for tag, ps in groups]
        self.flat = FlatParams([p for _, ps in groups for p in ps], dev)
        segs, off, self.bucket_params = [], 0, {}
        self.decay_segs = []      # (offset, numel, numel of the leading ndim >= 2 slice) per bucket
        for tag, ps in groups:
            n = sum(p.numel() for p in ps if p.requires_grad)
            if n:
                segs.append((tag, off, n))
                self.bucket_params[tag] = [p for p in ps if p.requires_grad]
                self.decay_segs.append((off, n, sum(p.numel() for p in ps if p.requires_grad and p.ndim >= 2)))
            off += n
        self.grad_sync = dist_sync.BucketedGradSync(self.flat.grad, segs, before_launch=self._fold_bucket,
                                                    status=(self.flat.status, self._local_status))
        self.m = torch.zeros_like(self.flat.data)
        self.v = torch.zeros_like(self.flat.data)
        self.lr, self.wd, self.max_grad_norm, self.betas, self.eps = lr, wd, max_grad_norm, betas, eps
        self.steps = 0
        self.norm = torch.zeros(2, device=dev, dtype=torch.float32)
        # the Adam kernels' skip guard of step s: skip_ring[s % 4] = (summed status slot != 0), written
        # after the all-reduce; a ring so a deferred text-bucket Adam still reads its own step's word
        self.skip_ring = torch.zeros(4, device=dev, dtype=torch.int32)
        self.world = dist_sync.world_rank()[0]
        # per-step host check of the LayerNorm-fused GEMMs' status word (kernels.ln_guard): an async
        # copy into pinned memory after each step, read once its event completed -- never more than
        # two steps after the step it covers, so the host stays up to two steps ahead of the GPU
        self._guard = dev.type == 'cuda'
        self._ln_pending = collections.deque()       # (step, event, pinned int32[1])
        self._ln_host = [torch.zeros(1, dtype=torch.int32, pin_memory=True) for _ in range(4)] if self._guard else []
        self.ln_steps_checked = 0
        # train_step_chunked leaves its latent caches and the chunks' dropout call states here; with
        # keep_chunk_latents also pass 2's raw latents and VQ indices per chunk (tests, diagnostics)
        self.keep_chunk_latents = False
        self.last_chunked = None

    def _local_status(self):
        """This rank's sticky LayerNorm-exchange status word (int32[1] on the device), or None (CPU)."""
        return K.ln_status_tensor(self.device) if self._guard else None

    def _fold_bucket(self, tag):
        self.flat.rebind_grads(self.bucket_params.get(tag, ()))

    def forward_backward(self, text, video, aug_image=None, pair_ids=None):
        self.grad_sync.arm()
        defer = hasattr(self.model, 'backward_deferred_text')
        if defer:
            self.model.defer_text_backward = True
        try:
            kw = {} if aug_image is None else dict(aug_image=aug_image)   # extra image views (multiview)
            if pair_ids is not None:
                kw['pair_ids'] = pair_ids                                  # a multi_positive model's group ids
            loss = self.model(text, video, device=self.device, return_loss=True, **kw)
            loss.backward()                      # the loss node (both towers' latents are leaves)
            if defer:
                # BERT first (text stream): its layer-group buckets go out to RCCL as its backward
                # finalises them, ahead of the 3D-ViT's (main stream), whose backward runs beside it
                # (TEXT_FIRST = False: the r02 order, 3D-ViT queued first)
                back_img = getattr(self.model, 'backward_deferred_image', None)
                if not TEXT_FIRST and back_img is not None:
                    back_img()
                self.model.backward_deferred_text()
                if TEXT_FIRST and back_img is not None:
                    back_img()
        except BaseException:
            dist_sync.disarm()
            K.discard_deferred()
            raise
        finally:
            if defer:
                self.model.defer_text_backward = False
        return loss

    def optimizer_step(self):
        try:
            self._optimizer_step()
        finally:
            vqs = getattr(self.model, '_vq_state', lambda: None)()
            if vqs is not None and vqs.pending_ema is not None and self._guard:
                # the pending update is guarded by this step's summed skip word (forward flags of
                # every rank + a non-finite gradient norm), whenever it runs
                vqs.ema_guard = self.skip_ring[self.steps % 4:self.steps % 4 + 1]
            fe = getattr(self.model, 'flush_ema', None)
            if fe is not None and _ema_site() != '3':
                fe()      # a codebook EMA train_step deferred past the optimizer (ct_clip.DEFER_EMA '2';
                #           '3': the next step's image tower queues it after its patch embedding)

    def _optimizer_step(self):
        if streams.pending_text(self.device):
            # the previous step's deferred text Adam was never queued (no text-tower forward ran
            # since): this step's text gradients were summed onto that step's and the shared clip
            # coefficient is about to be overwritten -- refuse rather than train on mixed gradients
            streams.drop_text(self.device)
            raise RuntimeError('CTClipTrainer: a deferred text-tower Adam is still pending at optimizer_step '
                               '(defer_text_adam needs a text-tower forward between optimizer steps; call '
                               'flush() after the last train_step)')
        # SUM (ClipLossFn gives each rank its own rows): buckets already in flight since their
        # tower's backward finished; the last one goes out here and all are waited on.  BERT's
        # backward ran on the text stream (streams.py): order the norm / Adam after it.
        streams.join_text(self.device)
        streams.join_aux(self.device)     # the VQ EMA update (already done by now; keeps state coherent)
        self.grad_sync.finish()
        self.steps += 1
        skip_word = self.skip_ring[self.steps % 4:self.steps % 4 + 1]
        # the ranks' summed status words (any rank flagged -> all skip); the norm kernel ORs in a
        # non-finite gradient (the norm of the all-reduced gradient: the same on every rank)
        skip_word.copy_(self.flat.status)
        K.grad_norm(self.flat.grad[:self.flat.numel], self.max_grad_norm if self.max_grad_norm else 0.0, self.norm,
                    skip=skip_word if self._guard else None)
        # the text bucket's Adam (and grad reset) goes on the text stream: the next step's image
        # tower does not wait for it, the next step's BERT (same stream) does.  It is queued
        # behind the 3D-ViT's Adam (main stream), not beside it: both are HBM-bound, and run side
        # by side the small 3D-ViT update (~25 M parameters) finished only with the large BERT one
        # (~110 M), holding the next step's image tower back by ~0.8 ms; queued after it, the
        # BERT update overlaps the next step's compute-bound image-tower GEMMs instead.
        ts = streams.text_stream(self.device)
        text = [b for b in self.grad_sync.buckets if b[0].startswith('text')] if ts is not None else []
        skip = []
        if text:          # the text buckets are adjacent in the arena (one slice)
            off = min(b[1] for b in text)
            n = sum(b[2] for b in text)
            assert max(b[1] + b[2] for b in text) == off + n
            skip = [(off, n)]
        lo = 0
        for off, n in skip + [(self.flat.numel, 0)]:
            if off > lo:
                self._adam(lo, off - lo)
            lo = off + n
        if skip and self.defer_text_adam:
            # queued by the next step's BERT forward, after the next image tower's patch embedding
            # (streams.defer_text); ``flush`` queues it when no step follows
            off, n = skip[0]
            step = self.steps
            streams.defer_text(self.device, lambda: self._adam(off, n, step=step))
            return
        if skip:
            off, n = skip[0]
            ts.wait_stream(torch.cuda.current_stream(self.device))   # clip coefficient ready
            with torch.cuda.stream(ts):
                self._adam(off, n)

    def flush(self):
        """Queue any deferred text-bucket Adam (``defer_text_adam``) now and verify every step's
        LayerNorm-exchange status (synchronises): call after the last ``train_step`` before reading
        the parameters."""
        streams.flush_text(self.device)
        fe = getattr(self.model, 'flush_ema', None)
        if fe is not None:
            fe()
        # the text-bucket Adam runs on the text stream, the codebook EMA on the auxiliary one: order
        # the caller's stream after both, so parameters read (or saved) on it are the updated ones
        streams.join_text(self.device)
        streams.join_aux(self.device)
        self.check()

    def save(self, path):
        """Write the whole training state to ``path`` (CTCLIPTrainer.py:289-298; checkpoint.py has the
        layout): model ``state_dict``, Adam moments and step count keyed by parameter name, the
        hyper-parameters and the RNG state (seed, BERT's dropout counter, torch's generators).

        EVERY rank calls it at the same step: ``flush()`` runs first (a deferred text Adam, a pending
        codebook EMA -- a collective with world > 1 -- and the step status check, which raises
        StepGuardError before anything is written), rank 0 alone writes, and all ranks meet at a
        barrier.  The write is atomic: ``path + '.tmp'`` then ``os.replace``; a failed write leaves an
        existing ``path`` as it was."""
        checkpoint.save(self, path)

    def load(self, path, strict=True, restore_rng=True):
        """Continue from ``save``'s package: a run stopped there and resumed here computes the bits of
        one that never stopped, whatever ``wd`` / ``overlap_grad_sync`` arena order either side uses
        (DESIGN.md §18 lists what must be equal on both sides).  EVERY rank calls it and reads the
        file.  ``flush()`` runs first; the weights land in the arena, the bf16 shadows are re-cast,
        the weights epoch advances (derived-weight caches), moments, step count and -- unless
        ``restore_rng=False`` -- the RNG state are restored, the gradient arena is cleared.

        Also read: a bare model ``state_dict`` (the reference's periodic ``CTClip.{steps}.pt``) and a
        ``{model, optim}`` package; a uniform ``module.`` key prefix is stripped.  Weights alone leave
        moments and step count as they are.  An ``optim`` that is not name-keyed (the reference's
        positional ``torch.optim.Adam.state_dict()``) raises ``checkpoint.ForeignOptimizerError``
        after the model was loaded.  A trainable parameter without moments in the file, or with
        another shape, raises KeyError / ValueError naming it before anything is changed.

        The hyper-parameters stay the constructor's; returns ``{missing_keys, unexpected_keys,
        hyper_mismatch, step}`` (``hyper_mismatch``: saved and current wd / betas / eps that differ,
        also warned)."""
        return checkpoint.load(self, path, strict=strict, restore_rng=restore_rng)

    def validate(self, volumes, labels, classifier=None, n_boot=0, batch_size=8, curves=False):
        """The reference trainer's validation pass between steps (CTCLIPTrainer.py:356-454): score
        ``volumes`` zero-shot with ``classifier`` (a ``zero_shot.ZeroShotClassifier`` of this model
        with its prompts set -- the reference's are ``VALIDATION_PATHOLOGIES`` with
        ``VALIDATION_TEMPLATE``; for a ``use_all_token_embeds`` model a
        ``token_eval.TokenZeroShotClassifier``; None: the one passed last time) and return
        ``evaluate.ZeroShotEvaluator.evaluate``'s dict (probs, auroc, ci, f1_micro, flat_accuracy; with
        ``curves=True`` also ``curves`` -- operating point, threshold, PR-AUC, average precision per
        label -- and, with n_boot > 0, ``curves_ci``).

        ``flush()`` runs first, so every queued step is applied and verified (a StepGuardError raised
        here belongs to a training step).  The prompts are encoded again with the current weights,
        the forwards run in eval mode under ``no_grad`` (no codebook EMA), and the training mode is
        restored afterwards.

        The pass owns its status bits: the sticky per-device status word is saved and cleared before
        the eval forwards, read after them and put back as it was found.  If the forwards set any
        bit (e.g. a non-finite volume), ``EvalGuardError`` names them; the next ``train_step`` is
        neither skipped nor blamed.

        With world > 1 EVERY rank must call ``validate`` at the same step: ``flush()`` runs a pending
        codebook EMA, whose counts are all-reduced, on all ranks together.  (The reference validates on
        the main process only; here the other ranks may pass an empty result away, but must call.)
        Should an EMA still be pending when the eval forward is about to start, this raises instead of
        letting the forward issue that collective on one rank."""
        from .evaluate import ZeroShotEvaluator
        if classifier is None:
            classifier = getattr(self, '_val_classifier', None)
            if classifier is None:
                raise ValueError('CTClipTrainer.validate: pass classifier= (a ZeroShotClassifier with prompts set)')
        if classifier.model is not self.model:
            raise ValueError('CTClipTrainer.validate: the classifier scores another model')
        self._val_classifier = classifier

        def run():
            classifier.refresh()
            return ZeroShotEvaluator(classifier).evaluate(volumes, labels, n_boot=n_boot, batch_size=batch_size,
                                                          curves=curves)
        return self._eval_pass('validate', 'validation', run)

    def validate_retrieval(self, volumes, text, pair=None, ks=(1, 5, 10, 50, 100), n_boot=0, batch_size=8):
        """Report <-> volume retrieval between steps: ``retrieval.RetrievalEvaluator(model).evaluate``'s
        dict (both directions' ranks, Recall@K, median rank, MRR, bootstrap CIs with n_boot > 0, and
        the latents) for ``volumes`` and the tokenised reports ``text``; ``pair`` [reports]: each
        report's volume (None: report i belongs to volume i).

        The contract is ``validate``'s: ``flush()`` first, a codebook EMA still pending afterwards
        raises, the forwards run in eval mode under ``no_grad``, the status word is saved, cleared,
        read and restored around the pass, ``EvalGuardError`` if the pass set any bit, the training
        mode restored.  With world > 1 every rank calls it at the same step.

        A ``use_all_token_embeds`` model is ranked on its token-wise scores
        (``token_eval.TokenRetrievalEvaluator``, direction 'mean'); the dict has the same keys."""
        if getattr(self.model, 'use_all_token_embeds', False):
            from .token_eval import TokenRetrievalEvaluator as Evaluator
        else:
            from .retrieval import RetrievalEvaluator as Evaluator
        return self._eval_pass('validate_retrieval', 'retrieval validation',
                               lambda: Evaluator(self.model).evaluate(volumes, text, pair=pair, ks=ks,
                                                                      n_boot=n_boot, batch_size=batch_size))

    def validate_case_retrieval(self, volumes, labels, groups=None, **kw):
        """Volume-to-volume retrieval scored by pathology labels between steps:
        ``retrieval.CaseRetrievalEvaluator(model).evaluate(volumes, labels, groups, **kw)``'s dict (the lists,
        MAP@K, precision@K, mean Jaccard@K, bootstrap CIs with n_boot > 0, and the latents).

        The contract is ``validate``'s: ``flush()`` first, a codebook EMA still pending afterwards
        raises, the forwards run in eval mode under ``no_grad``, the status word is saved, cleared,
        read and restored around the pass, ``EvalGuardError`` if the pass set any bit, the training
        mode restored.  With world > 1 every rank calls it at the same step; each rank ranks what it was
        passed (the gallery is not sharded), and the pass adds no collective.

        A ``use_all_token_embeds`` model is refused (``ct_clip.require_cls_latents``): token-wise case
        retrieval is not provided."""
        from .ct_clip import require_cls_latents
        from .retrieval import CaseRetrievalEvaluator
        require_cls_latents(self.model, 'CTClipTrainer.validate_case_retrieval')
        return self._eval_pass('validate_case_retrieval', 'case retrieval validation',
                               lambda: CaseRetrievalEvaluator(self.model).evaluate(volumes, labels, groups, **kw))

    def attribute(self, volumes, classifier=None, **kw):
        """Zero-shot attribution maps between steps: ``classifier.attribute(volumes, **kw)``'s dict
        (maps, probs, scores; ``attribution.ZeroShotAttribution.maps``) with the prompts encoded again
        for the current weights.  ``classifier``: as in ``validate`` (None: the one passed last time).

        The contract is ``validate``'s: ``flush()`` first, eval mode under ``no_grad``, the status word
        saved, cleared, read and restored around the pass, ``EvalGuardError`` if the pass set any bit
        (e.g. a non-finite volume), the training mode restored.  With world > 1 every rank calls it at
        the same step."""
        if classifier is None:
            classifier = getattr(self, '_val_classifier', None)
            if classifier is None:
                raise ValueError('CTClipTrainer.attribute: pass classifier= (a ZeroShotClassifier with prompts set)')
        if classifier.model is not self.model:
            raise ValueError('CTClipTrainer.attribute: the classifier scores another model')
        self._val_classifier = classifier

        def run():
            classifier.refresh()
            return classifier.attribute(volumes, **kw)
        return self._eval_pass('attribute', 'attribution', run)

    def linear_probe(self, train_volumes, train_labels, volumes, labels, *, n_boot=0, curves=False, batch_size=8,
                     **fit_kw):
        """Linear-probe evaluation between steps: fit a ``probe.LinearProbe`` (one logistic head per
        pathology, ``fit_kw`` to ``LinearProbe.fit``) on the frozen image latents of ``train_volumes`` /
        ``train_labels`` and score it on ``volumes`` / ``labels``.  Returns
        ``probe.LinearProbeEvaluator.evaluate``'s dict -- the keys of ``validate`` -- plus ``probe`` (the
        fitted head) and ``fit_loss`` (the per-step loss, on the device).  The number of labels is
        ``train_labels.shape[1]``.

        The contract is ``validate``'s: ``flush()`` first, a codebook EMA still pending afterwards raises, the
        forwards run in eval mode under ``no_grad``, the status word is saved, cleared, read and restored
        around the pass, ``EvalGuardError`` if the pass set any bit (e.g. a non-finite volume), the training
        mode restored.  No tower weight changes.  With world > 1 every rank calls it at the same step; each
        rank fits on what it was passed, and the pass adds no collective."""
        from .probe import LinearProbeEvaluator, NonFiniteLossError

        def run():
            ev = LinearProbeEvaluator(self.model, pathologies=range(torch.as_tensor(train_labels).shape[1]))
            try:
                fit_loss = ev.fit(train_volumes, train_labels, batch_size=batch_size, **fit_kw)
            except NonFiniteLossError:
                # a flagged training volume (e.g. NaN voxels) is the cause, not the fit: EvalGuardError names it
                if self._guard and int(K.status_word(self.device).item()):
                    return None
                raise
            res = ev.evaluate(volumes, labels, n_boot=n_boot, curves=curves, batch_size=batch_size)
            res['probe'], res['fit_loss'] = ev.probe, fit_loss
            return res
        return self._eval_pass('linear_probe', 'linear probe', run)

    def _eval_pass(self, method, what, run):
        """``run()`` as an evaluation pass between steps (``validate`` has the contract)."""
        self.flush()
        vqs = getattr(self.model, '_vq_state', lambda: None)()
        if vqs is not None and vqs.pending_ema is not None:
            raise RuntimeError(f'CTClipTrainer.{method}: a codebook EMA update is still pending after flush(); the eval '
                               'forward would queue it (a collective with world > 1) -- refusing to')
        word = K.status_word(self.device) if self._guard else None
        snap = word.clone() if word is not None else None
        was = self.model.training
        self.model.eval()
        try:
            if word is not None:
                word.zero_()
            with torch.no_grad():
                res = run()
            bits = int(word.item()) if word is not None else 0      # synchronises: the forwards are done
        finally:
            if word is not None:
                word.copy_(snap)
            self.model.train(was)
        if bits:
            raise EvalGuardError(
                f'{what} after step {self.steps} was flagged on the device, status {bits} '
                f'({describe_status(bits)}): its scores are not reported.  The status word was restored to '
                f'{int(snap.item())}, training is unaffected', bits=bits)
        return res

    def check(self):
        """Wait for every queued step-status copy and raise LayerNormExchangeError if a step's
        LayerNorm-fused GEMM timed out."""
        self._check_ln(block_upto=self.steps)

    def _queue_ln_check(self):
        if not self._guard:
            return
        host = self._ln_host[self.steps % len(self._ln_host)]
        # the step's skip word (the ranks' summed status): every rank raises for the same step.  The
        # copy goes on its own stream (STATUS_COPY_STREAM), ordered after the current stream's work so
        # far: the next step's first launches do not queue behind its blit kernel
        cs = streams.status_stream(self.device) if STATUS_COPY_STREAM else None
        ev = torch.cuda.Event()
        if cs is not None:
            cs.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(cs):
                host.copy_(self.skip_ring[self.steps % 4:self.steps % 4 + 1], non_blocking=True)
                ev.record()
        else:
            host.copy_(self.skip_ring[self.steps % 4:self.steps % 4 + 1], non_blocking=True)
            ev.record()
        self._ln_pending.append((self.steps, ev, host))

    def _check_ln(self, block_upto):
        """Consume the status copies: those of steps <= block_upto are waited for, newer ones are
        read only if already complete."""
        while self._ln_pending:
            step, ev, host = self._ln_pending[0]
            if step <= block_upto:
                ev.synchronize()
            elif not ev.query():
                break
            self._ln_pending.popleft()
            v = int(host[0])
            if v != 0:
                self._ln_pending.clear()
                raise_for_status(v, step)
            self.ln_steps_checked = step

    def _adam(self, off, n, step=None):
        """Adam over the arena slice [off, off + n), a run of whole buckets.  wd != 0: two launches
        per bucket, its ndim >= 2 slice with wd and the rest with 0 (optimizer.py:26-32)."""
        if self.wd == 0:
            return self._adam_slice(off, n, 0.0, step)
        done = 0
        for boff, bn, nd in self.decay_segs:
            if off <= boff and boff + bn <= off + n:
                if nd:
                    self._adam_slice(boff, nd, self.wd, step)
                if bn - nd:
                    self._adam_slice(boff + nd, bn - nd, 0.0, step)
                done += bn
        assert done == n, (off, n, done)

    def _adam_slice(self, off, n, wd, step=None):
        sl = slice(off, off + n)
        st = self.steps if step is None else step
        K.adam(self.flat.data[sl], self.flat.grad[sl], self.m[sl], self.v[sl], lr=self.lr, b1=self.betas[0],
               b2=self.betas[1], eps=self.eps, wd=wd, step=self.steps if step is None else step, coef=self.norm,
               p_bf16=self.flat.bf16[sl] if self.flat.bf16 is not None else None,
               p_bf16_lo=self.flat.bf16_lo[sl] if self.flat.bf16_lo is not None else None, zero_grad=True,
               skip=self.skip_ring[st % 4:st % 4 + 1] if self._guard else None)
        self.flat.sync_shadows(off, off + n)

    def train_step(self, text, video, aug_image=None, pair_ids=None):
        """One contrastive step; returns the loss tensor (no host sync).  ``aug_image``: augmented
        views of ``video`` for the multiview loss (CTCLIP.forward); ``pair_ids``: the int64 [B] group ids
        of a ``multi_positive`` model (default: a hash of each report, made on the device).  Raises
        LayerNormExchangeError once the status copy of an earlier step shows a timed-out LayerNorm
        exchange (at the latest two steps later; ``check()`` / ``flush()`` wait for all)."""
        hp = streams.main_stream(self.device)
        if hp is None:
            return self._train_step(text, video, aug_image, pair_ids)
        # CTCLIP_MAIN_PRIORITY=1: the step on the high-priority stream, ordered after the caller's
        # work so far, and the caller's stream after it
        caller = torch.cuda.current_stream(self.device)
        hp.wait_stream(caller)
        with torch.cuda.stream(hp):
            loss = self._train_step(text, video, aug_image, pair_ids)
        caller.wait_stream(hp)
        loss.record_stream(caller)
        return loss

    def train_step_augmented(self, text, video, augment, n_views=1):
        """``train_step`` with ``n_views`` views of ``video`` made on the device by ``augment`` (an
        ``augment.CTAugment``) as ``aug_image``.  The views are a function of (augment.seed,
        self.steps, rank * B + b, view): a resumed run draws the same ones, ranks draw different ones."""
        offset = dist_sync.world_rank()[1] * video.shape[0]
        return self.train_step(text, video, aug_image=augment.views(video, step=self.steps, n_views=n_views,
                                                                    sample_offset=offset))

    def _train_step(self, text, video, aug_image=None, pair_ids=None):
        self._check_ln(block_upto=self.steps - 2)
        self.model.train()
        own = hasattr(self.model, 'ema_after_step')
        if own:
            self.model.ema_after_step = True     # the codebook EMA goes after optimizer_step
        try:
            with K.ln_guard():
                loss = self.forward_backward(text, video, aug_image, pair_ids)
        finally:
            if own:
                self.model.ema_after_step = False
        self.optimizer_step()
        self._queue_ln_check()
        return loss.detach()

    # ------------------------------------------------------------------ chunked step
    def train_step_chunked(self, text, video, chunk, aug_image=None, pair_ids=None):
        """One contrastive step on ``Bg = len(video)`` pairs whose towers run ``chunk`` pairs at a time
        (the last chunk may be shorter): the loss and every gradient are those of the ONE batch of Bg
        pairs -- each row's negatives are all the others -- while only one chunk's activations are
        alive at a time.  ``video`` (int16 HU or f32) may sit in host (pinned) memory: a chunk is
        copied to the device when its turn comes.  Returns the loss [1] over the Bg rows.

        Three passes.  Pass 1 runs both towers per chunk under ``no_grad`` in train
        mode (BERT's dropout on, the codebook read and its EMA withheld) and writes the raw latents
        into two [1, Bg, Dl] caches.  One loss launch over the caches gives the loss, the gradient of
        every cached row and of the temperature (a ``sigmoid_loss`` model: the pairwise sigmoid loss,
        ``functional.sigmoid_loss_all_rows``, and the gradient of ``logit_bias`` too; a ``multi_positive``
        model: ``functional.multipos_loss_all_rows`` on ``pair_ids`` [Bg] or, without them, on the chunks'
        ``kernels.report_ids`` concatenated beside the caches).  Pass 2 rewinds BERT's dropout call state to the one
        recorded for the chunk, runs the chunk's training forward again and back-propagates its rows
        of the cached gradients; parameter gradients add up in the arena, the codebook's EMA
        statistics are held.  Then ONE ``optimizer_step``: one clip, one Adam, one skip word, one
        codebook update from the held statistics.  ``self.steps`` advances by one.

        A status flag raised by any chunk of either pass skips the whole step, as ``train_step``'s
        (``check()`` raises).  Refused: torch.distributed with more than one rank, ``aug_image``,
        ``extra_latent_projection`` (NotImplementedError); ``chunk < 1`` and differing row counts of
        ``text`` and ``video`` (ValueError)."""
        if aug_image is not None:
            raise NotImplementedError('train_step_chunked: image multiview (aug_image) is not chunked; use train_step')
        if getattr(self.model, 'extra_latent_projection', False):
            raise NotImplementedError('train_step_chunked: extra_latent_projection=True is not chunked; use train_step')
        if getattr(self.model, 'use_all_token_embeds', False):
            raise NotImplementedError('train_step_chunked: use_all_token_embeds=True is not chunked; use train_step')
        if getattr(self.model, 'visual_ssl', None) is not None:
            raise NotImplementedError('train_step_chunked: visual_ssl is not chunked (its BatchNorm statistics are '
                                      'one batch\'s); use train_step')
        if dist_sync.world_rank()[0] > 1:
            raise NotImplementedError('train_step_chunked: one rank only (the latent caches are not gathered '
                                      'across ranks yet)')
        if not hasattr(self.model, 'encode') or not hasattr(self.model, 'set_ema_mode'):
            raise NotImplementedError('train_step_chunked: needs a CTCLIP model (encode, set_ema_mode)')
        chunk = int(chunk)
        if chunk < 1:
            raise ValueError(f'train_step_chunked: chunk must be at least 1, got {chunk}')
        Bg = int(video.shape[0])
        if int(text.input_ids.shape[0]) != Bg or Bg < 1:
            raise ValueError(f'train_step_chunked: {int(text.input_ids.shape[0])} reports for {Bg} volumes')
        if pair_ids is not None:
            if not getattr(self.model, 'multi_positive', False):
                raise ValueError('train_step_chunked: pair_ids without a multi_positive model')
            if not torch.is_tensor(pair_ids) or pair_ids.dtype != torch.int64 or pair_ids.shape != (Bg,):
                raise ValueError(f'train_step_chunked: pair_ids must be an int64 tensor [{Bg}]')
        hp = streams.main_stream(self.device)
        if hp is None:
            return self._train_step_chunked(text, video, chunk, pair_ids)
        caller = torch.cuda.current_stream(self.device)
        hp.wait_stream(caller)
        with torch.cuda.stream(hp):
            loss = self._train_step_chunked(text, video, chunk, pair_ids)
        caller.wait_stream(hp)
        loss.record_stream(caller)
        return loss

    def _chunks(self, text, video, chunk):
        """(row0, row1, text rows, volume rows on the device) of every chunk, made as it is asked for."""
        Bg = int(video.shape[0])
        mask = getattr(text, 'attention_mask', None)
        for r0 in range(0, Bg, chunk):
            r1 = min(Bg, r0 + chunk)
            t = _Rows(input_ids=text.input_ids[r0:r1].to(self.device, non_blocking=True),
                      attention_mask=None if mask is None else mask[r0:r1].to(self.device, non_blocking=True))
            yield r0, r1, t, video[r0:r1].to(self.device, non_blocking=True)

    def _dropout_hooks(self):
        tt = getattr(self.model, 'text_transformer', None)
        return getattr(tt, 'dropout_state', None), getattr(tt, 'set_dropout_state', None)

    def _chunked_pass1(self, text, video, chunk, ids_out=None):
        """Pass 1 of ``train_step_chunked``: (text cache, image cache [1, Bg, Dl] f32 raw latents,
        BERT's dropout call state at the start of every chunk).  Train mode, no autograd graph, the
        codebook EMA withheld: the codebook and its cluster sizes are left as they were.  ``ids_out``: a
        list that receives every chunk's ``kernels.report_ids`` (a ``multi_positive`` model's default ids)."""
        model = self.model
        model.train()
        get, _ = self._dropout_hooks()
        tc = ic = None
        states = []
        old = model.set_ema_mode('skip')
        try:
            with torch.no_grad():
                for r0, r1, t, v in self._chunks(text, video, chunk):
                    states.append(get() if get is not None else None)
                    _, _, t_raw, i_raw = model.encode(t, v)
                    if ids_out is not None:
                        ids_out.append(K.report_ids(t.input_ids, t.attention_mask))
                    if tc is None:
                        Bg = int(video.shape[0])
                        tc = torch.empty(1, Bg, t_raw.shape[1], device=self.device, dtype=torch.float32)
                        ic = torch.empty(1, Bg, i_raw.shape[1], device=self.device, dtype=torch.float32)
                    tc[0, r0:r1].copy_(t_raw)
                    ic[0, r0:r1].copy_(i_raw)
        finally:
            model.set_ema_mode(old)
        return tc, ic, states

    def _chunked_pass2(self, text, video, chunk, dt, di, states, keep=None):
        """Pass 2: every chunk's training forward again, from the dropout call state recorded for it,
        and the backward of its rows of ``dt`` / ``di`` through the raw latents -- the text tower on
        the text stream beside the image tower, as ``forward_backward`` queues them.  The codebook's
        EMA statistics are held (CTCLIP.set_ema_mode)."""
        model = self.model
        _, put = self._dropout_hooks()
        old = model.set_ema_mode('hold')
        model.defer_text_backward = True
        try:
            for c, (r0, r1, t, v) in enumerate(self._chunks(text, video, chunk)):
                if put is not None and states[c] is not None:
                    put(states[c])
                _, _, t_raw, i_raw = model.encode(t, v)
                if keep is not None:
                    keep['pass2_text'].append(t_raw.detach().clone())
                    keep['pass2_image'].append(i_raw.detach().clone())
                    keep['indices'].append(model._vq_state().last_indices.clone())
                outs = [(x, g[r0:r1]) for x, g in ((t_raw, dt), (i_raw, di)) if x.requires_grad]
                if outs:
                    # what the loss node's backward does in forward_backward: the towers' latents are
                    # leaves (CTCLIP.encode), their hooks mark the gradient ready for the text stream
                    torch.autograd.backward([x for x, _ in outs], [g for _, g in outs])
                back_img = model.backward_deferred_image
                if not TEXT_FIRST:
                    back_img()
                model.backward_deferred_text()
                if TEXT_FIRST:
                    back_img()
        finally:
            model.defer_text_backward = False
            model.set_ema_mode(old)

    def _train_step_chunked(self, text, video, chunk, pair_ids=None):
        from . import functional as Fn
        self._check_ln(block_upto=self.steps - 2)
        model = self.model
        keep = None
        if self.keep_chunk_latents:
            keep = {'pass2_text': [], 'pass2_image': [], 'indices': []}
        # one status slot, one set of buckets for the whole call: nothing goes out before
        # optimizer_step (one rank: no all-reduce to overlap), which reads the sticky status word once
        self.grad_sync.arm()
        dist_sync.disarm()
        try:
            with K.ln_guard():
                multipos = getattr(model, 'multi_positive', False)
                hashed = [] if multipos and pair_ids is None else None
                tc, ic, states = self._chunked_pass1(text, video, chunk, hashed)
                if multipos:
                    ids = torch.cat(hashed) if pair_ids is None else pair_ids.to(self.device)
                    loss, dt, di, dlt, npos = Fn.multipos_loss_all_rows(tc[0], ic[0], ids, model.temperature)
                    model.last_positive_count = npos
                elif getattr(model, 'sigmoid_loss', False):
                    loss, dt, di, dlt, db = Fn.sigmoid_loss_all_rows(tc[0], ic[0], model.temperature,
                                                                     model.logit_bias)
                    if model.logit_bias.requires_grad:
                        # as the temperature's below: the bias gradient of the one loss launch, once
                        self.flat.rebind_grads([model.logit_bias])
                        model.logit_bias.grad.add_(db.reshape(()))
                else:
                    loss, dt, di, dlt = Fn.clip_loss_all_rows(tc, ic, model.temperature,
                                                              bool(model.decoupled_contrastive_learning))
                if model.temperature.requires_grad:
                    # the temperature's gradient comes from the one loss launch, once
                    self.flat.rebind_grads([model.temperature])
                    model.temperature.grad.add_(dlt.reshape(()))
                self._chunked_pass2(text, video, chunk, dt, di, states, keep)
            model.apply_held_ema()        # pending: optimizer_step guards and queues it, as train_step's
        except BaseException:
            dist_sync.disarm()
            K.discard_deferred()
            model._deferred_text = model._deferred_image = None
            model.drop_held_ema()
            # a deferred text Adam of the previous step reads (and clears) its gradients: queue it first
            streams.flush_text(self.device)
            streams.join_text(self.device)
            streams.join_aux(self.device)
            self.flat.grad.zero_()
            raise
        self.last_chunked = dict(text_cache=tc, image_cache=ic, dropout_states=states, **(keep or {}))
        self.optimizer_step()
        self._queue_ln_check()
        return loss.detach()
