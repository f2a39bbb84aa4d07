"""Trainer checkpoints (ct_clip/CTCLIPTrainer.py:289-307, :456-464): ``CTClipTrainer.save`` / ``load``.

The training state is not a ``torch.optim`` object: Adam's moments are two flat arenas whose order
follows the gradient buckets (and so ``wd`` and ``overlap_grad_sync``), the forward reads bf16 hi / lo
shadows the Adam kernel writes, BERT's dropout masks are hashes of ``torch.initial_seed()`` and a call
counter, and a text-tower Adam or a codebook EMA may still be queued.  A package therefore stores the
moments per parameter NAME, and a load rebuilds everything derived from the weights, so a run that is
stopped and continued computes the bits of one that never stopped.

Package (one ``torch.save``; CPU tensors and plain Python values only, read with weights_only=True):
  format  1
  model   ``model.state_dict()`` (the reference key layout, VQ buffers included)
  optim   {'exp_avg': {name: tensor}, 'exp_avg_sq': {name: tensor}, 'step': int}, trainable parameters
          under their first ``named_parameters()`` name, each tensor in the parameter's shape
  hyper   lr, wd, betas, eps, max_grad_norm (recorded; a load compares, the constructor's hold)
  rng     initial_seed, dropout_calls (the text tower's counter), cpu / device generator states
"""
from __future__ import annotations

import os
import warnings

import torch

from . import dist_sync
from . import kernels as K

FORMAT = 1
_OPTIM_KEYS = {'exp_avg', 'exp_avg_sq', 'step'}


class ForeignOptimizerError(ValueError):
    """The package's ``optim`` entry is not this trainer's name-keyed one.  The model weights of the
    package WERE loaded (``result`` holds load's return value); moments and step count are untouched."""

    def __init__(self, msg, result=None):
        super().__init__(msg)
        self.result = result


def named_slices(trainer):
    """[(name, parameter, arena offset, numel)] of the trainable parameters, in ``named_parameters()``
    order; a parameter tied under two names appears once, under the first."""
    where = {id(p): (off, k) for p, (off, k, _) in zip(trainer.flat.params, trainer.flat.views)}
    out = [(n, p) + where[id(p)] for n, p in trainer.model.named_parameters() if id(p) in where]
    assert len(out) == len(where), 'an arena parameter is not a named parameter of the model'
    return out


def _cpu(t):
    # a fresh, compact CPU tensor (torch.save writes a view's WHOLE storage: never hand it an arena view)
    return t.detach().to('cpu', copy=True).contiguous()


def _dropout_hooks(model):
    tt = getattr(model, 'text_transformer', None)
    return getattr(tt, 'dropout_state', None), getattr(tt, 'set_dropout_state', None)


def build_package(trainer):
    """The package of the trainer's current state, copied to the host on the current stream (the caller
    has flushed: nothing deferred, text and auxiliary streams joined)."""
    dev = trainer.device
    named = named_slices(trainer)
    rng = {'initial_seed': int(torch.initial_seed()), 'cpu': torch.get_rng_state().clone()}
    get, _ = _dropout_hooks(trainer.model)
    if get is not None:
        rng['dropout_calls'] = int(get())
    if dev.type == 'cuda':
        rng['device'] = torch.cuda.get_rng_state(dev).clone()
    return {
        'format': FORMAT,
        'model': {k: _cpu(v) for k, v in trainer.model.state_dict().items()},
        'optim': {'exp_avg': {n: _cpu(trainer.m[off:off + k].view_as(p)) for n, p, off, k in named},
                  'exp_avg_sq': {n: _cpu(trainer.v[off:off + k].view_as(p)) for n, p, off, k in named},
                  'step': int(trainer.steps)},
        'hyper': {'lr': float(trainer.lr), 'wd': float(trainer.wd), 'betas': tuple(float(b) for b in trainer.betas),
                  'eps': float(trainer.eps), 'max_grad_norm': float(trainer.max_grad_norm or 0.0)},
        'rng': rng,
    }


def _barrier():
    if dist_sync.world_rank()[0] > 1:
        torch.distributed.barrier()


def save(trainer, path):
    path = os.fspath(path)
    trainer.flush()
    pkg = build_package(trainer)
    try:
        if dist_sync.world_rank()[1] == 0:
            tmp = path + '.tmp'
            try:
                with open(tmp, 'wb') as f:
                    torch.save(pkg, f)
                os.replace(tmp, path)
            except BaseException:
                if os.path.exists(tmp):
                    os.remove(tmp)
                raise
    finally:
        # also when the write failed: the other ranks wait here, and none runs ahead into a step
        # while another still copies the arenas
        _barrier()


def _strip_module(sd):
    if sd and all(isinstance(k, str) and k.startswith('module.') for k in sd):
        return {k[len('module.'):]: v for k, v in sd.items()}
    return sd


def _classify(pkg):
    """(model state_dict, optim or None, hyper or None, rng or None, foreign optim?)"""
    if not isinstance(pkg, dict):
        raise TypeError(f'CTClipTrainer.load: expected a dict package or a state_dict, got {type(pkg).__name__}')
    if 'format' in pkg:
        if pkg['format'] != FORMAT:
            raise ValueError(f'CTClipTrainer.load: package format {pkg["format"]!r}, this build reads format {FORMAT}')
        return pkg['model'], pkg['optim'], pkg.get('hyper'), pkg.get('rng'), False
    if set(pkg) == {'model', 'optim'} and isinstance(pkg['model'], dict):
        opt = pkg['optim']
        ours = isinstance(opt, dict) and set(opt) == _OPTIM_KEYS
        return pkg['model'], opt if ours else None, None, None, not ours
    return pkg, None, None, None, False      # a bare model state_dict


def _check_optim(named, optim, strict):
    """Every trainable parameter has both moments in its shape, or nothing is read at all."""
    for kind in ('exp_avg', 'exp_avg_sq'):
        for n, p, _, _ in named:
            if n not in optim[kind]:
                raise KeyError(f"CTClipTrainer.load: optim['{kind}'] has no entry for trainable parameter '{n}'")
            t = optim[kind][n]
            if tuple(t.shape) != tuple(p.shape):
                raise ValueError(f"CTClipTrainer.load: optim['{kind}']['{n}'] has shape {tuple(t.shape)}, the "
                                 f'parameter {tuple(p.shape)}')
    names = {n for n, _, _, _ in named}
    extra = sorted({n for kind in ('exp_avg', 'exp_avg_sq') for n in optim[kind]} - names)
    if extra and strict:
        raise KeyError(f'CTClipTrainer.load: optimizer state for names that are not trainable here: {extra}')
    return ['optim.' + n for n in extra]


def load(trainer, path, strict=True, restore_rng=True):
    path = os.fspath(path)
    trainer.flush()
    pkg = torch.load(path, map_location='cpu', weights_only=True)
    model_sd, optim, hyper, rng, foreign = _classify(pkg)
    model_sd = _strip_module(model_sd)
    named = named_slices(trainer)
    extra = _check_optim(named, optim, strict) if optim is not None else []

    bad = trainer.model.load_state_dict(model_sd, strict=strict)     # arena views: lands in the arena
    flat = trainer.flat
    if flat.bf16 is not None and flat.numel:
        # the forward's operands: the same rounding the Adam kernel applies (optim.hip / elementwise.hip)
        K.cast_bf16_split(flat.data, hi=flat.bf16, lo=flat.bf16_lo)
        flat.sync_shadows(0, flat.numel)
    K.advance_weights_epoch()       # drops the MX-fp8 weights, packed weights and the frozen projection's cast
    flat.grad.zero_()               # the gradients and the status slot behind them

    if optim is not None:
        for n, p, off, k in named:
            trainer.m[off:off + k].view_as(p).copy_(optim['exp_avg'][n])
            trainer.v[off:off + k].view_as(p).copy_(optim['exp_avg_sq'][n])
        trainer.steps = int(optim['step'])
        trainer.ln_steps_checked = trainer.steps

    mismatch = {}
    if hyper is not None:
        now = {'wd': float(trainer.wd), 'betas': tuple(float(b) for b in trainer.betas), 'eps': float(trainer.eps)}
        for k, cur in now.items():
            was = hyper.get(k)
            was = tuple(float(b) for b in was) if k == 'betas' and was is not None else was
            if was is not None and was != cur:
                mismatch[k] = (was, cur)
        if mismatch:
            warnings.warn(f'CTClipTrainer.load: {path} was saved with other Adam hyper-parameters (saved, now): '
                          f'{mismatch}; the constructor\'s hold, the resumed run is not the saved run continued')

    if restore_rng and rng is not None:
        _, put = _dropout_hooks(trainer.model)
        if put is not None and 'dropout_calls' in rng:
            put(rng['dropout_calls'])
        torch.set_rng_state(rng['cpu'])           # the generator state carries the seed
        if torch.initial_seed() != rng['initial_seed']:
            torch.manual_seed(rng['initial_seed'])
            torch.set_rng_state(rng['cpu'])
        if trainer.device.type == 'cuda' and 'device' in rng:
            torch.cuda.set_rng_state(rng['device'], trainer.device)

    res = {'missing_keys': list(bad.missing_keys), 'unexpected_keys': list(bad.unexpected_keys) + extra,
           'hyper_mismatch': mismatch, 'step': trainer.steps}
    if foreign:
        raise ForeignOptimizerError(
            f"CTClipTrainer.load: the 'optim' entry of {path} is not this trainer's name-keyed state "
            "({'exp_avg', 'exp_avg_sq', 'step'}).  The reference saves torch.optim.Adam.state_dict(), indexed by "
            'position in a set() of parameters: that order differs from process to process, so a moment cannot be '
            'matched to its parameter.  The model weights were loaded; the moments and the step count were left '
            'as they were', result=res)
    return res
