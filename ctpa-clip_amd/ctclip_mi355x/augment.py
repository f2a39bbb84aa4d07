"""CT volume augmentation on the device: the views ``CTCLIP.forward(aug_image=...)`` and
``CTClipTrainer.train_step(aug_image=...)`` take.

The reference's own augmentation (``ct_clip/visual_ssl.py:24-45``) is torchvision's 2-D colour-image
pipeline and does not apply to a (1, 240, 480, 480) CT volume; this module is the 3-D counterpart:
a small rotation in the axial plane, scale, translation, an intensity gain / shift and additive
noise, every view of every sample in ONE HIP launch (``ctclip_augment_volume``, csrc/augment.hip),
about one read and one write of the volume and no full-size temporary.

  * ``AugmentParams``: the per (view, sample) records, host tensors.
  * ``apply(video, params)``: the kernel call, ``[V, B, 1, D, H, W]`` of ``video``'s dtype.
  * ``CTAugment``: draws the records as a pure function of (seed, step, global sample index, view)
    and hands the views to the trainer (``views`` / ``CTClipTrainer.train_step_augmented``).

The kernel's arithmetic, for the output voxel ``o = (d, h, w)`` and the centre
``c = ((D-1)/2, (H-1)/2, (W-1)/2)``: the source coordinate is ``s = M (o - c) + (c + t)``, sampled
trilinearly with taps outside the volume reading -1 (the loader's pad value), then
``y = clip(gain * x + shift + sigma * n, -1, 1)`` with ``n`` a zero-mean, unit-variance
Irwin-Hall(4) variate hashed from the record's seed and the voxel's index.  All of it is float64 in
a fixed order, rounded once, so identity records return the input bit for bit (int16 HU inside
[-1000, 1000]; a float -0.0 comes back as +0.0), ``diag(1, 1, -1)`` is ``torch.flip`` along w, an
integer ``t`` an exact shift with fill, and a quarter-turn matrix ``torch.rot90``.

int16 and f32 views are NOT the same bits: for int16 HU ``x = clip(HU, -1000, 1000) / 1000`` and the
view is stored as ``rint(1000 y)`` (half to even), so it is the f32 view rounded to whole HU.  (An
un-augmented int16 volume and its normalised f32 form do give the image tower the same bits.)

No gradients (the input is data), no text augmentation, no elastic deformation.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass

import torch

from ._lib import call, ptr, stream_ptr, AugmentArgs

_DT = {torch.float32: 0, torch.int16: 1}
_M64 = (1 << 64) - 1
_PHI = 0x9E3779B97F4A7C15


def mix64(seed: int, index: int) -> int:
    """The hash of csrc/common.h ``hid_keep`` on plain Python ints: the splitmix64 finaliser of
    ``seed ^ index * phi`` (mod 2^64)."""
    x = (seed ^ (index * _PHI)) & _M64
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & _M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & _M64
    x ^= x >> 33
    return x


@dataclass
class AugmentParams:
    """Records of V views x B samples, host tensors: ``matrix [V, B, 3, 4]`` f64 (``[M | t]``, the
    inverse map output -> source, axes (d, h, w)), ``gain``, ``shift``, ``sigma`` ``[V, B]`` f64 and
    ``seed [V, B]`` int64 (the noise seed's 64 bits)."""
    matrix: torch.Tensor
    gain: torch.Tensor
    shift: torch.Tensor
    sigma: torch.Tensor
    seed: torch.Tensor

    @classmethod
    def identity(cls, V, B):
        m = torch.zeros(V, B, 3, 4, dtype=torch.float64)
        m[..., 0, 0] = m[..., 1, 1] = m[..., 2, 2] = 1.0
        z = torch.zeros(V, B, dtype=torch.float64)
        return cls(m, torch.ones(V, B, dtype=torch.float64), z.clone(), z.clone(), torch.zeros(V, B, dtype=torch.int64))

    def pack(self, pin=False):
        """The records as the kernel reads them: ``[V, B, 16]`` f64 words (12 matrix, gain, shift,
        sigma, the seed's bits), on the host.  Raises ValueError for wrong shapes / dtypes / devices
        and for non-finite values (the kernel does not check)."""
        m = self.matrix
        if m.ndim != 4 or tuple(m.shape[2:]) != (3, 4) or m.shape[0] < 1:
            raise ValueError(f'augment: matrix must be [V, B, 3, 4] with V >= 1, got {tuple(m.shape)}')
        V, B = m.shape[:2]
        for n, t, dt in (('matrix', m, torch.float64), ('gain', self.gain, torch.float64),
                         ('shift', self.shift, torch.float64), ('sigma', self.sigma, torch.float64),
                         ('seed', self.seed, torch.int64)):
            if t.is_cuda or t.dtype != dt:
                raise ValueError(f'augment: {n} must be a host {dt} tensor, got {t.dtype} on {t.device}')
            if n != 'matrix' and tuple(t.shape) != (V, B):
                raise ValueError(f'augment: {n} must be {(V, B)}, got {tuple(t.shape)}')
            if n != 'seed' and not bool(torch.isfinite(t).all()):
                raise ValueError(f'augment: non-finite {n}')
        rec = torch.empty(V, B, 16, dtype=torch.float64, pin_memory=pin)
        rec[..., :12] = m.reshape(V, B, 12)
        rec[..., 12], rec[..., 13], rec[..., 14] = self.gain, self.shift, self.sigma
        rec.view(torch.int64)[..., 15] = self.seed
        return rec


def augment_volume(video, records):
    """The launch: ``video`` (B, 1, D, H, W) contiguous int16 / f32 device tensor, ``records``
    [V, B, 16] f64 device tensor (``AugmentParams.pack``; finite) -> [V, B, 1, D, H, W]."""
    if not video.is_cuda:
        raise ValueError('augment: the volume must be a device tensor')
    if video.dtype not in _DT:
        raise ValueError(f'augment: unsupported volume dtype {video.dtype} (int16 HU or float32)')
    if video.ndim != 5 or video.shape[1] != 1 or not video.is_contiguous() or video.numel() == 0:
        raise ValueError(f'augment: expected a contiguous (B, 1, D, H, W) volume, got {tuple(video.shape)} '
                         f'with strides {video.stride()}')
    B, _, D, H, W = video.shape
    if (records.ndim != 3 or records.shape[0] < 1 or tuple(records.shape[1:]) != (B, 16)
            or records.dtype != torch.float64 or records.device != video.device or not records.is_contiguous()):
        raise ValueError(f'augment: records must be a contiguous float64 [V, {B}, 16] tensor on {video.device}, '
                         f'got {records.dtype} {tuple(records.shape)} on {records.device}')
    V = records.shape[0]
    out = torch.empty(V, B, 1, D, H, W, device=video.device, dtype=video.dtype)
    a = AugmentArgs()
    a.src, a.dtype = ptr(video), _DT[video.dtype]
    a.B, a.D, a.H, a.W, a.V = B, D, H, W, V
    a.recs = ptr(records)
    call('ctclip_augment_volume', ctypes.byref(a), ptr(out), stream_ptr())
    return out


def apply(video, params: AugmentParams):
    """``video`` (B, 1, D, H, W) device tensor, int16 HU or f32 in [-1, 1] -> ``[V, B, 1, D, H, W]``
    of the same dtype: view v of sample b under ``params``' record (v, b).  The records are checked
    on the host and go to the device in one non-blocking copy from pinned memory; nothing waits."""
    if not video.is_cuda:
        raise ValueError('augment: the volume must be a device tensor')
    rec = params.pack(pin=True)
    if rec.shape[1] != video.shape[0]:
        raise ValueError(f'augment: records for {rec.shape[1]} samples, volume batch of {video.shape[0]}')
    return augment_volume(video, rec.to(video.device, non_blocking=True))


class CTAugment:
    """Random affine + intensity augmentation of CT volumes.

    ``rotate_deg``: the view is the volume rotated about the d axis (in the axial plane) by an angle
    uniform in [-rotate_deg, rotate_deg]; ``scale = (lo, hi)``: an isotropic in-plane scale and an
    independent d scale, each uniform in [lo, hi]; ``translate = (td, th, tw)``: a shift uniform in
    [-t, t] voxels per axis (the view's centre shows the source point c + t); ``flip_w``: the
    probability of a left-right flip -- 0 by default because radiology reports name sides ("left
    lower lobe"), and a flipped volume no longer matches its report; ``gain = (lo, hi)`` and
    ``shift`` (uniform in [-shift, shift]) act on the normalised voxel, ``noise_sigma = (lo, hi)`` is
    the range of the additive noise level.

    ``draw`` is a pure function of (seed, step, sample_offset + b, v), computed on the host from a
    counter hash and no generator state: uniform number ``slot`` of view v of global sample g at
    step ``step`` is ``mix64(mix64(mix64(seed, step), g), 16 v + slot) / 2^64``.  So a run resumed
    from a checkpoint (``trainer.steps`` is saved) sees the same views, ranks with disjoint
    ``sample_offset`` see different ones, and re-chunking a batch changes no sample's view."""

    _ANGLE, _SCALE_HW, _SCALE_D, _TD, _TH, _TW, _FLIP, _GAIN, _SHIFT, _SIGMA, _SEED = range(11)

    def __init__(self, seed=0, rotate_deg=10.0, scale=(0.9, 1.1), translate=(8, 24, 24), flip_w=0.0,
                 gain=(0.9, 1.1), shift=0.05, noise_sigma=(0.0, 0.02)):
        self.seed = int(seed)
        self.rotate_deg = float(rotate_deg)
        self.scale = (float(scale[0]), float(scale[1]))
        self.translate = tuple(float(t) for t in translate)
        self.flip_w = float(flip_w)
        self.gain = (float(gain[0]), float(gain[1]))
        self.shift = float(shift)
        self.noise_sigma = (float(noise_sigma[0]), float(noise_sigma[1]))
        vals = (self.rotate_deg, *self.scale, *self.translate, self.flip_w, *self.gain, self.shift, *self.noise_sigma)
        if not all(math.isfinite(v) for v in vals) or len(self.translate) != 3:
            raise ValueError('CTAugment: finite ranges and a (d, h, w) translation')
        if not (0 < self.scale[0] <= self.scale[1]) or self.noise_sigma[0] < 0 or not 0 <= self.flip_w <= 1:
            raise ValueError('CTAugment: 0 < scale lo <= hi, noise_sigma >= 0, 0 <= flip_w <= 1')

    def _record(self, step, g, v):
        key = mix64(mix64(self.seed & _M64, step), g)
        h = lambda slot: mix64(key, 16 * v + slot)
        u = lambda slot: h(slot) / 18446744073709551616.0        # [0, 1]
        sym = lambda slot, r: (2.0 * u(slot) - 1.0) * r
        rng = lambda slot, lo_hi: lo_hi[0] + u(slot) * (lo_hi[1] - lo_hi[0])
        th = math.radians(sym(self._ANGLE, self.rotate_deg))
        s_hw, s_d = rng(self._SCALE_HW, self.scale), rng(self._SCALE_D, self.scale)
        f = -1.0 if u(self._FLIP) < self.flip_w else 1.0
        cs, sn = math.cos(th), math.sin(th)
        # forward: view - c = Flip R(th) S (src - c); M = S^-1 R(th)^T Flip
        m = [[1.0 / s_d, 0.0, 0.0, sym(self._TD, self.translate[0])],
             [0.0, cs / s_hw, sn * f / s_hw, sym(self._TH, self.translate[1])],
             [0.0, -sn / s_hw, cs * f / s_hw, sym(self._TW, self.translate[2])]]
        seed = h(self._SEED)
        return (m, rng(self._GAIN, self.gain), sym(self._SHIFT, self.shift), rng(self._SIGMA, self.noise_sigma),
                seed - (1 << 64) if seed >> 63 else seed)

    def draw(self, step, B, n_views=1, sample_offset=0) -> AugmentParams:
        """The records of ``n_views`` views of samples ``sample_offset .. sample_offset + B - 1`` at
        ``step`` (host tensors)."""
        if B < 1 or n_views < 1:
            raise ValueError('CTAugment.draw: B >= 1 and n_views >= 1')
        recs = [[self._record(int(step), int(sample_offset) + b, v) for b in range(B)] for v in range(n_views)]
        col = lambda k, dt: torch.tensor([[r[k] for r in row] for row in recs], dtype=dt)
        return AugmentParams(col(0, torch.float64), col(1, torch.float64), col(2, torch.float64),
                             col(3, torch.float64), col(4, torch.int64))

    def views(self, video, step, n_views=1, sample_offset=0):
        """``n_views`` augmented views of ``video`` (B, 1, D, H, W), each (B, 1, D, H, W): slices of
        the one output buffer of one launch, ready to pass as ``aug_image=``.  No host sync."""
        if not video.is_cuda:
            raise ValueError('augment: the volume must be a device tensor')
        out = apply(video, self.draw(step, video.shape[0], n_views, sample_offset))
        return tuple(out[v] for v in range(n_views))


__all__ = ['AugmentParams', 'CTAugment', 'apply', 'augment_volume', 'mix64']
