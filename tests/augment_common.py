"""Shared helpers of the volume-augmentation tests (a plain module, imported by test_augment_cpu.py
and test_gpu_augment.py): the float64 numpy restatement of csrc/augment.hip, operation by operation
in the kernel's order, and the plain-Python-int restatement of its hash.

numpy evaluates every float64 operation on its own (no fused multiply-add), which is what the kernel
does with FMA contraction off, so ``restate`` gives the kernel's bits.
"""
import numpy as np
import torch

M64 = (1 << 64) - 1
PHI = 0x9E3779B97F4A7C15
NOISE_DIV = 37837.22723720648          # sqrt(4 * (65536^2 - 1) / 12), the kernel's literal
FILL = -1.0


def mix64(seed, index):
    """splitmix64 finaliser of seed ^ index * phi (csrc/common.h hid_keep), on Python ints."""
    x = (seed ^ (index * PHI)) & M64
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & M64
    x ^= x >> 33
    return x


def noise_int(seed, index):
    """The noise variate of one voxel from Python ints: (sum of the four 16-bit fields - 2 * 65535) /
    NOISE_DIV, one float64 division."""
    x = mix64(seed & M64, index)
    s = (x & 0xffff) + ((x >> 16) & 0xffff) + ((x >> 32) & 0xffff) + (x >> 48)
    return float(s - 2 * 65535) / NOISE_DIV


def noise_field(seed, n):
    """noise_int for flat indices 0 .. n-1, vectorised on uint64 (wrapping arithmetic)."""
    with np.errstate(over='ignore'):
        x = np.uint64(seed & M64) ^ (np.arange(n, dtype=np.uint64) * np.uint64(PHI))
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xff51afd7ed558ccd)
        x ^= x >> np.uint64(33)
        x *= np.uint64(0xc4ceb9fe1a85ec53)
        x ^= x >> np.uint64(33)
    m = np.uint64(0xffff)
    s = ((x & m) + ((x >> np.uint64(16)) & m) + ((x >> np.uint64(32)) & m) + (x >> np.uint64(48))).astype(np.int64)
    return (s - 2 * 65535).astype(np.float64) / NOISE_DIV


def _axis(s, n):
    fl = np.floor(s)
    l1 = s - fl
    l0 = 1.0 - l1
    i0 = np.clip(fl, -2.0, float(n)).astype(np.int64)
    return i0, i0 + 1, l0, l1


def restate_one(vol, m, gain, shift, sigma, seed):
    """One (D, H, W) volume (numpy int16 or float32) under one record -> the view, same dtype."""
    D, H, W = vol.shape
    is_i16 = vol.dtype == np.int16
    x = vol.astype(np.float64)
    if is_i16:
        x = np.clip(x, -1000.0, 1000.0) / 1000.0
    m = np.asarray(m, dtype=np.float64)
    cd, ch, cw = (D - 1) / 2.0, (H - 1) / 2.0, (W - 1) / 2.0
    od = (np.arange(D, dtype=np.float64) - cd)[:, None, None]
    oh = (np.arange(H, dtype=np.float64) - ch)[None, :, None]
    ow = (np.arange(W, dtype=np.float64) - cw)[None, None, :]
    c = (cd, ch, cw)
    ax = []
    for a, n in enumerate((D, H, W)):
        s = ((m[a, 0] * od + m[a, 1] * oh) + m[a, 2] * ow) + (c[a] + m[a, 3])
        ax.append(_axis(s, n))
    (d0, d1, ld0, ld1), (h0, h1, lh0, lh1), (w0, w1, lw0, lw1) = ax

    def tap(di, hi, wi):
        ok = (di >= 0) & (di < D) & (hi >= 0) & (hi < H) & (wi >= 0) & (wi < W)
        v = x[np.clip(di, 0, D - 1), np.clip(hi, 0, H - 1), np.clip(wi, 0, W - 1)]
        return np.where(ok, v, FILL)

    def fw(di, hi):
        o = tap(di, hi, w0) * lw0
        return o + tap(di, hi, w1) * lw1

    def fh(di):
        o = fw(di, h0) * lh0
        return o + fw(di, h1) * lh1

    xi = fh(d0) * ld0
    xi = xi + fh(d1) * ld1
    y = gain * xi + shift
    if sigma != 0.0:
        y = y + sigma * noise_field(int(seed), D * H * W).reshape(D, H, W)
    y = np.where(y < -1.0, -1.0, np.where(y > 1.0, 1.0, y))
    if is_i16:
        return np.rint(1000.0 * y).astype(np.int16)
    return y.astype(np.float32)


def restate(video, params):
    """``video`` (B, 1, D, H, W) torch tensor (any device), ``params`` an AugmentParams ->
    [V, B, 1, D, H, W] host tensor of the same dtype: the float64 restatement of the kernel."""
    v = video.detach().cpu().numpy()
    V, B = params.gain.shape
    out = np.empty((V,) + v.shape, dtype=v.dtype)
    for vi in range(V):
        for b in range(B):
            out[vi, b, 0] = restate_one(v[b, 0], params.matrix[vi, b].numpy(), float(params.gain[vi, b]),
                                        float(params.shift[vi, b]), float(params.sigma[vi, b]),
                                        int(params.seed[vi, b]))
    return torch.from_numpy(out)


def make_volume(B, D, H, W, dtype, seed=0):
    """A random (B, 1, D, H, W) volume: int16 HU inside [-1000, 1000] or f32 in [-1, 1] (host)."""
    g = torch.Generator().manual_seed(1000 * D + 10 * H + W + seed)
    if dtype == torch.int16:
        return torch.randint(-1000, 1001, (B, 1, D, H, W), generator=g, dtype=torch.int16)
    return torch.rand(B, 1, D, H, W, generator=g) * 2.0 - 1.0


def set_matrix(params, m3x3=None, t=None):
    """Overwrite every record's matrix / translation of an AugmentParams in place; returns it."""
    if m3x3 is not None:
        params.matrix[..., :, :3] = torch.tensor(m3x3, dtype=torch.float64)
    if t is not None:
        params.matrix[..., :, 3] = torch.tensor(t, dtype=torch.float64)
    return params


QUARTER_TURN_HW = [[1.0, 0.0, 0.0], [0.0, 0.0, 1.0], [0.0, -1.0, 0.0]]     # out[d, h, w] = in[d, w, W-1-h]
FLIP_W = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, -1.0]]


def shifted(video, t, fill):
    """out[o] = video[o + t] inside the volume, ``fill`` outside: integer t = (td, th, tw)."""
    out = torch.full_like(video, fill)
    D, H, W = video.shape[-3:]
    sl_o, sl_i = [], []
    for n, k in zip((D, H, W), t):
        lo, hi = max(0, -k), min(n, n - k)
        if hi <= lo:
            return out
        sl_o.append(slice(lo, hi))
        sl_i.append(slice(lo + k, hi + k))
    out[(..., *sl_o)] = video[(..., *sl_i)]
    return out


def compare(got, ref):
    """(number of differing voxels, largest difference in f32 ulps / in HU) of two equal-shape tensors."""
    got, ref = got.cpu(), ref.cpu()
    ne = got != ref
    n = int(ne.sum())
    if n == 0:
        return 0, 0
    if got.dtype == torch.int16:
        return n, int((got.int() - ref.int()).abs().max())
    key = lambda x: torch.where(x.view(torch.int32) < 0, -2147483648 - x.view(torch.int32), x.view(torch.int32)).long()
    return n, int((key(got) - key(ref)).abs().max())
