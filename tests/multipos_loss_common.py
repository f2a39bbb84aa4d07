"""The multi-positive (duplicate-report-aware) InfoNCE loss restated in torch, shared by
test_multipos_loss_cpu.py and test_gpu_multipos_loss.py:

    t^_i, i^_j = F.normalize(raw latents, eps 1e-12);  x_ij = exp(log_temp) <t^_i, i^_j>;
    P_i = { j : ids_j == ids_i },  n_i = |P_i|;
    L = 1/2Bg [ sum_i (logsumexp_j x_ij - 1/n_i sum_{j in P_i} x_ij)
              + sum_j (logsumexp_i x_ij - 1/n_j sum_{i in P_j} x_ij) ],

logsumexp by ``torch.logsumexp``.  It follows the dtype of its inputs; the float64 reference is the
restatement on float64 copies with autograd.  Also the id hash of ``kernels.report_ids`` on plain Python
ints."""
import math
import types

import torch
import torch.nn.functional as F

LOG_TEMPS = [1.0, math.log(10.0), math.log(1 / 0.07)]
_M64 = (1 << 64) - 1
PHI, LEN_MULT = 0x9E3779B97F4A7C15, 0xD1B54A32D192ED03


def multipos_loss(t_raw, i_raw, ids, log_temp):
    """The loss (0-d) of raw latents [Bg, Dl], integer group ids [Bg] and log_temp (0-d or [1])."""
    tn, inn = F.normalize(t_raw, dim=-1, eps=1e-12), F.normalize(i_raw, dim=-1, eps=1e-12)
    x = log_temp.reshape(()).exp() * (tn @ inn.t())
    same = (ids[:, None] == ids[None, :]).to(x.dtype)       # symmetric, so n of a row = n of a column
    n = same.sum(1)
    t2i = torch.logsumexp(x, dim=1) - (x * same).sum(1) / n
    i2t = torch.logsumexp(x, dim=0) - (x * same).sum(0) / n
    return 0.5 * (t2i.mean() + i2t.mean())


def positive_count(ids):
    """sum_i (n_i - 1): the ordered positive pairs off the diagonal."""
    same = ids[:, None] == ids[None, :]
    return int(same.sum().item()) - ids.numel()


def loss_and_grads(t_raw, i_raw, ids, log_temp):
    """(loss [1], dt, di, dlt [1], npos [1] int32) by autograd, in the dtype of the inputs: the outputs of
    kernels.multipos_loss, and a stand-in for it as ``MultiPosLossFn``'s ``impl``."""
    a = [x.detach().clone().requires_grad_(True) for x in (t_raw, i_raw, log_temp)]
    with torch.enable_grad():          # also called inside an autograd.Function forward
        loss = multipos_loss(a[0], a[1], ids, a[2])
        loss.backward()
    npos = torch.tensor([positive_count(ids)], dtype=torch.int32, device=ids.device)
    return loss.detach().reshape(1), a[0].grad, a[1].grad, a[2].grad.reshape(1), npos


def ref64(t_raw, i_raw, ids, log_temp):
    """The float64 reference of f32 inputs (CPU)."""
    return loss_and_grads(t_raw.detach().double().cpu(), i_raw.detach().double().cpu(), ids.cpu(),
                          log_temp.detach().double().cpu())


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / b.norm().clamp_min(1e-30)).item()


OBSERVED = {'loss': 0.0, 'dt': 0.0, 'di': 0.0, 'dlt': 0.0}       # the session's maxima, printed by the GPU tests


def check(out, ref, what=''):
    """The project's loss tolerances (test_gpu_sigmoid_loss.py): loss 1e-5 max(1, |ref|); every gradient and
    dlt 1e-4 relative (norm of the difference over the norm of the reference); npos exact."""
    loss, dt, di, dlt, npos = out
    rl, rdt, rdi, rdlt, rnpos = ref
    el = abs(loss.item() - rl.item()) / max(1.0, abs(rl.item()))
    errs = dict(loss=el, dt=rel(dt, rdt), di=rel(di, rdi), dlt=rel(dlt, rdlt))
    for k, v in errs.items():
        OBSERVED[k] = max(OBSERVED[k], v)
    print(f'{what} loss {loss.item():.7f} ref {rl.item():.7f} ({el:.2e}); rel dt {errs["dt"]:.2e} '
          f'di {errs["di"]:.2e} dlt {errs["dlt"]:.2e}; npos {npos.item()}')
    assert all(torch.isfinite(x).all() for x in (loss, dt, di, dlt))
    assert npos.dtype == torch.int32 and npos.item() == rnpos.item()
    assert el < 1e-5
    assert dt.shape == rdt.shape and di.shape == rdi.shape
    assert errs['dt'] < 1e-4 and errs['di'] < 1e-4 and errs['dlt'] < 1e-4


# ------------------------------------------------------------------------------ the id hash on Python ints
def mix(x):
    """The splitmix64 finaliser (csrc/common.h hid_keep; ``augment.mix64(x, 0)``)."""
    x &= _M64
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & _M64
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & _M64
    x ^= x >> 33
    return x


def report_id(tokens, mask):
    """One report's id as a signed 64-bit Python int: with t_0 .. t_{n-1} the tokens whose mask is non-zero,
    in order, id = mix(sum_k mix(mix(t_k) + (k + 1) PHI) + n LEN_MULT), everything mod 2^64."""
    kept = [int(t) for t, m in zip(tokens, mask) if int(m) != 0]
    acc = 0
    for k, t in enumerate(kept):
        acc = (acc + mix(mix(t) + (k + 1) * PHI)) & _M64
    h = mix(acc + len(kept) * LEN_MULT)
    return h - (1 << 64) if h >= (1 << 63) else h


def report_ids(input_ids, attention_mask):
    return torch.tensor([report_id(r, m) for r, m in zip(input_ids.tolist(), attention_mask.tolist())],
                        dtype=torch.int64)


# ------------------------------------------------------------------------------ id patterns (GPU tests)
def id_pattern(kind, Bg, seed=0):
    """int64 [Bg] group ids of one of the patterns the kernel tests run."""
    base = torch.arange(Bg, dtype=torch.int64) * 7919 - 1234567           # all distinct, some negative
    if kind == 'distinct':
        return base
    if kind == 'equal':
        return torch.full((Bg,), -42, dtype=torch.int64)
    if kind == 'pair_tile':            # rows 63 and 64 when they exist, else the last two rows
        a, b = (63, 64) if Bg > 64 else (max(Bg - 2, 0), Bg - 1)
        base[b] = base[a]
        return base
    if kind == 'pair_ends':            # rows 0 and Bg - 1
        base[Bg - 1] = base[0]
        return base
    if kind == 'random':               # ceil(Bg / 4) groups
        g = torch.Generator().manual_seed(100 + seed)
        return torch.randint(0, (Bg + 3) // 4, (Bg,), generator=g, dtype=torch.int64) * 1000003
    if kind == 'high32':               # ids that differ only in the high 32 bits: two groups, by row parity
        return (torch.arange(Bg, dtype=torch.int64) % 2 + 1) * (1 << 32) + 5
    raise ValueError(kind)


ID_PATTERNS = ('distinct', 'equal', 'pair_tile', 'pair_ends', 'random', 'high32')


# ------------------------------------------------------------------------------ model level (GPU tests)
def duplicate_batch(cfg, B=2, seed=0, dup=(0, 1)):
    """``sigmoid_loss_common.batch`` with report ``dup[1]`` made a copy of report ``dup[0]`` in its kept
    tokens; behind the mask (at least the last four positions) row ``dup[0]`` holds pad id 0 and the copy 7."""
    from sigmoid_loss_common import batch
    hu, text = batch(cfg, B=B, seed=seed)
    ids, mask = text.input_ids.clone(), text.attention_mask.clone()
    a, b = dup
    mask[a, -4:] = 0
    ids[a, -4:] = 0
    mask[b] = mask[a]
    keep = mask[a] != 0
    ids[b] = torch.where(keep, ids[a], torch.full_like(ids[a], 7))
    return hu, types.SimpleNamespace(input_ids=ids, attention_mask=mask)
