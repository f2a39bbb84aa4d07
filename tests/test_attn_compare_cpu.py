"""The attention comparison of attn_common (block-scaled maximum error against float64, tolerance
from a bf16 pipeline emulation) on the CPU: it accepts the emulation and rejects three local faults
of the kind a kernel can have, two of which the suite's whole-tensor Frobenius ratio accepts.

16 x 36 grid, nseq = 2, H = 2, D = 32 (one base-layout case of test_gpu_attn_plan.py)."""
import pytest
import torch

import attn_common as A

GH, GW, NSEQ, H, D, SCALE = 16, 36, 2, 2, 32, 8.0
L = GH * GW
M = NSEQ * L


@pytest.fixture(scope='module')
def case():
    g = torch.Generator().manual_seed(11)
    q = (torch.randn(M, H * D, generator=g) * 0.18).bfloat16()
    k = (torch.randn(M, H * D, generator=g) * 0.18).bfloat16()
    v = (torch.randn(M, H * D, generator=g) * 0.18).bfloat16()
    do = torch.randn(M, H * D, generator=g).bfloat16()
    u = torch.randn(H, (2 * GH - 1) * (2 * GW - 1), generator=g) * 0.5
    bins = A._cpb_bins(GH, GW, 'cpu')
    rows = A._gather_rows(1, L, 0, 1, NSEQ, L, 'cpu')
    ref = A.attn_ref64(q, k, v, do, rows, H, D, SCALE, u, bins)
    emul = A.attn_emul_bf16(q, k, v, do, rows, H, D, SCALE, u, bins)
    return dict(q=q, k=k, v=v, do=do, u=u, bins=bins, rows=rows, ref=ref, emul=emul)


def _verdict(c, got, label):
    res = A.attn_compare(got, c['ref'], c['emul'], c['rows'], H, D, label)
    block_ok = all(r['ok'] for r in res.values())
    rel_ok = all(r['frob_ok'] for r in res.values())
    print(f'{label}: block-scaled metric {"accepts" if block_ok else "REJECTS"}, Frobenius rel '
          f'{"accepts" if rel_ok else "rejects"}')
    return block_ok, rel_ok


def test_emulation_passes(case):
    block_ok, rel_ok = _verdict(case, case['emul'], 'emulation')
    assert block_ok and rel_ok


def test_swapped_grid_bins_rejected(case):
    """(a) the bias gathered with Hg and Wg swapped in the bin formula"""
    c = case
    pos = torch.stack(torch.meshgrid(torch.arange(GH), torch.arange(GW), indexing='ij')).reshape(2, -1).t()
    d = pos[:, None, :] - pos[None, :, :]
    swapped = (d[..., 0] + GW - 1) * (2 * GH - 1) + (d[..., 1] + GH - 1)
    assert int(swapped.max()) < c['u'].shape[1] and not torch.equal(swapped, c['bins'])
    got = A.attn_emul_bf16(c['q'], c['k'], c['v'], c['do'], c['rows'], H, D, SCALE, c['u'], swapped)
    got['du'] = None      # (its bins are the swapped ones: not comparable)
    block_ok, _ = _verdict(c, got, '(a) Hg/Wg swapped bins')
    assert not block_ok


def test_dropped_last_key_chunk_rejected(case):
    """(b) the last 32-key chunk dropped for the last 4 queries of one (sequence, head): the
    Frobenius ratio accepts it, the block-scaled metric does not.  (With all 16 queries of the last
    block the Frobenius ratio of O is 1.1e-2 > 8e-3 and rejects too; 4 queries is the fault it misses.)"""
    c = case
    smask = torch.zeros(NSEQ, H, L, L)
    smask[1, 0, L - 4:, L - 32:] = float('-inf')
    got = A.attn_emul_bf16(c['q'], c['k'], c['v'], c['do'], c['rows'], H, D, SCALE, c['u'], c['bins'], smask=smask)
    block_ok, rel_ok = _verdict(c, got, '(b) last key chunk dropped')
    assert not block_ok
    assert rel_ok, 'the corruption must be one the Frobenius bound accepts'


def test_scaled_query_block_rejected(case):
    """(c) one 16-row query block of one head of O scaled by 1.02 (the block holding that
    (sequence, head)'s largest |O|): accepted by the Frobenius ratio, rejected block-scaled"""
    c = case
    got = {n: (t.clone() if t is not None else None) for n, t in c['emul'].items()}
    s, h = 0, 1
    blk = got['o'][s * L:(s + 1) * L, h * D:(h + 1) * D]
    qb = int(blk.abs().amax(-1).argmax()) // 16
    blk[qb * 16:(qb + 1) * 16] = (blk[qb * 16:(qb + 1) * 16] * 1.02).bfloat16().float()
    block_ok, rel_ok = _verdict(c, got, '(c) query block x 1.02')
    assert not block_ok
    assert rel_ok, 'the corruption must be one the Frobenius bound accepts'
