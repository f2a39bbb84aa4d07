"""The LayerNorm row bounds of ln_rows_common are neither vacuous nor too tight, shown on three f32
torch restatements (no GPU):

  * the two-pass algorithm with norm.hip's chunked summation shape satisfies the bound on every
    family at every D the GPU file uses.  Largest error / bound ratio over D in {64, 512, 768, 4000},
    eps in {1e-5, 1e-12}, seeds 0 and 5 (printed by the test; y | mean | rstd):
        base 0.164|0.019|0.142  offset 0.102|0.095|0.111  const 0.124|0.124|0.065  outlier 0.227|0.089|0.242
        tiny 0.384|0.022|0.123  large 0.130|0.021|0.111   step 0.124|0.044|0.165   spike 0.822|0.027|0.496
    -- the margin the GPU assertions rest on: the worst case bound (every rounding at its limit, all of
    one sign) against errors that mostly cancel.  The largest ratio (spike: the zero columns, where
    y = beta + a tiny term) is the final rounding of y itself, half an ulp against the bound's u |y|:
    that term cannot be tighter than 1 / 0.89;
  * a one-pass E[x^2] - E[x]^2 violates it on `offset`;
  * a (mean, M2) merge with a wrong count, or without the d^2 n / 2 term, at any one level violates the
    merged-form bound on `step` (the rows whose block width matches that level).  On the existing tests'
    randn rows the same fault at the upper levels (groups of 128 or 256 columns; with the halved count
    also 64) leaves the output inside their 4e-3 norm tolerance, which is what a norm of a 16-bit output
    over such rows cannot see; at the lower levels the lost share of the variance is a few per cent and
    that norm does see it.  The existing per-row mean / rstd assertions (1e-5 relative, in
    test_gpu_gemm_ln.py and test_gpu_ln1_fold.py) see a dropped term at every level on randn rows too;
    what no earlier assertion sees are errors that scale with (mean / sigma)^2 u -- the one-pass form.

Also: hard_rows puts every family into every block of 8 consecutive rows."""
import pytest
import torch

import ln_rows_common as C

DS = (64, 512, 768, 4000)


def _params(D, seed):
    g = torch.Generator().manual_seed(77 + seed)
    return 1 + 0.2 * torch.randn(D, generator=g), 0.1 * torch.randn(D, generator=g)


def _violations(fn, x, labels, gamma, beta, eps, depth, merged, ratios=None, what=''):
    """families whose rows break any of the three bounds under restatement fn"""
    y, mean, rstd = fn(x, gamma, beta, eps)
    yr, mr, _, rr = C.ln_ref(x, gamma, beta, eps)
    b = C.fwd_bounds(x, gamma, beta, eps, depth, merged=merged)
    bad = set()
    for name, got, ref, bd in (('y', y, yr, b['y']), ('mean', mean, mr, b['mean']),
                               ('rstd', rstd.double() / rr - 1, torch.zeros_like(rr), b['rstd'])):
        r = {}
        try:
            C.check(f'{what}{name}', got, ref, bd, labels, r)
        except AssertionError:
            pass
        for (k, f), v in r.items():
            if ratios is not None:
                ratios[(k, f)] = max(ratios.get((k, f), 0.0), v)
            if v > 1.0:
                bad.add(f)
    return bad


def test_every_family_in_every_block_of_8():
    for D in DS:
        for rows in (None, 67, 2048):
            _, labels = C.hard_rows(D, seed=3, rows=rows)
            for i in range(0, len(labels) - 7):
                assert set(C.family_of(l) for l in labels[i:i + 8]) == set(C.FAMILIES), (D, i)
    # the variants rotate with the seed: two seeds cover every outlier column and step cut of D = 512
    seen = set()
    for seed in (0, 5):
        seen |= set(C.hard_rows(512, seed=seed, rows=67)[1])
    for c in (0, 511, 7, 8, 255, 256, 31, 32, 63, 64):
        assert f'outlier:{c}' in seen
    for c in C.STEP_CUTS:
        assert f'step:{c}' in seen
    x, labels = C.hard_rows(512, dtype=torch.bfloat16)
    assert torch.equal(x, x.bfloat16().float()) and torch.isfinite(x).all()


def test_two_pass_restatement_within_bound():
    ratios = {}
    for D in DS:
        for eps in (1e-5, 1e-12):
            for seed in (0, 5):
                x, labels = C.hard_rows(D, seed=seed, rows=67)
                gamma, beta = _params(D, seed)
                bad = _violations(C.two_pass_f32, x, labels, gamma, beta, eps, C.depth_ln(D), False, ratios)
                assert not bad, (D, eps, seed, bad)
    print('\ntwo-pass f32 restatement, largest error / bound:\n' + C.format_ratios(ratios))
    # not vacuous: somewhere the restatement uses more than 1 % of the bound
    assert max(ratios.values()) > 0.01


def test_merged_restatement_within_bound():
    ratios = {}
    for eps in (1e-5, 1e-12):
        for seed in (0, 5):
            x, labels = C.hard_rows(512, seed=seed, rows=80)
            gamma, beta = _params(512, seed)
            bad = _violations(C.chan_f32, x, labels, gamma, beta, eps, C.DEPTH_GEMM_LN, True, ratios, 'merged ')
            assert not bad, (eps, seed, bad)
    print('\nmerged (mean, M2) f32 restatement, largest error / bound:\n' + C.format_ratios(ratios))


def test_one_pass_violates_on_offset():
    x, labels = C.hard_rows(512, seed=0, rows=80)
    gamma, beta = _params(512, 0)
    bad = _violations(C.one_pass_f32, x, labels, gamma, beta, 1e-5, C.depth_ln(512), False)
    assert 'offset' in bad


@pytest.mark.parametrize('fault', ['count', 'drop'])
@pytest.mark.parametrize('level', range(6))
def test_faulty_merge_violates_on_step(level, fault):
    x, labels = C.hard_rows(512, seed=0, rows=80)
    gamma, beta = _params(512, 0)

    def fn(x, g, b, eps):
        return C.chan_f32(x, g, b, eps, bad_level=level, fault=fault)
    bad = _violations(fn, x, labels, gamma, beta, 1e-5, C.DEPTH_GEMM_LN, True)
    assert 'step' in bad
    # and it is the row whose block width this level merges (8 << level columns) that fails
    cut = 8 << level
    rows = [i for i, l in enumerate(labels) if l == f'step:{cut}']
    assert rows
    y, _, _ = fn(x[rows], gamma, beta, 1e-5)
    yr = C.ln_ref(x[rows], gamma, beta, 1e-5)[0]
    b = C.fwd_bounds(x[rows], gamma, beta, 1e-5, C.DEPTH_GEMM_LN, merged=True)['y']
    assert ((y.double() - yr).abs() > b).any()


@pytest.mark.parametrize('fault,level', [('count', 3), ('count', 4), ('count', 5), ('drop', 4), ('drop', 5)])
def test_faulty_upper_levels_pass_old_norm_tolerance_on_base(fault, level):
    """On randn rows two groups of n columns have means ~ sqrt(2 / n) apart, so a level that merges them
    carries ~ 1 / (2 n) of the variance: dropping it moves y by ~ 1 / (4 n) relative, halving its count by
    ~ 1 / (8 n).  From n = 128 (drop) or n = 64 (count) up to the last level (n = 256, the two workgroups
    of a row block) that stays below the 4e-3 relative Frobenius norm the existing tests allow a bf16
    output; at the lower levels it does not, and there the norm sees the fault (asserted below)."""
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2048, 512, generator=g) + 0.3      # the existing tests' rows
    gamma, beta = _params(512, 1)
    y, _, _ = C.chan_f32(x, gamma, beta, 1e-5, bad_level=level, fault=fault)
    yr = C.ln_ref(x, gamma, beta, 1e-5)[0]
    rel = ((y.bfloat16().double() - yr).norm() / yr.norm()).item()
    print(f'\n{fault} at level {level}: relative norm {rel:.2e}')
    assert rel < C.OLD_NORM_TOL_BF16
    y0, _, _ = C.chan_f32(x, gamma, beta, 1e-5, bad_level=0, fault=fault)
    assert ((y0.bfloat16().double() - yr).norm() / yr.norm()).item() > C.OLD_NORM_TOL_BF16
    labels = ['base:None'] * x.shape[0]
    b = C.fwd_bounds(x, gamma, beta, 1e-5, C.DEPTH_GEMM_LN, merged=True)['y']
    assert ((y.double() - yr).abs() > b).any()         # ... which the per-element bound does see
