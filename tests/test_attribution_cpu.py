"""Zero-shot attribution maps, host side: the float64 restatement of the decomposition (used by
tests/test_gpu_attribution.py as the reference of the kernels) and its completeness.

The restatement is written from the algebra of DESIGN.md §24: after the VQ and the mean over t the image
latent is v_n = W . pooled_n with pooled_n[hw] = (1/T) sum_t C[idx[n, t, hw]], so for a direction d
    tau d . v_n / ||v_n|| = sum_{t, hw} tau / (T ||v_n||) (W[:, hw*D:(hw+1)*D]^T d) . C[idx[n, t, hw]].
In float64 both sides agree to rounding (asserted at 1e-12)."""
import pytest
import torch

F64 = torch.float64


def direction_rows(t_raw, which):
    """'log_odds': [P, Dl], the difference of each l2-normalised (present, not present) pair; 'scores':
    [2P, Dl], the normalised prompt latents."""
    if which not in ('log_odds', 'scores'):
        raise ValueError(which)
    u = t_raw.to(F64)
    u = u / u.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    return u[0::2] - u[1::2] if which == 'log_odds' else u


def pooled_reference(codebook, idx, T, HW, D):
    """pooled [N, HW * D] f64: the mean over t of the code rows, flattened (hw, d)."""
    N = idx.numel() // (T * HW)
    rows = codebook.to(F64)[idx.reshape(N, T, HW).long()]            # [N, T, HW, D]
    return rows.mean(dim=1).reshape(N, HW * D)


def attribution_reference(W, codebook, idx, t_raw, log_temp, T, HW, D, which, norm=None, normalize=True):
    """maps [N, R, T, HW] f64 (R = P for 'log_odds', 2P for 'scores') from W [Dl, HW * D], codebook
    [codes, D], idx [N * T * HW] (layout [n][t][hw]), raw prompt latents t_raw [2P, Dl] and the log
    temperature.  ``norm`` [N]: the image latents' norms to divide by (None: ||W . pooled_n|| computed
    here); ``normalize=False``: the raw contributions V . C[idx]."""
    W = W.to(F64)
    dirs = direction_rows(t_raw, which)                               # [R, Dl]
    V = (dirs @ W).reshape(-1, HW, D)                                 # [R, HW, D]
    if not normalize:
        return map_reference(V, codebook, idx, T, HW)
    if norm is None:
        norm = (pooled_reference(codebook, idx, T, HW, D) @ W.t()).norm(dim=-1)
    return map_reference(V, codebook, idx, T, HW, scale_reference(log_temp, T, norm))


def scale_reference(log_temp, T, norm):
    """s_n [N] f64 = exp(log_temp) / (T max(norm_n, 1e-12))."""
    return torch.exp(torch.as_tensor(log_temp).to(F64).reshape(())) / (T * norm.to(F64).clamp_min(1e-12))


def map_reference(V, codebook, idx, T, HW, scale=None):
    """out [N, R, T, HW] f64 = scale_n V[r, hw, :] . codebook[idx[n, t, hw], :] (scale None: 1)."""
    N = idx.numel() // (T * HW)
    rows = codebook.to(F64)[idx.reshape(N, T, HW).long()]             # [N, T, HW, D]
    maps = torch.einsum('rhd,nthd->nrth', V.to(F64), rows)
    return maps if scale is None else maps * scale.reshape(N, 1, 1, 1)


def scores_reference(W, codebook, idx, t_raw, log_temp, T, HW, D):
    """scores [N, P, 2] f64 the direct way: project the pooled tokens, normalise, dot, temperature."""
    v = pooled_reference(codebook, idx, T, HW, D) @ W.to(F64).t()
    v = v / v.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    u = direction_rows(t_raw, 'scores')
    tau = torch.exp(torch.as_tensor(log_temp, dtype=F64).reshape(()))
    return (tau * v @ u.t()).reshape(v.shape[0], -1, 2)


@pytest.fixture(scope='module')
def case():
    g = torch.Generator().manual_seed(24)
    N, P, T, HW, D, Dl, codes = 3, 2, 4, 5, 64, 32, 16
    W = torch.randn(Dl, HW * D, generator=g, dtype=F64) / (HW * D) ** 0.5
    cb = torch.randn(codes, D, generator=g, dtype=F64)
    idx = torch.randint(0, codes, (N * T * HW,), generator=g, dtype=torch.int32)
    t_raw = torch.randn(2 * P, Dl, generator=g, dtype=F64)
    log_temp = torch.tensor(0.7, dtype=F64)
    return dict(W=W, codebook=cb, idx=idx, t_raw=t_raw, log_temp=log_temp, T=T, HW=HW, D=D), (N, P)


def test_log_odds_completeness(case):
    kw, (N, P) = case
    maps = attribution_reference(which='log_odds', **kw)
    assert maps.shape == (N, P, kw['T'], kw['HW'])
    s = scores_reference(**kw)
    total = maps.sum(dim=(2, 3))
    assert (total - (s[..., 0] - s[..., 1])).abs().max().item() <= 1e-12
    probs = torch.softmax(s, dim=-1)[..., 0]
    assert (total - torch.logit(probs)).abs().max().item() <= 1e-12


def test_scores_completeness(case):
    kw, (N, P) = case
    maps = attribution_reference(which='scores', **kw)
    assert maps.shape == (N, 2 * P, kw['T'], kw['HW'])
    s = scores_reference(**kw)
    assert (maps.sum(dim=(2, 3)).reshape(N, P, 2) - s).abs().max().item() <= 1e-12
    # the log-odds map is the difference of the pair's score maps
    lo = attribution_reference(which='log_odds', **kw)
    assert (lo - (maps[:, 0::2] - maps[:, 1::2])).abs().max().item() <= 1e-12


def test_raw_contributions_sum_to_the_unnormalised_product(case):
    kw, (N, P) = case
    raw = attribution_reference(which='log_odds', normalize=False, **kw)
    v = pooled_reference(kw['codebook'], kw['idx'], kw['T'], kw['HW'], kw['D']) @ kw['W'].t()
    d = direction_rows(kw['t_raw'], 'log_odds')
    assert (raw.sum(dim=(2, 3)) - kw['T'] * v @ d.t()).abs().max().item() <= 1e-12


def test_package_directions_match_the_restatement(case):
    from ctclip_mi355x.attribution import directions
    kw, _ = case
    for which in ('log_odds', 'scores'):
        got = directions(kw['t_raw'].float(), which)
        assert got.dtype == torch.float32
        assert (got.double() - direction_rows(kw['t_raw'].float(), which)).abs().max().item() <= 1e-6


def test_to_volume_preserves_sums(case):
    from ctclip_mi355x.attribution import to_volume
    kw, (N, P) = case
    maps = attribution_reference(which='log_odds', **kw).reshape(N, P, kw['T'], 5, 1)
    vol = to_volume(maps, patch=(3, 2, 4))
    assert vol.shape == (N, P, kw['T'] * 3, 10, 4)
    assert (vol.sum(dim=(2, 3, 4)) - maps.sum(dim=(2, 3, 4))).abs().max().item() <= 1e-12
    # nearest neighbour: every voxel of a token's block holds the token's value / block size
    assert torch.equal(vol[..., 0::3, 0::2, 0::4], vol[..., 2::3, 1::2, 3::4])
    assert (vol[..., 0::3, 0::2, 0::4] * 24 - maps).abs().max().item() <= 1e-14


def test_bad_which_raises_on_the_host():
    """``which`` is checked before anything touches the model or the device."""
    from ctclip_mi355x.attribution import ZeroShotAttribution, directions
    import types
    cl = types.SimpleNamespace(model=None, _t_raw=None, pathologies=())
    with pytest.raises(ValueError, match='which'):
        ZeroShotAttribution(cl).maps(torch.zeros(1, 1, 2, 2, 2), which='gradients')
    with pytest.raises(ValueError, match='which'):
        directions(torch.zeros(2, 4), 'both')
    with pytest.raises(ValueError):
        direction_rows(torch.zeros(2, 4), 'both')
