"""Evaluation of a use_all_token_embeds model on the GPU (csrc/filip_eval.hip, kernels.filip_scores /
score_ranks, ctclip_mi355x.token_eval) against the float64 restatements of test_filip_eval_cpu.

Tolerance of A, C and val, derived, not tuned: |error| <= (4 Dl + T + I) 2^-24 exp(log_temp) -- 4 Dl 2^-24
exp(log_temp) is DESIGN §27's bound on one f32 score of unit vectors, the rest covers the fixed-order sums of
at most T and I terms of that size.  A maximum is continuous in the scores, so the values need no forced
indices; every kernel index is shown to score, in float64, within the one-score bound of the float64 maximum."""
import math
import types

import pytest
import torch

from test_filip_cpu import _tiny_model, ragged_mask
from test_filip_eval_cpu import filip_scores_full, filip_scores_ref, scattered_mask, score_ranks_ref

pytestmark = pytest.mark.gpu
dev = 'cuda'
CASES = [(1, 1, 1, 1, 16), (2, 3, 7, 4, 32), (3, 2, 17, 65, 64), (5, 4, 33, 63, 128), (2, 2, 40, 576, 512),
         (3, 2, 512, 64, 32), (2, 2, 130, 1024, 16), (70, 3, 5, 9, 16)]
LOG_TEMPS = [0.0, math.log(14.0)]


@pytest.fixture(scope='module')
def K():
    from ctclip_mi355x import kernels
    return kernels


def score_bound(Dl, lt):
    return 4 * Dl * 2.0 ** -24 * math.exp(lt)


def value_bound(T, I, Dl, lt):
    return (4 * Dl + T + I) * 2.0 ** -24 * math.exp(lt)


def _mask(R, T, g):
    """Row 0: the single token T - 1; row 1: every token; then scattered (non-prefix) rows and seeded prefixes
    in turn."""
    mask = ragged_mask(R, T, g)
    for b in range(2, R, 2):
        mask[b] = scattered_mask(1, T, g)[0]
    return mask


def _inputs(R, V, T, I, Dl, seed=0):
    """Seeded latents and masks; the masked text positions hold 1e4-scaled garbage."""
    g = torch.Generator().manual_seed(1000 * R + 100 * V + T + 3 * I + Dl + seed)
    t, i = torch.randn(R, T, Dl, generator=g), torch.randn(V, I, Dl, generator=g)
    mask = _mask(R, T, g)
    junk = 1e4 * torch.randn(R, T, Dl, generator=torch.Generator().manual_seed(seed + 99))
    return torch.where(mask.bool()[..., None], t, junk), i, mask


def _run(K, t, i, mask, lt, want_idx=True):
    out = K.filip_scores(t.to(dev), i.to(dev), mask.to(dev), torch.tensor([lt], device=dev), want_idx=want_idx)
    return {k: v.cpu() for k, v in out.items()}


def _check(out, t, i, mask, lt, tag=''):
    R, T, Dl = t.shape
    V, I = i.shape[:2]
    A, C, idx, val, S = filip_scores_full(t, i, mask, lt)
    tol, sb = value_bound(T, I, Dl, lt), score_bound(Dl, lt)
    errs = {k: (out[k].double() - ref).abs().max().item() for k, ref in (('A', A), ('C', C), ('val_t2i', val))}
    mm = mask.bool()[:, None, :].expand(R, V, T)
    ki = out['idx_t2i'].long()
    assert out['A'].shape == (R, V) and out['idx_t2i'].dtype == torch.int32 and out['val_t2i'].shape == (R, V, T)
    assert (ki[~mm] == -1).all() and (out['val_t2i'][~mm] == 0).all()        # -1 / 0 exactly at masked tokens
    assert (ki[mm] >= 0).all() and (ki[mm] < I).all()
    gap = (S.amax(3) - S.gather(3, ki.clamp_min(0)[..., None]).squeeze(3))[mm].max().item()
    print(f'{tag} A {errs["A"]:.2e} C {errs["C"]:.2e} val {errs["val_t2i"]:.2e} (bound {tol:.2e}); '
          f'index gap {gap:.2e} (bound {sb:.2e}); indices equal to float64: {(ki == idx).float().mean().item():.4f}')
    assert errs['A'] <= tol and errs['C'] <= tol and errs['val_t2i'] <= tol
    assert gap <= sb


# ------------------------------------------------------------------------------ kernel vs restatement
@pytest.mark.parametrize('lt', LOG_TEMPS)
@pytest.mark.parametrize('case', CASES)
def test_scores_match_restatement(K, case, lt):
    t, i, mask = _inputs(*case)
    out = _run(K, t, i, mask, lt)
    _check(out, t, i, mask, lt, tag=str(case))
    plain = _run(K, t, i, mask, lt, want_idx=False)                           # the optional outputs left out
    assert set(plain) == {'A', 'C'} and torch.equal(plain['A'], out['A']) and torch.equal(plain['C'], out['C'])


def test_duplicate_image_tokens_give_the_lowest_index(K):
    t, i, mask = _inputs(3, 2, 17, 65, 64, seed=5)
    i[:, 40] = i[:, 7]
    i[:, 64] = i[:, 7]
    out = _run(K, t, i, mask, 1.0)
    _check(out, t, i, mask, 1.0, tag='duplicates')
    idx = filip_scores_ref(t, i, mask, 1.0)[2]
    ki = out['idx_t2i'].long()
    assert (ki != 40).all() and (ki != 64).all()
    assert torch.equal(ki == 7, idx == 7) and (ki == 7).any()


def test_masked_garbage_moves_nothing(K):
    t, i, mask = _inputs(3, 2, 512, 64, 32)
    t2 = torch.where(mask.bool()[..., None], t, _inputs(3, 2, 512, 64, 32, seed=1)[0])
    assert not torch.equal(t, t2)
    a, b = _run(K, t, i, mask, 1.0), _run(K, t2, i, mask, 1.0)
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------ invariance
def test_position_invariance(K):
    """A full (5, 4) problem against every 1 x 1 sub-call, and against a ragged 2 x 3 blocking."""
    t, i, mask = _inputs(5, 4, 33, 63, 128, seed=3)
    full = _run(K, t, i, mask, math.log(14.0))
    for x in range(5):
        for y in range(4):
            one = _run(K, t[x:x + 1], i[y:y + 1], mask[x:x + 1], math.log(14.0))
            for k in ('A', 'C', 'idx_t2i', 'val_t2i'):
                assert torch.equal(one[k][0, 0], full[k][x, y]), (k, x, y)
    for r0 in range(0, 5, 2):
        for v0 in range(0, 4, 3):
            blk = _run(K, t[r0:r0 + 2], i[v0:v0 + 3], mask[r0:r0 + 2], math.log(14.0))
            for k in ('A', 'C', 'idx_t2i', 'val_t2i'):
                assert torch.equal(blk[k], full[k][r0:r0 + 2, v0:v0 + 3]), (k, r0, v0)


def test_two_runs_are_bit_identical(K):
    t, i, mask = _inputs(3, 2, 512, 64, 32, seed=2)
    a, b = _run(K, t, i, mask, 2.0), _run(K, t, i, mask, 2.0)
    for k in ('A', 'C', 'idx_t2i', 'val_t2i'):
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------ agreement with training
@pytest.mark.parametrize('shape', [(3, 17, 65, 64), (5, 33, 63, 128)])
def test_agrees_with_the_loss_kernel(K, shape):
    """Square and paired: A and C of kernels.filip_loss within twice the bound (the loss recomputes its
    winners as plain dots, so bit equality is not asked)."""
    Bg, T, I, Dl = shape
    t, i, mask = _inputs(Bg, Bg, T, I, Dl, seed=4)
    lt = math.log(14.0)
    out = _run(K, t, i, mask, lt, want_idx=False)
    loss = K.filip_loss(t.to(dev), i.to(dev), mask.to(dev), torch.tensor([lt], device=dev), want_logits=True)
    tol = 2 * value_bound(T, I, Dl, lt)
    ea = (out['A'] - loss['A'].cpu()).abs().max().item()
    ec = (out['C'] - loss['C'].cpu()).abs().max().item()
    print(f'{shape}: |A - A_loss| {ea:.2e} |C - C_loss| {ec:.2e} (bound {tol:.2e})')
    assert ea <= tol and ec <= tol


# ------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize('shape', [(1, 1, 513, 1, 16), (1, 1, 1, 1025, 16), (1, 1, 1, 1, 24), (1, 1, 1, 1, 528)])
def test_unsupported_shapes_are_refused(K, shape):
    from ctclip_mi355x import _lib
    R, V, T, I, Dl = shape
    t, i = torch.zeros(R, T, Dl, device=dev), torch.zeros(V, I, Dl, device=dev)
    mask = torch.ones(R, T, dtype=torch.uint8, device=dev)
    with pytest.raises(_lib.KernelError, match='1003'):                      # CT_ESHAPE, before any launch
        K.filip_scores(t, i, mask, torch.zeros(1, device=dev))
    a = _lib.FilipScoresArgs(R=R, V=V, T=T, I=I, Dl=Dl)
    assert _lib.lib().ctclip_filip_scores_ws_bytes(_lib.ctypes.byref(a)) == 0


def test_workspace_formula_and_row_limit():
    from ctclip_mi355x import _lib
    up4 = lambda n: (n + 3) // 4 * 4
    for R, V, T, I, Dl in ((36, 8, 512, 576, 512), (65535, 1, 1, 1, 16), (3, 5, 7, 9, 32)):
        a = _lib.FilipScoresArgs(R=R, V=V, T=T, I=I, Dl=Dl)
        assert _lib.lib().ctclip_filip_scores_ws_bytes(_lib.ctypes.byref(a)) == 4 * (R * T * Dl + V * I * Dl + up4(R)
                                                                                     + up4(R * T))
    a = _lib.FilipScoresArgs(R=65536, V=1, T=1, I=1, Dl=16)
    assert _lib.lib().ctclip_filip_scores_ws_bytes(_lib.ctypes.byref(a)) == 0
    with pytest.raises(ValueError, match='without a kept token'):
        from ctclip_mi355x import kernels
        kernels.filip_scores(torch.zeros(2, 3, 16, device=dev), torch.zeros(1, 2, 16, device=dev),
                             torch.tensor([[1, 0, 0], [0, 0, 0]], dtype=torch.uint8, device=dev),
                             torch.zeros(1, device=dev))


# ------------------------------------------------------------------------------ score_ranks
def test_score_ranks(K):
    g = torch.Generator().manual_seed(8)
    S = torch.randn(37, 150, generator=g)
    S[:, 9] = S[:, 3]                                                         # bit-equal columns tie
    S[:, 140] = S[:, 3]
    S[5] = 0.25                                                               # a row of one value
    pair = torch.randint(0, 150, (37,), generator=g)
    pair[:6] = torch.tensor([3, 9, 140, 9, 3, 77])                            # several queries per gallery row
    got = K.score_ranks(S.to(dev), pair.to(dev)).cpu()
    assert got.dtype == torch.int32 and torch.equal(got, score_ranks_ref(S, pair))
    assert got[5] == 77
    assert torch.equal(K.score_ranks(S.to(dev), pair.int().to(dev)).cpu(), got)
    sq = S[:, :37].contiguous()
    assert torch.equal(K.score_ranks(sq.to(dev)).cpu(), score_ranks_ref(sq))      # the identity pairing
    one = S[:1]                                                               # N = 1
    assert torch.equal(K.score_ranks(one.to(dev), torch.tensor([140], device=dev)).cpu(),
                       score_ranks_ref(one, torch.tensor([140])))
    assert torch.equal(K.score_ranks(S.t().to(dev), torch.arange(150, device=dev) % 37).cpu(),    # a strided view
                       score_ranks_ref(S.t(), torch.arange(150) % 37))
    with pytest.raises(ValueError, match='pair=None pairs row i'):
        K.score_ranks(S.to(dev))
    with pytest.raises(ValueError, match='must lie in'):
        K.score_ranks(S.to(dev), torch.full((37,), 150, device=dev))


# ------------------------------------------------------------------------------ model level
PATHS = ('alpha', 'beta', 'gamma')
T_TEXT = 12


def _text(rows, seed):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, 100, (rows, T_TEXT), generator=g)
    mask = torch.zeros(rows, T_TEXT, dtype=torch.long)
    for r in range(rows):
        mask[r, :int(torch.randint(1, T_TEXT + 1, (1,), generator=g))] = 1
    return types.SimpleNamespace(input_ids=(ids * mask).to(dev), attention_mask=mask.to(dev))


@pytest.fixture(scope='module')
def tiny(K):
    torch.manual_seed(0)
    model = _tiny_model(use_all_token_embeds=True).to(dev)
    g = torch.Generator().manual_seed(1)
    volumes = torch.randn(5, 1, 20, 40, 40, generator=g).to(dev)
    volumes[3] = volumes[1]                                                   # identical volumes
    K.reset_ln_status()
    from ctclip_mi355x.trainer import CTClipTrainer
    model.trainer = CTClipTrainer(model, lr=1e-3)                             # one arena for the module's tests
    model.eval()
    return model, volumes, _text(2 * len(PATHS), 2), _text(5, 3)


def _state(model):
    return {k: v.detach().clone() for k, v in model.state_dict().items()}


def test_classifier_equals_restatement(tiny):
    from ctclip_mi355x.token_eval import TokenZeroShotClassifier, token_latents_image, token_latents_text
    model, volumes, prompts, _ = tiny
    t, v = token_latents_text(model, prompts), token_latents_image(model, volumes)
    Dl = model.dim_latent
    assert t.shape == (6, T_TEXT, Dl) and v.shape == (5, 4, Dl)
    lt = model.temperature.detach().item()
    A, C, idx, val = filip_scores_ref(t.cpu(), v.cpu(), prompts.attention_mask.cpu(), lt)
    tol = value_bound(T_TEXT, 4, Dl, lt)
    for direction, M in (('t2i', A), ('i2t', C), ('mean', (A + C) / 2)):
        zs = TokenZeroShotClassifier(model, PATHS, direction=direction).set_prompts(prompts)
        probs, scores = zs.predict(volumes)
        assert probs.shape == (5, 3) and scores.shape == (5, 3, 2) and probs.dtype == torch.float32
        want = M.t().reshape(5, 3, 2)
        es = (scores.cpu().double() - want).abs().max().item()
        # the pair's softmax moves by at most a quarter of the change of the score difference (<= 2 tol),
        # plus the f32 rounding of the softmax itself
        ep = (probs.cpu().double() - torch.softmax(want, 2)[..., 0]).abs().max().item()
        print(f'{direction}: scores {es:.2e} (bound {tol:.2e}) probs {ep:.2e}')
        assert es <= tol and ep <= tol / 2 + 4 * 2.0 ** -24
        p1, s1 = zs.predict(volumes, batch_size=1)
        p8, s8 = zs.predict(volumes, batch_size=8)
        assert torch.equal(p1, p8) and torch.equal(s1, s8) and torch.equal(p8, probs)
        assert torch.equal(scores[3], scores[1])
    gr = zs.ground(volumes, batch_size=2)
    assert gr['grid'] == (2, 2) and gr['idx'].shape == gr['score'].shape == (5, 3, 2, T_TEXT)
    mm = prompts.attention_mask.bool().cpu().view(3, 2, T_TEXT)[None].expand(5, 3, 2, T_TEXT)
    gi = gr['idx'].cpu().long()
    assert (gi[~mm] == -1).all() and (gi[mm] >= 0).all() and (gi[mm] < 4).all()
    want_val = val.permute(1, 0, 2).reshape(5, 3, 2, T_TEXT)
    assert (gr['score'].cpu().double() - want_val).abs().max().item() <= tol


def test_evaluator_and_trainer_validate(tiny, K):
    from ctclip_mi355x.evaluate import ZeroShotEvaluator
    from ctclip_mi355x.token_eval import TokenZeroShotClassifier
    model, volumes, prompts, _ = tiny
    labels = torch.tensor([[1, 0, 1], [0, 1, 0], [1, 1, 0], [0, 0, 1], [1, 0, 0]], device=dev)
    zs = TokenZeroShotClassifier(model, PATHS).set_prompts(prompts)
    keys = {'probs', 'auroc', 'ci', 'f1_micro', 'flat_accuracy'}
    res = ZeroShotEvaluator(zs).evaluate(volumes, labels, batch_size=2)
    assert set(res) == keys and res['probs'].shape == (5, 3) and torch.isfinite(res['auroc']).all()
    K.reset_ln_status()
    model.train()
    tr = model.trainer
    before, word = _state(model), K.status_word(volumes.device)
    snap = word.clone()
    val = tr.validate(volumes, labels, classifier=zs, batch_size=2)
    assert set(val) == keys and torch.equal(val['probs'], res['probs'])
    assert model.training and torch.equal(word, snap)
    after = _state(model)
    assert all(torch.equal(before[k], after[k]) for k in before)              # weights and codebook unchanged
    model.eval()


def test_validate_retrieval_uses_the_token_evaluator(tiny, K):
    from ctclip_mi355x.token_eval import TokenRetrievalEvaluator
    model, volumes, _, reports = tiny
    K.reset_ln_status()
    model.train()
    tr = model.trainer
    before, word = _state(model), K.status_word(volumes.device)
    snap = word.clone()
    res = tr.validate_retrieval(volumes, reports, ks=(1, 2), n_boot=4, batch_size=2)
    assert model.training and torch.equal(word, snap)
    after = _state(model)
    assert all(torch.equal(before[k], after[k]) for k in before)
    model.eval()
    assert res['text_latents'].shape == (5, T_TEXT, model.dim_latent) and res['image_latents'].shape[:2] == (5, 4)
    ev = TokenRetrievalEvaluator(model)
    mask = reports.attention_mask.to(torch.uint8)
    S = ev.scores(res['text_latents'], res['image_latents'], mask).cpu()
    assert torch.equal(S, ev.scores(res['text_latents'], res['image_latents'], mask, 2, 3).cpu())     # block-wise
    A, C, _, _ = filip_scores_ref(res['text_latents'].cpu(), res['image_latents'].cpu(), mask.cpu(),
                                  model.temperature.detach().item())
    assert (S.double() - (A + C) / 2).abs().max().item() <= value_bound(T_TEXT, 4, model.dim_latent,
                                                                         model.temperature.detach().item())
    for name, M in (('report_to_volume', S), ('volume_to_report', S.t())):
        d = res[name]
        assert torch.equal(d['ranks'].cpu(), score_ranks_ref(M)) and d['recall'].shape == (2,)
        assert d['ci'].shape == (3, 2) and isinstance(d['mrr'], float)
    # volumes 1 and 3 are identical: equal scores, and the lower index comes first
    assert torch.equal(S[:, 1], S[:, 3])
    full = ev.evaluate(volumes, reports, topk=5, batch_size=2)
    r2v = full['report_to_volume']
    assert torch.equal(r2v['ranks'].cpu(), score_ranks_ref(S))
    idx = r2v['idx'].cpu().long()
    assert r2v['score'].shape == (5, 5) and idx.dtype == torch.int64
    pos = {v: (idx == v).int().argmax(1) for v in (1, 3)}
    assert (pos[3] == pos[1] + 1).all()
    assert torch.equal(r2v['score'].cpu(), S.gather(1, idx))
    # several reports per volume
    pair = torch.tensor([0, 0, 1, 4, 4])
    res2 = ev.evaluate(volumes, reports, pair=pair, ks=(1, 2), batch_size=3, report_block=2, volume_block=2)
    assert torch.equal(res2['report_to_volume']['ranks'].cpu(), score_ranks_ref(S, pair))
    per = score_ranks_ref(S.t()[pair])
    best = torch.full((5,), -1, dtype=torch.int32)
    for vol in (0, 1, 4):
        best[vol] = min(int(per[r]) for r in range(5) if int(pair[r]) == vol)
    assert torch.equal(res2['volume_to_report']['ranks'].cpu(), best)
