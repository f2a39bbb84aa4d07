"""Case retrieval on the GPU: ctclip_case_retrieval (csrc/case_retrieval.hip), ``kernels.case_retrieval``, its
custom op, ``retrieval.CaseRetrievalEvaluator`` and ``CTClipTrainer.validate_case_retrieval``.

Reference: the float64 restatement of case_retrieval_common.py (checked on hand-worked cases by
test_case_retrieval_cpu.py).

Exact-arithmetic inputs (rows of 16 entries +-1: every score is a multiple of 1/16, exact in f32 in any
order): EVERY output must equal the restatement -- lists with their ties, integer counts, and the float64
bits of ap and gain.

Random inputs: the score bound (2 Dl + 8) 2^-24 is test_gpu_retrieval's (an f32 fma chain over Dl products of
unit vectors, the rounding of the two normalised vectors, the norm and the division).  hits / ap / gain must
equal the restatement applied to the kernel's OWN idx bit for bit on every query; nrel and filled do not
depend on a score and must equal the reference on every query; idx must equal the reference list on every
query whose float64 gaps between adjacent list places (and places K_max / K_max + 1) are all at least 1e-6
-- far above the score bound's reach on a difference only where Dl is small, so this is the one check with
a left-out share, which must stay within 2 % of the queries.  Left out by the reference alone (computed on
the CPU for the seeds below): (300, 300, 512) seed 0: 3 of 300; (65, 130, 100) seed 1: 0 of 65;
(257, 64, 64) seed 2: 0 of 257."""
import types

import pytest
import torch

import case_retrieval_common as C
from oracle import ctclip_oracle as O
from oracle import weights as W

pytestmark = pytest.mark.gpu

OUTS = ('idx', 'score', 'filled', 'nrel', 'hits', 'ap', 'gain')


def _K():
    from ctclip_mi355x import kernels as K
    return K


def _dev(t):
    return None if t is None else t.cuda()


def _run(case, ks, rel):
    q = case.q.cuda()
    g = q if case.g is case.q else case.g.cuda()                     # one buffer when the gallery queries itself
    return _K().case_retrieval(q, g, case.qlab.cuda(), case.glab.cuda(), _dev(case.qgrp), _dev(case.ggrp), ks=ks,
                               rel=rel)


def _ref(case, ks, rel):
    return C.reference(case.q, case.g, case.qlab, case.glab, case.qgrp, case.ggrp, ks, rel)


def _assert_equal(got, want, what=OUTS):
    for name in what:
        a, b = getattr(got, name).cpu(), getattr(want, name)
        assert a.shape == b.shape, name
        if name == 'score':
            assert a.dtype == torch.float32
            a = a.double()
        assert a.dtype == b.dtype, name
        assert torch.equal(a, b), name                                # f64: the same bits (no NaN, no -0 here)


def _ks(M):
    return tuple(sorted({1, 5, 50, min(M, 128)}))


# ------------------------------------------------------------------------------------ exact inputs
# (1, 1, 16) ... (130, 257, 258): odd sizes around the 64 x 64 tile; (6, 130, 32): few rows; (70, 1100, 24):
# more column tiles than column chunks, so a workgroup walks several tiles and the chunk merge runs
EXACT_SHAPES = [(1, 1, 16), (3, 2, 20), (63, 65, 64), (64, 64, 100), (65, 129, 127), (130, 257, 258), (6, 130, 32),
                (70, 1100, 24)]


@pytest.mark.parametrize('groups', ['none', 'self', 'groups'])
@pytest.mark.parametrize('shape', EXACT_SHAPES)
def test_exact_inputs_equal_the_reference(shape, groups):
    K = _K()
    N, M, Dl = shape
    case = C.exact_case(N, M, Dl, seed=N + M, groups=groups)
    ks = _ks(M)
    for rel in ('any', 'exact'):
        want = _ref(case, ks, rel)
        assert torch.equal(want.S * 16, (want.S * 16).round())        # the construction is exact
        got = _run(case, ks, rel)
        _assert_equal(got, want)
        if groups == 'self':
            mid = M // 2                                             # the middle duplicate: rows 0 and M - 1 remain
            if M >= 3:
                assert got.idx[mid, :2].tolist() == [0, M - 1] and got.score[mid, :2].tolist() == [1.0, 1.0]
            assert int((got.idx.cpu() == torch.arange(M)[:, None]).sum()) == 0
            if M == 1:
                assert got.filled.tolist() == [0] and got.ap.tolist() == [[-1.0] * len(ks)]
        if groups == 'groups' and M <= 5:                            # query 0's group is the whole gallery
            assert int(got.filled[0]) == 0 and got.ap[0].tolist() == [-1.0] * len(ks)
            assert got.idx[0].tolist() == [-1] * ks[-1] and got.gain[0].tolist() == [0.0] * len(ks)
        if groups == 'none' and ks[-1] <= M:                         # the existing kernel's lists, bit for bit
            s, i = K.retrieval_topk(case.q.cuda(), case.g.cuda(), ks[-1])
            assert torch.equal(got.idx, i) and torch.equal(got.score, s)


def test_a_group_that_is_the_whole_gallery():
    """Beyond one tile: every gallery row in group 7; query 0 (group 7) sees nothing, query 1 (-1) and query 2
    (another id) see everything."""
    case = C.exact_case(6, 130, 32, seed=3, groups='none')
    case.ggrp = torch.full((130,), 7, dtype=torch.int32)
    case.qgrp = torch.tensor([7, -1, 8, 7, -1, 0], dtype=torch.int32)
    ks = (1, 5, 50, 128)
    for rel in ('any', 'exact'):
        got, want = _run(case, ks, rel), _ref(case, ks, rel)
        _assert_equal(got, want)
        assert got.filled.tolist() == [0, 128, 128, 0, 128, 128] and got.nrel[0].item() == 0
        assert got.ap[0].tolist() == [-1.0] * 4 and got.ap[3].tolist() == [-1.0] * 4


# ----------------------------------------------------------------------------------- random inputs
RANDOM_CASES = [((300, 300, 512), 0), ((65, 130, 100), 1), ((257, 64, 64), 2)]
RANDOM_KS = (1, 5, 10, 50)


@pytest.mark.parametrize('shape,seed', RANDOM_CASES)
def test_random_inputs(shape, seed):
    K = _K()
    N, M, Dl = shape
    case = C.random_case(N, M, Dl, seed)
    bound = (2 * Dl + 8) * 2.0 ** -24
    for rel in ('any', 'exact'):
        want = _ref(case, RANDOM_KS, rel)
        got = _run(case, RANDOM_KS, rel)
        _assert_equal(got, want, ('filled', 'nrel'))
        own = types.SimpleNamespace()
        own.hits, own.ap, own.gain = C.metrics_on_lists(got.idx, case.qlab, case.glab, got.nrel.cpu(), RANDOM_KS, rel)
        _assert_equal(got, own, ('hits', 'ap', 'gain'))              # on the kernel's own lists: bit for bit
        err = (got.score.cpu().double() - want.score).abs().max().item()
        clear = C.clear_queries(want, RANDOM_KS[-1])
        left_out = int((~clear).sum())
        wrong = int((got.idx.cpu()[clear] != want.idx[clear]).any(1).sum())
        print(f'{shape} {rel}: max |score - float64| {err:.3e} (bound {bound:.3e}); {left_out} of {N} queries left '
              f'out (gap < 1e-6), {wrong} lists differ outside them')
        assert err <= bound
        assert left_out <= 0.02 * N
        assert wrong == 0
        assert int((got.idx.cpu() == torch.arange(N)[:, None]).sum()) == 0         # self-exclusion
    # no groups: the existing kernel's lists, bit for bit
    free = K.case_retrieval(case.q.cuda(), case.g.cuda(), case.qlab.cuda(), case.glab.cuda(), ks=RANDOM_KS)
    s, i = K.retrieval_topk(case.q.cuda(), case.g.cuda(), RANDOM_KS[-1])
    assert torch.equal(free.idx, i) and torch.equal(free.score, s)


def test_bit_reproducible():
    for case, ks in ((C.random_case(300, 300, 512, 0), RANDOM_KS), (C.exact_case(70, 1100, 24, 5, 'groups'), (1, 128))):
        a, b = _run(case, ks, 'any'), _run(case, ks, 'any')
        for name in OUTS:
            assert torch.equal(getattr(a, name), getattr(b, name)), name


# ---------------------------------------------------------------------------- the C-ABI directly
def _raw(q, g, qlab, glab, qgrp, ggrp, ks, rel, outs, ws, ws_bytes):
    from ctclip_mi355x import _lib
    N, Dl = q.shape
    arr = (_lib.c_i32 * max(len(ks), 1))(*ks)
    return _lib.lib().ctclip_case_retrieval(
        _lib.ptr(q), _lib.ptr(g), _lib.ptr(qlab), _lib.ptr(glab), _lib.ptr(qgrp), _lib.ptr(ggrp), N, g.shape[0], Dl,
        arr, len(ks), rel, *[_lib.ptr(o) for o in outs], _lib.ptr(ws), ws_bytes, _lib.stream_ptr())


def test_guard_bands():
    """Every output lies inside a sentinel-filled buffer (NaN for floats, 0x5a5a5a5a for integers): nothing
    outside the output changes, and the unfilled places hold exactly -1 / 0 (never the sentinel)."""
    from ctclip_mi355x import _lib
    case = C.exact_case(70, 130, 24, seed=9, groups='groups')
    case.qgrp[5] = -1
    ks, rel, N, M, PAD = (1, 5, 128), 0, 70, 130, 64
    want = _ref(case, ks, 'any')
    assert int(want.filled.min()) < 128                              # some places stay unfilled
    shapes = dict(idx=((N, 128), torch.int32), score=((N, 128), torch.float32), filled=((N,), torch.int32),
                  nrel=((N,), torch.int32), hits=((N, 3), torch.int32), ap=((N, 3), torch.float64),
                  gain=((N, 3), torch.float64))
    bufs, outs = {}, {}
    for name, (shp, dt) in shapes.items():
        n = int(torch.tensor(shp).prod())
        fill = float('nan') if dt.is_floating_point else 0x5a5a5a5a
        bufs[name] = torch.full((n + 2 * PAD,), fill, device='cuda', dtype=dt)
        outs[name] = bufs[name][PAD:PAD + n].view(shp)
    nbytes = _lib.lib().ctclip_case_retrieval_ws_bytes(N, M, 24, 128)
    ws = torch.full((nbytes // 4 + 2 * PAD,), float('nan'), device='cuda')
    rc = _raw(case.q.cuda(), case.g.cuda(), case.qlab.cuda(), case.glab.cuda(), case.qgrp.cuda(), case.ggrp.cuda(),
              ks, rel, [outs[n] for n in OUTS], ws[PAD:], nbytes)
    torch.cuda.synchronize()
    assert rc == 0
    _assert_equal(types.SimpleNamespace(**outs), want)
    for name, (shp, dt) in shapes.items():
        for band in (bufs[name][:PAD], bufs[name][-PAD:]):
            assert bool(torch.isnan(band).all() if dt.is_floating_point else (band == 0x5a5a5a5a).all()), name
    assert bool(torch.isnan(ws[:PAD]).all()) and bool(torch.isnan(ws[PAD + nbytes // 4:]).all())
    behind = torch.arange(128, device='cuda')[None, :] >= outs['filled'][:, None]
    assert bool((outs['idx'][behind] == -1).all()) and bool((outs['score'][behind] == 0).all())
    assert bool((outs['idx'][~behind] >= 0).all())


def test_c_abi_refusals():
    from ctclip_mi355x import _lib
    CT_EINVAL, CT_ESHAPE = 1001, 1003
    case = C.exact_case(6, 9, 32, seed=1, groups='groups')
    q, g, ql, gl, qg, gg = (t.cuda() for t in (case.q, case.g, case.qlab, case.glab, case.qgrp, case.ggrp))
    outs = [torch.zeros(6, 5, dtype=torch.int32, device='cuda'), torch.zeros(6, 5, device='cuda'),
            torch.zeros(6, dtype=torch.int32, device='cuda'), torch.zeros(6, dtype=torch.int32, device='cuda'),
            torch.zeros(6, 2, dtype=torch.int32, device='cuda'), torch.zeros(6, 2, dtype=torch.float64, device='cuda'),
            torch.zeros(6, 2, dtype=torch.float64, device='cuda')]
    nbytes = _lib.lib().ctclip_case_retrieval_ws_bytes(6, 9, 32, 5)
    assert nbytes > 0 and _lib.lib().ctclip_case_retrieval_ws_bytes(6, 9, 32, 129) == 0
    assert _lib.lib().ctclip_case_retrieval_ws_bytes(65537, 9, 32, 5) == 0
    ws = torch.zeros(nbytes // 4, device='cuda')
    assert _raw(q, g, ql, gl, qg, gg, (1, 5), 0, outs, ws, nbytes) == 0
    assert _raw(q[:, :0], g[:, :0], ql, gl, qg, gg, (1, 5), 0, outs, ws, nbytes) == CT_ESHAPE          # Dl = 0
    assert _raw(q, g, ql, gl, qg, gg, (5, 5), 0, outs, ws, nbytes) == CT_EINVAL                       # not ascending
    assert _raw(q, g, ql, gl, qg, gg, (1, 5), 0, outs, ws, nbytes - 16) == CT_EINVAL                  # short workspace
    assert _raw(q, g, ql, gl, qg, None, (1, 5), 0, outs, ws, nbytes) == CT_EINVAL                     # one group pointer
    assert _raw(q, g, ql, gl, None, gg, (1, 5), 0, outs, ws, nbytes) == CT_EINVAL
    assert _raw(q, g, None, gl, qg, gg, (1, 5), 0, outs, ws, nbytes) == CT_EINVAL                     # a missing pointer
    assert _raw(q, g, ql, gl, qg, gg, (1, 5), 2, outs, ws, nbytes) == CT_EINVAL                       # rel_mode
    assert _raw(q, g, ql, gl, qg, gg, (1, 129), 0, outs, ws, nbytes) == CT_ESHAPE                     # K above 128
    torch.cuda.synchronize()


# -------------------------------------------------------------------------------------- custom op
def test_custom_op():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from ctclip_mi355x import ops  # noqa: F401
    case = C.exact_case(20, 70, 40, seed=5, groups='groups')
    args = [t.cuda() for t in (case.q, case.g, case.qlab, case.glab, case.qgrp, case.ggrp)]
    got = torch.ops.ctclip.case_retrieval(*args, [1, 5, 50], 'exact')
    want = _run(case, (1, 5, 50), 'exact')
    for a, name in zip(got, OUTS):
        assert torch.equal(a, getattr(want, name)), name
    utils = ('test_schema', 'test_faketensor', 'test_autograd_registration')
    torch.library.opcheck(torch.ops.ctclip.case_retrieval, (*args, [1, 5, 50], 'exact'), test_utils=utils)
    torch.library.opcheck(torch.ops.ctclip.case_retrieval, (*args[:4], None, None, [3]), test_utils=utils)
    with FakeTensorMode():
        fq, fg = torch.empty(300, 512, device='cuda'), torch.empty(1000, 512, device='cuda')
        fl = torch.empty(300, dtype=torch.int64, device='cuda'), torch.empty(1000, dtype=torch.int64, device='cuda')
        out = torch.ops.ctclip.case_retrieval(fq, fg, *fl, None, None, [1, 10, 100])
        assert [tuple(o.shape) for o in out] == [(300, 100), (300, 100), (300,), (300,), (300, 3), (300, 3), (300, 3)]
        assert [o.dtype for o in out] == [torch.int32, torch.float32, torch.int32, torch.int32, torch.int32,
                                          torch.float64, torch.float64]
    assert not any(o.requires_grad for o in got)


# --------------------------------------------------------------------------- evaluator and trainer
@pytest.fixture(scope='module')
def tiny():
    from test_gpu_model import build, cfg_small
    K = _K()
    torch.manual_seed(0)
    cfg = cfg_small()
    model = build(cfg)
    ids, mask = W.make_text(2, 32, cfg.bert.vocab_size, seed=7, ragged=True)
    text = types.SimpleNamespace(input_ids=ids.cuda(), attention_mask=mask.cuda())
    video = O.normalize_hu(W.make_hu(10, cfg.vit)).cuda()
    K.reset_ln_status()
    return cfg, model, text, video


LABELS6 = torch.tensor([[1, 0, 0, 1], [1, 0, 0, 0], [0, 0, 0, 0], [0, 1, 1, 0], [0, 0, 0, 0], [1, 0, 0, 1]])
GROUPS6 = torch.tensor([0, 0, 1, 2, -1, 3])                          # volumes 0 and 1: one scan; 4 hides nothing
LABELS4 = torch.tensor([[1, 0, 0, 1], [0, 0, 0, 0], [0, 1, 0, 0], [1, 1, 1, 1]])
GROUPS4 = torch.tensor([0, 5, 2, 9])


def _check_result(res, q, g, qlab, glab, qgrp, ggrp, ks, rel):
    """The evaluator's dict against the restatement on the latents it returned: counts equal, scores within
    the f32 bound, the lists equal wherever no float64 gap is below 1e-6, hits / ap / gain the restatement's
    bits on the returned lists, and the host metrics the helpers' values on those outputs."""
    from ctclip_mi355x.retrieval import map_at_k, mean_jaccard_at_k, precision_at_k
    want = C.reference(q, g, qlab, glab, qgrp, ggrp, ks, rel)
    got = types.SimpleNamespace(**{n: res[n] for n in OUTS})
    _assert_equal(got, want, ('filled', 'nrel'))
    assert (res['score'].cpu().double() - want.score).abs().max().item() <= (2 * q.shape[1] + 8) * 2.0 ** -24
    clear = C.clear_queries(want, ks[-1])
    print(f'{int(clear.sum())} of {clear.numel()} queries without a float64 gap below 1e-6')
    assert torch.equal(res['idx'].cpu()[clear], want.idx[clear])
    own = types.SimpleNamespace()
    own.hits, own.ap, own.gain = C.metrics_on_lists(res['idx'], qlab, glab, want.nrel, ks, rel)
    _assert_equal(got, own, ('hits', 'ap', 'gain'))
    m, n = map_at_k(own.ap)
    assert res['n_scored'] == n == int((want.nrel > 0).sum())
    assert torch.equal(res['map'], m) and torch.equal(res['precision'], precision_at_k(own.hits, want.filled, ks))
    assert torch.equal(res['mean_jaccard'], mean_jaccard_at_k(own.gain, want.filled, ks))
    if n:
        assert torch.allclose(res['map'], own.ap[own.ap[:, 0] != -1].mean(0), rtol=1e-14, atol=0)
    assert res['map'].dtype == res['precision'].dtype == res['mean_jaccard'].dtype == torch.float64
    assert not res['map'].is_cuda and res['ks'] == tuple(ks)


def test_evaluator(tiny):
    from ctclip_mi355x.retrieval import CaseRetrievalEvaluator, pack_labels
    cfg, model, text, video = tiny
    ev = CaseRetrievalEvaluator(model)
    ks = (1, 2, 5)
    qlab = pack_labels(LABELS6)
    # the six volumes against themselves, hand-set groups
    res = ev.evaluate(video[:6], LABELS6, GROUPS6, ks=ks, n_boot=20, batch_size=4)
    q = res['image_latents']
    assert q.shape == (6, cfg.dim_latent) and 'gallery_latents' not in res
    _check_result(res, q, q, qlab, qlab, GROUPS6, GROUPS6, ks, 'any')
    assert res['filled'].tolist() == [4, 4, 5, 5, 5, 5]          # K_max = 5 caps query 4's six rows
    assert set(res['ci']) == {'map', 'precision', 'mean_jaccard'}
    for t in res['ci'].values():
        assert t.shape == (3, len(ks)) and t.dtype == torch.float64
    # groups=None: every volume is its own group; exclude_self=False: the query finds itself first
    res1 = ev.evaluate([video[:4], video[4:6]], LABELS6.float(), ks=ks, rel='exact', batch_size=3)
    assert torch.equal(res1['image_latents'], q) and res1['ci'] is None
    ar = torch.arange(6)
    _check_result(res1, q, q, qlab, qlab, ar, ar, ks, 'exact')
    res2 = ev.evaluate(video[:6], qlab, ks=ks, exclude_self=False)
    _check_result(res2, q, q, qlab, qlab, None, None, ks, 'any')
    assert res2['idx'][:, 0].tolist() == list(range(6))
    # a separate gallery of four volumes, with and without groups
    glab = pack_labels(LABELS4)
    res3 = ev.evaluate(video[:6], LABELS6, GROUPS6, gallery_volumes=video[6:10], gallery_labels=LABELS4,
                       gallery_groups=GROUPS4, ks=ks, n_boot=5)
    g = res3['gallery_latents']
    assert g.shape == (4, cfg.dim_latent) and torch.equal(res3['image_latents'], q)
    _check_result(res3, q, g, qlab, glab, GROUPS6, GROUPS4, ks, 'any')
    assert res3['filled'].tolist() == [3, 3, 4, 3, 4, 4]
    res4 = ev.evaluate(video[:6], LABELS6, gallery_volumes=video[6:10], gallery_labels=LABELS4, ks=ks)
    _check_result(res4, q, g, qlab, glab, None, None, ks, 'any')


def test_validate_case_retrieval_keeps_the_training_state(tiny):
    K = _K()
    from ctclip_mi355x.retrieval import pack_labels
    from ctclip_mi355x.trainer import CTClipTrainer, EvalGuardError
    cfg, model, text, video = tiny
    K.reset_ln_status()
    model.train()
    tr = CTClipTrainer(model, lr=1e-3)
    tr.train_step(text, video[:2])
    tr.flush()
    word = K.status_word(video.device)
    snap = word.clone()
    codebook = model.visual_transformer.vq._codebook.embed.clone()
    assert model.training
    res = tr.validate_case_retrieval(video[:6], LABELS6, GROUPS6, ks=(1, 5), n_boot=4, batch_size=3)
    assert model.training and torch.equal(word, snap)
    assert torch.equal(model.visual_transformer.vq._codebook.embed, codebook)      # no EMA from the pass
    qlab = pack_labels(LABELS6)
    q = res['image_latents']
    _check_result(res, q, q, qlab, qlab, GROUPS6, GROUPS6, (1, 5), 'any')
    assert res['ci']['map'].shape == (3, 2)
    bad = video[:6].clone()
    bad[1, 0, 17, 33, 71] = float('nan')
    with pytest.raises(EvalGuardError) as ei:
        tr.validate_case_retrieval(bad, LABELS6)
    assert ei.value.bits != 0 and model.training and torch.equal(word, snap)
    before = tr.flat.data.clone()
    loss = tr.train_step(text, video[:2])
    tr.check()
    assert torch.isfinite(loss) and not torch.equal(before, tr.flat.data)
    model.eval()
    tr.validate_case_retrieval(video[:2], LABELS6[:2])
    assert not model.training
    model.train()
