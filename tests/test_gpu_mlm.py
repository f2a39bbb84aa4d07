"""Masked-language-model pretraining on the GPU (ctclip_mi355x/mlm.py, csrc/mlm.hip).

* the mask kernel against ``ref_mask`` below, a torch restatement of the same hash stream (bit-exact);
* the head's loss against the reference fixture (tests/golden/make_golden_mlm.py), within 1e-3 -- the bf16
  path's bound of SURVEY §8(c);
* the head forward / backward against float64 on the operands the kernels use, rounded to bf16 where the
  kernels round them (the forward GEMM reads hi + lo bf16 pairs of both operands, the backward GEMMs the
  bf16 images).  Tolerances, none of them taken from this code:
    - GEMM results (logits through the loss, dW, dH): relative Frobenius error 1e-5, what
      tests/test_gpu_gemm.py allows bf16-operand / f32-accumulate products at every K it runs
      (64 .. 65,536);
    - loss: 1e-5 * max(1, |loss|) -- log-sum-exp moves by at most the largest logit error;
    - dlogits (softmax - onehot) / count: 2e-5 relative Frobenius -- a softmax entry is a ratio of two
      exponentials of logits, each off by at most the logit error;
    - db: a sum of M <= 8 f32 terms, |error| <= M * 2^-24 * sum |term| per column.
  Measured maxima are in DESIGN.md §23;
* structure (the logit buffer has B * ceil(p L) rows; bit-identical repeats) and an end-to-end run on a
  64-wide, 2-layer BERT: finite loss near ln(vocab), every gradient filled, the word-embedding gradient
  against a finite-difference probe, ten Adam steps lowering the loss.
"""
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'golden_mlm.safetensors')
dev = 'cuda'
M64 = (1 << 64) - 1
PAD, MASK, CLS, SEP = 0, 2, 101, 102


# ------------------------------------------------------------------------------ hash restatement
def _s64(x):
    x &= M64
    return x - (1 << 64) if x >= (1 << 63) else x


def _lsr(x, n):
    return (x >> n) & ((1 << (64 - n)) - 1)


def _u32(seed, s, idx):
    """Upper 32 bits of fmix64((seed ^ s * C) ^ idx * PHI) for an int64 tensor idx (int64 arithmetic wraps
    like the kernel's uint64; shifts made logical by masking)."""
    x = (idx * _s64(0x9E3779B97F4A7C15)) ^ _s64(seed ^ ((s * 0xBF58476D1CE4E5B9) & M64))
    x = x ^ _lsr(x, 33)
    x = x * _s64(0xff51afd7ed558ccd)
    x = x ^ _lsr(x, 33)
    x = x * _s64(0xc4ceb9fe1a85ec53)
    x = x ^ _lsr(x, 33)
    return _lsr(x, 32)


def ref_mask(ids, seed, *, mask_prob, replace_prob, random_token_prob, num_tokens, ignore):
    ids = ids.cpu()
    B, L = ids.shape
    m_max = math.ceil(mask_prob * L)
    gi = torch.arange(B * L, dtype=torch.int64).view(B, L)
    ign = torch.tensor(sorted(set(ignore) | {PAD}), dtype=torch.int64)
    elig = ~torch.isin(ids, ign)
    big = 1 << 62
    key = torch.where(elig, _u32(seed, 0, gi) * 512 + torch.arange(L), torch.full_like(ids, big))
    rank = (key[:, :, None] > key[:, None, :]).sum(-1)
    c = torch.tensor([min(math.ceil(int(n) * mask_prob), m_max) for n in elig.sum(-1)])
    selected = elig & (rank < c[:, None])
    labels = torch.where(selected, ids, torch.full_like(ids, PAD))
    masked = ids.clone()
    rnd = torch.zeros_like(elig)
    t_rnd = int(random_token_prob * 4294967296.0)
    if t_rnd:
        tok = (_u32(seed, 3, gi) * num_tokens) >> 32
        rnd = (_u32(seed, 2, gi) < t_rnd) & ~torch.isin(tok, ign)
        masked = torch.where(rnd, tok, masked)
    rep = selected & ~rnd & (_u32(seed, 1, gi) < int(replace_prob * 4294967296.0))
    masked[rep] = MASK
    sel = torch.full((B, m_max), -1, dtype=torch.int32)
    b, l = selected.nonzero(as_tuple=True)
    sel[b, rank[b, l]] = gi[b, l].int()
    return masked, labels, sel.view(-1), elig, c


def _ids(L, V=1000, seed=0):
    """Row 0: all pad (n_b = 0); row 1: one token (n_b = 1); row 2: CLS, tokens, SEP, pads; row 3: no pad,
    ignored ids sprinkled in."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(4, L, dtype=torch.int64)
    ids[1, L // 3] = 57
    n = (3 * L) // 4
    ids[2, :n] = torch.randint(110, V, (n,), generator=g)
    ids[2, 0], ids[2, n - 1] = CLS, SEP
    ids[3] = torch.randint(110, V, (L,), generator=g)
    ids[3, ::5] = CLS
    return ids


@pytest.mark.parametrize('L,p,rp,rtp', [(16, 0.15, 0.9, 0.0), (512, 0.15, 0.9, 0.0), (16, 0.4, 0.5, 0.3),
                                        (100, 0.15, 1.0, 0.1)])
def test_mask_matches_restatement(L, p, rp, rtp):
    from ctclip_mi355x import kernels as K
    ids = _ids(L)
    kw = dict(mask_prob=p, replace_prob=rp, random_token_prob=rtp, num_tokens=1000)
    for seed in (0x1234567890ABCDEF, 7):
        masked, labels, sel = K.mlm_mask(ids.to(dev), seed=seed, mask_token_id=MASK, pad_token_id=PAD,
                                         ignore_ids=[CLS, SEP, PAD], **kw)
        rm, rl, rs, elig, c = ref_mask(ids, seed, ignore=[CLS, SEP], **kw)
        assert torch.equal(masked.cpu(), rm) and torch.equal(labels.cpu(), rl) and torch.equal(sel.cpu(), rs)
        picked = labels.cpu() != PAD
        assert picked.sum(-1).tolist() == [math.ceil(p * int(n)) for n in elig.sum(-1)]
        assert picked.sum(-1).tolist()[:2] == [0, math.ceil(p)]
        assert not bool((picked & ~elig).any())
        sel = sel.cpu().view(4, -1)
        assert sel.shape[1] == math.ceil(p * L)
        assert ((sel >= 0).sum(-1) == picked.sum(-1)).all()
        flat = sel[sel >= 0].long()
        assert flat.unique().numel() == flat.numel() and bool(picked.view(-1)[flat].all())
        if rtp == 0:
            changed = masked.cpu() != ids
            assert not bool((changed & ~picked).any()) and bool((masked.cpu()[changed] == MASK).all())


def test_mask_stream_and_fixture_counts():
    from safetensors.torch import load_file
    from ctclip_mi355x import MLM
    g = load_file(GOLDEN)
    ids = g['ids'].to(dev)
    m = MLM(None, dim=64, num_tokens=257, mask_token_id=MASK, pad_token_id=PAD, mask_ignore_token_ids=[CLS, SEP])
    torch.manual_seed(3)
    a = m.mask(ids)
    b = m.mask(ids)
    assert m.mask_state() == 2
    # the reference's per-row masked counts on the same ids (its labels; the masked ids it recorded differ
    # from the ids only where it selected)
    ref_counts = (g['labels'] != PAD).sum(-1)
    assert not bool(((g['masked_ids'] != g['ids']) & (g['labels'] != PAD) & (g['masked_ids'] != MASK)).any())
    for out in (a, b):
        assert torch.equal((out[1].cpu() != PAD).sum(-1), ref_counts)
    assert not torch.equal(a[1], b[1]) or not torch.equal(a[0], b[0])       # the next call: another mask
    m.set_mask_state(0)
    a2 = m.mask(ids)
    assert all(torch.equal(x, y) for x, y in zip(a, a2))                    # same seed, same mask
    m.set_mask_state(1)
    b2 = m.mask(ids)
    assert all(torch.equal(x, y) for x, y in zip(b, b2))                    # a replayed call
    torch.manual_seed(4)
    m.set_mask_state(0)
    a3 = m.mask(g['ids'].to(dev).repeat(8, 1))                              # 24 rows: the seed matters
    torch.manual_seed(3)
    m.set_mask_state(0)
    a4 = m.mask(g['ids'].to(dev).repeat(8, 1))
    assert not torch.equal(a3[1], a4[1])
    # the module's seed: torch.initial_seed() and the call counter, nothing else
    seed = ((3 * 0x2545F4914F6CDD1D + 1 * 0x9E3779B97F4A7C15) ^ 0x94D049BB133111EB) & M64
    rm, rl, rs, _, _ = ref_mask(g['ids'], seed, mask_prob=0.15, replace_prob=0.9, random_token_prob=0.0,
                                num_tokens=257, ignore=[CLS, SEP])
    assert torch.equal(a[0].cpu(), rm) and torch.equal(a[1].cpu(), rl) and torch.equal(a[2].cpu(), rs)


def _sel_of(labels, m_max):
    """Selection list of a label tensor [B, L]: the labelled positions of each row, m_max slots per row."""
    B, L = labels.shape
    sel = torch.full((B, m_max), -1, dtype=torch.int32)
    for b in range(B):
        pos = (labels[b] != PAD).nonzero().view(-1)
        assert pos.numel() <= m_max
        sel[b, :pos.numel()] = (b * L + pos).int()
    return sel.view(-1)


def test_loss_matches_reference_fixture():
    from safetensors.torch import load_file
    from ctclip_mi355x import functional as Fn
    g = load_file(GOLDEN)
    hidden = g['hidden'][:, 1:].contiguous().to(dev)
    labels = g['labels'].to(dev)
    sel = _sel_of(g['labels'], 3).to(dev)
    W, b = g['weight'].to(dev).requires_grad_(True), g['bias'].to(dev).requires_grad_(True)
    loss = Fn.MlmHeadFn.apply(hidden, sel, labels, W, b)
    print(f'fixture loss: ours {loss.item():.6f}, reference {g["loss"].item():.6f}')
    assert abs(loss.item() - g['loss'].item()) < 1e-3


def _rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


@pytest.mark.parametrize('D,V,M', [(64, 257, 6), (768, 30522, 8)])
def test_head_forward_backward_vs_float64(D, V, M):
    from ctclip_mi355x import functional as Fn
    from ctclip_mi355x import kernels as K
    torch.manual_seed(5)
    R = 2 * M + 3
    hidden = torch.randn(R, D, device=dev)
    W = (torch.randn(V, D, device=dev) * 0.02).requires_grad_(True)
    b = (torch.randn(V, device=dev) * 0.02).requires_grad_(True)
    rows = torch.randperm(R)[:M].int()
    rows[2] = -1                                          # an unused slot
    sel = rows.to(dev)
    labels = torch.zeros(R, dtype=torch.int64, device=dev)
    labels[rows[rows >= 0].long().to(dev)] = torch.randint(1, V, (M - 1,), device=dev)
    labels[rows[0].item()] = V - 1                        # in the last, partial tile of V
    labels[rows[1].item()] = V - (V % 8) if V % 8 else V - 8
    valid = rows >= 0
    n_valid = int(valid.sum())
    Vp = K.mlm_pad_cols(V)
    # ---- the kernels' own buffers
    wp, wl, bp = Fn.mlm_weight(W, b)
    assert torch.equal(wp[:V], W.detach().bfloat16()) and not bool(wp[V:].any()) and tuple(wp.shape) == (Vp, D)
    assert torch.equal(wl[:V], (W.detach() - wp[:V].float()).bfloat16()) and not bool(wl[V:].any())
    assert torch.equal(bp[:V], b.detach()) and not bool(bp[V:].any())
    loss, count, hsel, hlo, dlog, dlb = K.mlm_head_fwd(hidden, sel, labels, wp, wl, bp, V)
    assert tuple(dlog.shape) == (M, Vp) and count.item() == n_valid
    safe = rows.clamp_min(0).long().to(dev)
    hs_ref = hidden[safe].bfloat16() * valid.to(dev)[:, None]
    assert torch.equal(hsel, hs_ref)
    assert torch.equal(hlo, (hidden[safe] - hidden[safe].bfloat16().float()).bfloat16() * valid.to(dev)[:, None])
    # ---- float64 on the same operands: the forward reads hi + lo pairs and drops the lo . lo product
    z = (hsel.double() @ (wp[:V].double() + wl[:V].double()).t() + hlo.double() @ wp[:V].double().t()
         + b.detach().double())
    tgt = labels[safe]
    lse = torch.logsumexp(z, -1)
    row_loss = (lse - z.gather(1, tgt[:, None])[:, 0])[valid.to(dev)]
    loss_ref = row_loss.sum() / n_valid
    g_ref = torch.softmax(z, -1)
    g_ref[torch.arange(M, device=dev), tgt] -= 1
    g_ref = g_ref / n_valid * valid.to(dev)[:, None]
    e_loss = abs(loss.item() - loss_ref.item())
    e_dlog = _rel(dlog[:, :V], g_ref)
    print(f'(D, V, M) = {(D, V, M)}: loss {loss.item():.6f} |d| {e_loss:.2e}, dlogits rel {e_dlog:.2e}')
    assert e_loss <= 1e-5 * max(1.0, abs(loss_ref.item()))
    assert e_dlog < 2e-5
    assert not bool(dlog[:, V:].any()) and not bool(dlog[2].any())
    assert torch.equal(dlb, dlog.bfloat16())
    # ---- through autograd
    h = hidden.clone().requires_grad_(True)
    out = Fn.MlmHeadFn.apply(h, sel, labels, W, b)
    assert torch.equal(out.reshape(1), loss)
    out.backward()
    dW_ref = (dlb.double().t() @ hsel.double())[:V]
    dsel_ref = dlb.double() @ wp.double()
    dH_ref = torch.zeros(R, D, dtype=torch.float64, device=dev)
    dH_ref[safe[valid.to(dev)]] = dsel_ref[valid.to(dev)]
    db_ref = dlog.double().sum(0)[:V]
    e_dw, e_dh = _rel(W.grad, dW_ref), _rel(h.grad, dH_ref)
    e_db = ((b.grad.double() - db_ref).abs() - M * 2.0 ** -24 * dlog.double().abs().sum(0)[:V]).max().item()
    print(f'  dW rel {e_dw:.2e}, dH rel {e_dh:.2e}, db excess over bound {e_db:.2e}, '
          f'db vs f64 gradient rel {_rel(b.grad, g_ref.sum(0)):.2e}')
    assert e_dw < 1e-5 and e_dh < 1e-5 and e_db <= 0
    assert _rel(b.grad, g_ref.sum(0)) < 2e-5
    unsel = torch.ones(R, dtype=torch.bool, device=dev)
    unsel[safe[valid.to(dev)]] = False
    assert not bool(h.grad[unsel].any())


def _tiny(vocab=1000):
    from ctclip_mi355x import MLM
    from ctclip_mi355x.bert import BertConfig, BertModel
    torch.manual_seed(0)
    bert = BertModel(BertConfig(vocab_size=vocab, hidden_size=64, num_hidden_layers=2, num_attention_heads=2,
                                intermediate_size=256, max_position_embeddings=64, hidden_dropout_prob=0.0,
                                attention_probs_dropout_prob=0.0))
    m = MLM(bert, dim=64, num_tokens=vocab, mask_token_id=4, pad_token_id=PAD, mask_ignore_token_ids=[2, 3]).to(dev)
    from oracle import weights as Wt
    ids, mask = Wt.make_text(4, 16, vocab, ragged=True)
    return m, ids.to(dev), mask.to(dev)


def test_structure_rows_and_bit_identical_repeats():
    from ctclip_mi355x import functional as Fn
    from ctclip_mi355x import kernels as K
    m, ids, mask = _tiny()
    B, L = ids.shape
    masked, labels, sel = m.mask(ids)
    assert sel.numel() == B * math.ceil(0.15 * L) == 12
    hidden = m.transformer(masked, attention_mask=mask)[0].detach()
    wp, wl, bp = Fn.mlm_weight(m.to_logits.weight, m.to_logits.bias)
    dlog = K.mlm_head_fwd(hidden.view(B * L, -1), sel, labels.view(-1), wp, wl, bp, 1000)[4]
    assert dlog.shape[0] == B * math.ceil(0.15 * L) and dlog.shape[0] < B * L
    runs = []
    for _ in range(2):
        m.zero_grad(set_to_none=True)
        m.set_mask_state(0)
        loss = m(ids, attention_mask=mask)
        loss.backward()
        torch.cuda.synchronize()
        runs.append([loss.detach().clone()] + [p.grad.clone() for p in m.parameters() if p.grad is not None])
    assert len(runs[0]) == len(runs[1]) > 10
    assert all(torch.equal(x, y) for x, y in zip(*runs))


def test_end_to_end_tiny_bert():
    m, ids, mask = _tiny()
    m.set_mask_state(0)
    loss = m(ids, attention_mask=mask)
    loss.backward()
    torch.cuda.synchronize()
    print(f'tiny BERT MLM loss at init {loss.item():.4f} (ln 1000 = {math.log(1000):.4f})')
    assert math.isfinite(loss.item()) and abs(loss.item() - math.log(1000)) < 0.5
    for n, p in m.named_parameters():
        if n.startswith('transformer.pooler.'):
            continue
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and bool(p.grad.any()), n
    # ---- finite differences on the word table (the gradient path through every position)
    we = m.transformer.embeddings.word_embeddings.weight
    g = we.grad.clone()
    # Central differences of the module's own loss (hidden states recomputed, mask pinned), the six entries
    # of largest gradient.  Step 1e-2 against embedding rows of spread ~0.035: the third-order term is
    # (0.29)^2 / 6 ~ 1.4 % of the derivative -> 5 % relative.  The loss is computed through bf16
    # activations: ~10 rounding sites of 2^-9 relative error on the ~3 of 12 rows a perturbed sequence
    # holds move it by ~1e-4 between the two evaluations, i.e. 7e-3 in the quotient -> 1e-2 absolute.
    m.set_mask_state(0)
    masked_ids = m.mask(ids)[0]
    used = masked_ids.unique()
    top = g[used].abs().flatten().topk(6).indices
    eps = 1e-2
    for t in top.tolist():
        r, c = used[t // 64].item(), t % 64
        vals = []
        for sgn in (1, -1):
            with torch.no_grad():
                we[r, c] += sgn * eps
            m.set_mask_state(0)
            with torch.no_grad():
                vals.append(m(ids, attention_mask=mask).double().item())
            with torch.no_grad():
                we[r, c] -= sgn * eps
        fd = (vals[0] - vals[1]) / (2 * eps)
        print(f'  d loss / d word[{r}, {c}]: analytic {g[r, c].item():+.5e}, finite difference {fd:+.5e}')
        assert abs(fd - g[r, c].item()) <= 0.05 * abs(g[r, c].item()) + 1e-2
    # ---- ten Adam steps on the fixed batch with the pinned mask
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    losses = []
    for _ in range(10):
        opt.zero_grad(set_to_none=True)
        m.set_mask_state(0)
        loss = m(ids, attention_mask=mask)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    print('  Adam losses', ' '.join(f'{x:.4f}' for x in losses))
    assert losses[-1] < losses[0] - 0.05 and all(math.isfinite(x) for x in losses)
