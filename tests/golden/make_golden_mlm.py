"""Golden fixture for masked-language-model pretraining: the reference's own ``MLM`` class
(ct_clip/mlm.py) run on CPU.

Run in the build container only (needs the reference checkout, see make_golden.py):
    python tests/golden/make_golden_mlm.py

The reference class was written for a transformer that returns (B, L + 1, D) hidden states with a CLS
column in front (its built-in TextTransformer), so the transformer here is a stub that returns a fixed
table of that shape and records the ``masked_seq`` it is given.  B = 3, L = 16, D = 64, V = 257; CLS = 101
and SEP = 102 are in ``mask_ignore_token_ids``, pad = 0, mask = 2.  Rows:

  0  all pad                          n_b = 0
  1  one token at position 5, pads    n_b = 1
  2  CLS, 14 tokens, SEP              n_b = 14

On these rows the reference selects exactly ceil(0.15 * n_b) positions per row (0, 1, 3) that carry a
label: its ``mask_excess`` slice never trims here, the surplus slots of rows 0 and 1 fall on pads, whose
label is the ignore index, and row 2 fills all ceil(0.15 * 16) = 3 slots with eligible positions.

Saved: ids, masked_ids (recorded by the stub), labels (the target F.cross_entropy is called with),
hidden (the stub's table), weight / bias of ``to_logits`` and the reference's loss.  The fixture is DATA;
nothing of the reference's source is copied into it.
"""
from __future__ import annotations

import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as G  # noqa: E402  (sets up sys.path and the import-time stubs)
import torch  # noqa: E402
from safetensors.torch import save_file  # noqa: E402

B, L, D, V = 3, 16, 64, 257
CLS, SEP, PAD, MASK = 101, 102, 0, 2


class _Stub(torch.nn.Module):
    def __init__(self, table):
        super().__init__()
        self.table = table
        self.seen = None

    def forward(self, masked_seq, **kw):
        self.seen = masked_seq.detach().clone()
        return self.table


def main():
    G.import_reference()
    import ct_clip.mlm as R
    g = torch.Generator().manual_seed(20)
    ids = torch.zeros(B, L, dtype=torch.int64)
    ids[1, 5] = 57
    ids[2, 0], ids[2, L - 1] = CLS, SEP
    ids[2, 1:L - 1] = torch.randint(110, V, (L - 2,), generator=g)
    hidden = torch.randn(B, L + 1, D, generator=g)
    stub = _Stub(hidden)
    torch.manual_seed(7)
    mlm = R.MLM(stub, dim=D, num_tokens=V, mask_token_id=MASK, pad_token_id=PAD, mask_ignore_token_ids=[CLS, SEP])
    with torch.no_grad():
        mlm.to_logits.weight.copy_(torch.randn(V, D, generator=g) * 0.1)
        mlm.to_logits.bias.copy_(torch.randn(V, generator=g) * 0.1)
    cap = {}
    ce = R.F.cross_entropy

    def record(logits, target, **kw):
        cap['labels'] = target.detach().clone()
        return ce(logits, target, **kw)
    R.F.cross_entropy = record
    try:
        torch.manual_seed(11)
        with torch.no_grad():
            loss = mlm(ids)
    finally:
        R.F.cross_entropy = ce
    labels = cap['labels']
    counts = (labels != PAD).sum(-1).tolist()
    assert counts == [0, 1, 3], counts
    out = {'ids': ids, 'masked_ids': stub.seen, 'labels': labels, 'hidden': hidden,
           'weight': mlm.to_logits.weight.detach().clone(), 'bias': mlm.to_logits.bias.detach().clone(),
           'loss': loss.detach().reshape(1).float()}
    path = os.path.join(HERE, 'golden_mlm.safetensors')
    save_file({k: v.contiguous() for k, v in out.items()}, path)
    print(path, os.path.getsize(path), 'bytes; loss', float(loss), 'labelled per row', counts)


if __name__ == '__main__':
    main()
