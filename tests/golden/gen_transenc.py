"""Generate the TransformerSequenceEncoder fixtures by running the REFERENCE implementation.

Container-only tool, like gen_convenc.py: it imports the reference's ``src/encoders.py``
(read-only, never copied) and writes ``transenc_train.npz`` / ``transenc_eval.npz`` (and their
``.part<N>.npz`` files, gen_golden.save_fixture) next to this file.  The GPU box never runs it.

Both records are the reference's ``SequenceEncoder(17, 16, 16, num_layers=1,
encoder_type="transformer", dropout=0.0)`` on a (3, 37, 17) input with lengths [37, 20, 1], float32
on the CPU at matmul precision "highest", once in train mode and once in eval mode (with gradients
enabled, so torch's inference fast path stays off and the two modes compute the same thing).
Each holds the state dict (``sd/<key>``, in state_dict order), the input ``x``, ``lengths``, the
upstream gradient ``gout``, the output ``out``, ``dx`` and every parameter gradient
(``grad/<key>``) of sum(out * gout).

Run:  python tests/golden/gen_transenc.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

from gen_golden import save_fixture

REF_SRC = Path("/root/reference/src")
SHAPE = (3, 37, 17)
LENGTHS = (37, 20, 1)
HIDDEN, OUT = 16, 16


def main() -> None:
    sys.path.insert(0, str(REF_SRC))
    import encoders as ref_encoders
    torch.set_float32_matmul_precision("highest")
    for name, train in (("transenc_train", True), ("transenc_eval", False)):
        torch.manual_seed(21 if train else 22)
        enc = ref_encoders.SequenceEncoder(SHAPE[2], HIDDEN, OUT, num_layers=1, encoder_type="transformer",
                                           dropout=0.0)
        with torch.no_grad():
            for layer in enc.transformer.layers:
                for norm in (layer.norm1, layer.norm2):
                    norm.weight.uniform_(0.5, 1.5)
                    norm.bias.uniform_(-0.5, 0.5)
                layer.self_attn.in_proj_bias.uniform_(-0.1, 0.1)
                layer.self_attn.out_proj.bias.uniform_(-0.1, 0.1)
        enc.train(train)
        rec = {f"sd/{k}": v.detach().clone().numpy() for k, v in enc.state_dict().items()}
        x = torch.randn(*SHAPE, requires_grad=True)
        gout = torch.randn(SHAPE[0], OUT)
        lengths = torch.tensor(LENGTHS, dtype=torch.int64)
        out = enc(x, lengths)
        (out * gout).sum().backward()
        rec.update(x=x.detach().numpy(), lengths=lengths.numpy(), gout=gout.numpy(), out=out.detach().numpy(),
                   dx=x.grad.numpy())
        for k, p in enc.named_parameters():
            rec[f"grad/{k}"] = p.grad.numpy()
        assert all(np.isfinite(v).all() for v in rec.values())
        save_fixture(name, rec)


if __name__ == "__main__":
    main()
