"""Generate the GRUSequenceEncoder fixtures by running the REFERENCE implementation.

Container-only tool, like gen_convenc.py: it imports the reference's ``src/encoders.py``
(read-only, never copied) and writes ``gruenc_2layer_len.npz`` / ``gruenc_h128.npz`` next to
this file.  The GPU box never runs it.

Both records are the reference's ``SequenceEncoder(..., encoder_type="gru", dropout=0.0)``,
float32 on the CPU at matmul precision "highest":
  * gruenc_2layer_len: (17, 64, 16), 2 layers, input (3, 37, 17), lengths [37, 12, 1], ``.eval()``;
  * gruenc_h128:       (9, 128, 32), 1 layer, input (2, 11, 9), no lengths, train mode.
Each holds the state dict (``sd/<key>``), the input ``x``, ``lengths`` (if any), the upstream
gradient ``gout``, the output ``out``, ``dx`` and every parameter gradient (``grad/<key>``) of
sum(out * gout).

Run:  python tests/golden/gen_gruenc.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
REF_SRC = Path("/root/reference/src")
# name, (input_dim, hidden, out), layers, input shape, lengths, train, seed
CASES = (
    ("gruenc_2layer_len", (17, 64, 16), 2, (3, 37, 17), [37, 12, 1], False, 21),
    ("gruenc_h128", (9, 128, 32), 1, (2, 11, 9), None, True, 22),
)


def main() -> None:
    sys.path.insert(0, str(REF_SRC))
    import encoders as ref_encoders
    torch.set_float32_matmul_precision("highest")
    for name, (din, hidden, out_dim), layers, shape, lengths, train, seed in CASES:
        torch.manual_seed(seed)
        enc = ref_encoders.SequenceEncoder(din, hidden, out_dim, num_layers=layers, encoder_type="gru", dropout=0.0)
        enc.train(train)
        rec = {f"sd/{k}": v.detach().clone().numpy() for k, v in enc.state_dict().items()}
        x = torch.randn(*shape, requires_grad=True)
        gout = torch.randn(shape[0], out_dim)
        lens = torch.tensor(lengths) if lengths is not None else None
        out = enc(x, lens)
        (out * gout).sum().backward()
        rec.update(x=x.detach().numpy(), gout=gout.numpy(), out=out.detach().numpy(), dx=x.grad.numpy())
        if lens is not None:
            rec["lengths"] = lens.numpy()
        for k, p in enc.named_parameters():
            rec[f"grad/{k}"] = p.grad.numpy()
        path = HERE / f"{name}.npz"
        np.savez_compressed(path, **rec)
        print(f"{path.name}: {path.stat().st_size} bytes, {len(rec)} arrays")
        assert path.stat().st_size < (1 << 20)


if __name__ == "__main__":
    main()
