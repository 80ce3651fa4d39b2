"""Generate the ConvSequenceEncoder fixtures by running the REFERENCE implementation.

Container-only tool, like gen_golden.py: it imports the reference's ``src/encoders.py``
(read-only, never copied) and writes ``convenc_eval.npz`` / ``convenc_train.npz`` next to
this file.  The GPU box never runs it.

Both records are the reference's ``SequenceEncoder(17, 64, 16, encoder_type="cnn")`` on a
(3, 37, 17) input, float32 on the CPU at matmul precision "highest":
  * convenc_eval:  ``.eval()`` with non-trivial running statistics;
  * convenc_train: train mode, ``dropout=0.0``.
Each holds the state dict before the forward (``sd/<key>``), the input ``x``, the upstream
gradient ``gout``, the output ``out``, ``dx``, every parameter gradient (``grad/<key>``) of
sum(out * gout), and the BatchNorm buffers after the forward (``post/<key>``).

Run:  python tests/golden/gen_convenc.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
REF_SRC = Path("/root/reference/src")
SHAPE = (3, 37, 17)
HIDDEN, OUT = 64, 16


def main() -> None:
    sys.path.insert(0, str(REF_SRC))
    import encoders as ref_encoders
    torch.set_float32_matmul_precision("highest")
    for name, train in (("convenc_eval", False), ("convenc_train", True)):
        torch.manual_seed(11 if train else 12)
        enc = ref_encoders.SequenceEncoder(SHAPE[2], HIDDEN, OUT, encoder_type="cnn", dropout=0.0)
        with torch.no_grad():
            for i in (1, 4):
                bn = enc.conv_net[i]
                bn.weight.uniform_(0.5, 1.5)
                bn.bias.uniform_(-0.5, 0.5)
                bn.running_mean.normal_(0.0, 0.5)
                bn.running_var.uniform_(0.5, 1.5)
                bn.num_batches_tracked.fill_(3)
        enc.train(train)
        rec = {f"sd/{k}": v.detach().clone().numpy() for k, v in enc.state_dict().items()}
        x = torch.randn(*SHAPE, requires_grad=True)
        gout = torch.randn(SHAPE[0], OUT)
        out = enc(x)
        (out * gout).sum().backward()
        rec.update(x=x.detach().numpy(), gout=gout.numpy(), out=out.detach().numpy(), dx=x.grad.numpy())
        for k, p in enc.named_parameters():
            rec[f"grad/{k}"] = p.grad.numpy()
        for k, b in enc.named_buffers():
            rec[f"post/{k}"] = b.detach().numpy()
        path = HERE / f"{name}.npz"
        np.savez_compressed(path, **rec)
        print(f"{path.name}: {path.stat().st_size} bytes, {len(rec)} arrays")
        assert path.stat().st_size < (1 << 20)


if __name__ == "__main__":
    main()
