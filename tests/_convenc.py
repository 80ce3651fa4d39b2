"""Helpers of the ConvSequenceEncoder tests: the plain torch.nn comparator (the reference's
nn.Sequential, src/encoders.py:87-97 / 168-175, on the CPU in float64 or float32), the parity
cases and their preconditions."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, Optional

import torch
import torch.nn as nn

from _util import close, diff_report, zero_grad_bound

OUT_DIM = 16
BIAS_KEYS = ("conv_net.0.bias", "conv_net.3.bias")
# Device noise allowed in the (mathematically zero) train-mode conv bias gradients, as a multiple of
# fp32 torch's own largest element there: the device sums the same dy values in another order, so it
# gets 4x fp32 torch's noise, not a different algorithm's.
ZERO_GRAD_C = 4.0


@dataclass(frozen=True)
class Case:
    B: int
    T: int
    cin: int
    hidden: int
    seed: int = 0
    train: bool = True
    bias_offset: float = 0.0
    momentum: Optional[float] = 0.1

    @property
    def id(self) -> str:
        return f"b{self.B}_t{self.T}_c{self.cin}_h{self.hidden}" + ("" if self.train else "_eval") + (
            f"_off{self.bias_offset:g}" if self.bias_offset else "") + ("_cma" if self.momentum is None else "")


class TorchConvEncoder(nn.Module):
    """The reference's 'cnn' SequenceEncoder in plain torch.nn (dropout 0), keeping the BatchNorm
    outputs of the last forward (z1, z2: what the ReLUs see) for the kink precondition."""

    def __init__(self, cin: int, hidden: int, out: int):
        super().__init__()
        self.conv_net = nn.Sequential(
            nn.Conv1d(cin, hidden, kernel_size=3, padding=1), nn.BatchNorm1d(hidden), nn.ReLU(),
            nn.Conv1d(hidden, hidden, kernel_size=3, padding=1), nn.BatchNorm1d(hidden), nn.ReLU())
        self.pool = nn.AdaptiveAvgPool1d(1)
        self.projection = nn.Linear(hidden, out)

    def forward(self, sequence):
        x = sequence.transpose(1, 2)
        self.z1 = self.conv_net[1](self.conv_net[0](x))
        self.z2 = self.conv_net[4](self.conv_net[3](self.conv_net[2](self.z1)))
        x = self.pool(self.conv_net[5](self.z2)).squeeze(-1)
        return self.projection(x)


def make_case(case: Case):
    """(state dict, input (B, T, cin), output gradient (B, OUT_DIM)) of a case, float32 on the CPU:
    BatchNorm weights uniform(0.5, 1.5) and biases uniform(-0.5, 0.5) (relu(shift) != 0 at padded rows
    of a kernel that pads before the activation), random running statistics."""
    g = torch.Generator().manual_seed(1000 + case.seed)
    torch.manual_seed(case.seed)
    m = TorchConvEncoder(case.cin, case.hidden, OUT_DIM)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    for i in (1, 4):
        sd[f"conv_net.{i}.weight"] = torch.rand(case.hidden, generator=g) + 0.5
        sd[f"conv_net.{i}.bias"] = torch.rand(case.hidden, generator=g) - 0.5
        sd[f"conv_net.{i}.running_mean"] = 0.5 * torch.randn(case.hidden, generator=g) + case.bias_offset
        sd[f"conv_net.{i}.running_var"] = torch.rand(case.hidden, generator=g) + 0.5
        sd[f"conv_net.{i}.num_batches_tracked"] = torch.tensor(3)
    for k in BIAS_KEYS:
        sd[k] = sd[k] + case.bias_offset
    x = torch.randn(case.B, case.T, case.cin, generator=g)
    gout = torch.randn(case.B, OUT_DIM, generator=g)
    return sd, x, gout


def run_torch(case: Case, sd, x, gout, dtype) -> Dict[str, torch.Tensor]:
    """Forward + backward of sum(out * gout) in plain torch on the CPU -> {"out", "dx", "grad/<param>",
    "buf/<buffer>" (after the forward), "z1", "z2"}."""
    m = TorchConvEncoder(case.cin, case.hidden, OUT_DIM).to(dtype)
    m.load_state_dict(sd)
    for i in (1, 4):
        m.conv_net[i].momentum = case.momentum
    m.train(case.train)
    xin = x.detach().to(dtype).clone().requires_grad_(True)
    out = m(xin)
    (out * gout.to(dtype)).sum().backward()
    res = {"out": out.detach(), "dx": xin.grad, "z1": m.z1.detach(), "z2": m.z2.detach()}
    for k, p in m.named_parameters():
        res[f"grad/{k}"] = p.grad
    for k, b in m.named_buffers():
        res[f"buf/{k}"] = b.detach().clone()
    return res


def run_device(enc_mod, case: Case, sd, x, gout, need_dx: bool = True) -> Dict[str, torch.Tensor]:
    """The same through encoders.ConvSequenceEncoder on the GPU."""
    e = enc_mod.ConvSequenceEncoder(case.cin, case.hidden, OUT_DIM, dropout=0.0)
    e.load_state_dict(sd)
    for i in (1, 4):
        e.conv_net[i].momentum = case.momentum
    e = e.cuda().train(case.train)
    xin = x.detach().to("cuda").clone().requires_grad_(need_dx)
    out = e(xin)
    (out * gout.cuda()).sum().backward()
    torch.cuda.synchronize()
    res = {"out": out.detach().cpu(), "dx": xin.grad.cpu() if need_dx else None}
    for k, p in e.named_parameters():
        res[f"grad/{k}"] = p.grad.cpu()
    for k, b in e.named_buffers():
        res[f"buf/{k}"] = b.detach().cpu()
    return res


def compared_keys(case: Case, ref):
    return [k for k in ref if k == "out" or k == "dx" or k.startswith("grad/")]


def check_preconditions(case: Case, ref64, ref32) -> None:
    """The case is well posed: no BatchNorm output within 1e-5 (relative) of the ReLU kink in either
    layer, and fp32 torch on the CPU within 1e-4 of float64 on every compared tensor (the train-mode
    conv bias gradients, mathematically zero, excepted: they have a bound of their own)."""
    for z in ("z1", "z2"):
        a = ref64[z].abs()
        assert float(a.min()) >= 1e-5 * float(a.max()), (case.id, z, float(a.min()), float(a.max()))
    for k in compared_keys(case, ref64):
        if case.train and k[5:] in BIAS_KEYS:
            continue
        assert close(ref32[k], ref64[k], 1e-4), (case.id, k, diff_report(ref32[k], ref64[k], 1e-4))


def check_parity(case: Case, got, ref64, ref32, rtol: float = 1e-3) -> None:
    """close(got, float64, 1e-3) on the output, dx and every parameter gradient; the train-mode conv
    bias gradients within zero_grad_bound of zero."""
    scale = max(float(ref64[k].abs().max()) for k in compared_keys(case, ref64) if k.startswith("grad/"))
    for k in compared_keys(case, ref64):
        if got[k] is None:
            continue
        if case.train and k[5:] in BIAS_KEYS:
            bound = zero_grad_bound(ref32[k], scale, ZERO_GRAD_C)
            worst = float(got[k].double().abs().max())
            print(f"{case.id} {k}: device max {worst:.3e}, fp32 torch max {float(ref32[k].abs().max()):.3e}, "
                  f"bound {bound:.3e}")
            assert worst <= bound, (case.id, k, worst, bound)
            continue
        print(f"{case.id} {k}: {diff_report(got[k], ref64[k], rtol)}")
        assert close(got[k], ref64[k], rtol), (case.id, k, diff_report(got[k], ref64[k], rtol))


def check_buffers(case: Case, got, ref64, rtol: float = 1e-3) -> None:
    for i in (1, 4):
        for name in ("running_mean", "running_var"):
            k = f"buf/conv_net.{i}.{name}"
            assert close(got[k], ref64[k], rtol), (case.id, k, diff_report(got[k], ref64[k], rtol))
        k = f"buf/conv_net.{i}.num_batches_tracked"
        assert int(got[k]) == int(ref64[k]), (case.id, k)
