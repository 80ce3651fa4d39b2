"""Helpers of the TransformerSequenceEncoder tests: the reference's 'transformer' SequenceEncoder in plain
torch.nn (src/encoders.py:99-111, 177-206: the comparator, on the CPU in float64 or float32), the same
stack restated with explicit formulas and torch.matmul (the oracle: float64-capable, takes a dropout-mask
provider such as _philox.mask_provider, and gives a sample of length 0 the library's zeros instead of
torch's NaN), the parity cases and their preconditions."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Callable, Dict, Optional, Tuple

import torch
import torch.nn as nn

from _util import close, diff_report

OUT_DIM = 16
HEADS = 4
SITE_TR = 0x500   # + 4 * layer + {0 attention probabilities, 1 out_proj, 2 ffn, 3 linear2} (csrc/transformer.hip)


@dataclass(frozen=True)
class Case:
    B: int
    T: int
    cin: int
    hidden: int
    ffn: int = 2048
    layers: int = 1
    lengths: Optional[Tuple[int, ...]] = None
    seed: int = 0
    train: bool = True
    bias_offset: float = 0.0     # added to input_projection.bias: LayerNorm's variance at a large mean

    @property
    def id(self) -> str:
        return (f"b{self.B}_t{self.T}_c{self.cin}_h{self.hidden}_f{self.ffn}_l{self.layers}"
                + ("" if self.lengths is None else "_len" + "-".join(str(v) for v in self.lengths))
                + ("" if self.train else "_eval") + (f"_off{self.bias_offset:g}" if self.bias_offset else ""))


class TorchTransformerEncoder(nn.Module):
    """The reference's 'transformer' SequenceEncoder in plain torch.nn (any dim_feedforward)."""

    def __init__(self, cin: int, hidden: int, out: int, layers: int, ffn: int = 2048, dropout: float = 0.0):
        super().__init__()
        self.input_projection = nn.Linear(cin, hidden)
        layer = nn.TransformerEncoderLayer(d_model=hidden, nhead=4 if hidden % 4 == 0 else 1, dim_feedforward=ffn,
                                           dropout=dropout, batch_first=True)
        self.transformer = nn.TransformerEncoder(layer, num_layers=layers, enable_nested_tensor=False)
        self.projection = nn.Linear(hidden, out)

    def forward(self, sequence, lengths=None):
        B, T, _ = sequence.shape
        x = self.input_projection(sequence)
        if lengths is None:
            return self.projection(self.transformer(x).mean(dim=1))
        pad = torch.arange(T).unsqueeze(0).expand(B, -1) >= lengths.to(torch.long).unsqueeze(1)
        y = self.transformer(x, src_key_padding_mask=pad)
        valid = (~pad).unsqueeze(-1).to(y.dtype)
        return self.projection((y * valid).sum(dim=1) / valid.sum(dim=1).clamp_min(1.0))


def make_case(case: Case):
    """(state dict, input (B, T, cin), lengths or None, output gradient (B, OUT_DIM)) of a case, float32 on
    the CPU: torch's initialisation under the case's seed, the LayerNorm weights uniform(0.5, 1.5) and
    biases uniform(-0.5, 0.5) (at torch's 1 / 0 a wrong gamma or beta path goes unseen), in_proj / out_proj
    / linear biases uniform(-0.1, 0.1) (torch zeroes the attention's)."""
    g = torch.Generator().manual_seed(2000 + case.seed)
    torch.manual_seed(case.seed)
    m = TorchTransformerEncoder(case.cin, case.hidden, OUT_DIM, case.layers, case.ffn)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    for k in range(case.layers):
        for n in ("norm1", "norm2"):
            sd[f"transformer.layers.{k}.{n}.weight"] = torch.rand(case.hidden, generator=g) + 0.5
            sd[f"transformer.layers.{k}.{n}.bias"] = torch.rand(case.hidden, generator=g) - 0.5
        for n in ("self_attn.in_proj_bias", "self_attn.out_proj.bias"):
            key = f"transformer.layers.{k}.{n}"
            sd[key] = 0.2 * torch.rand(sd[key].shape, generator=g) - 0.1
    if case.bias_offset:
        # The offset is LayerNorm's test (z = x + a at a mean of 100), not the attention's: left alone, the
        # first layer's scores would be ~1e4 and fp32 torch itself 1e-4 .. 1e-3 from float64.  With the rows
        # of its in_proj summing to zero a constant offset over the channels cancels in Q, K and V.
        w = sd["transformer.layers.0.self_attn.in_proj_weight"]
        sd["transformer.layers.0.self_attn.in_proj_weight"] = w - w.mean(dim=1, keepdim=True)
    sd["input_projection.bias"] = sd["input_projection.bias"] + case.bias_offset
    x = torch.randn(case.B, case.T, case.cin, generator=g)
    gout = torch.randn(case.B, OUT_DIM, generator=g)
    lengths = None if case.lengths is None else torch.tensor(case.lengths, dtype=torch.int64)
    return sd, x, lengths, gout


def _collect(out, xin, named_params) -> Dict[str, torch.Tensor]:
    res = {"out": out.detach(), "dx": xin.grad}
    for k, p in named_params:
        res[f"grad/{k}"] = p.grad if p.grad is not None else torch.zeros_like(p)
    return res


def run_torch(case: Case, sd, x, lengths, gout, dtype) -> Dict[str, torch.Tensor]:
    """Forward + backward of sum(out * gout) through the real nn.TransformerEncoder on the CPU (dropout 0)
    -> {"out", "dx", "grad/<param>"}.  (Not for a case with a length of 0: torch gives NaN there.)"""
    m = TorchTransformerEncoder(case.cin, case.hidden, OUT_DIM, case.layers, case.ffn).to(dtype)
    m.load_state_dict(sd)
    m.train(case.train)
    xin = x.detach().to(dtype).clone().requires_grad_(True)
    out = m(xin, lengths)
    (out * gout.to(dtype)).sum().backward()
    return _collect(out, xin, m.named_parameters())


def _layer_norm(z, gamma, beta, eps):
    d = z - z.mean(dim=-1, keepdim=True)
    var = (d * d).mean(dim=-1, keepdim=True)
    return d / torch.sqrt(var + eps) * gamma + beta


def stack_forward(params: Dict[str, torch.Tensor], x, lengths, layers: int, p: float = 0.0,
                  mask_fn: Optional[Callable] = None, eps: float = 1e-5, taps: Optional[dict] = None):
    """The encoder in formulas: sequence (B, T, cin) -> out (B, OUT_DIM).  mask_fn(site, tensor) -> the keep
    mask of a dropout site (row-major element order), applied as tensor * keep / (1 - p); None: no dropout.
    taps (optional dict) receives linear1's pre-activation and its rounding scale |y1| |W1|^T + |b1| per
    layer ("pre/k", "scale/k": (B, T, ffn)) and the valid-step mask ("valid": (B, T) bool)."""
    def drop(site, t):
        if mask_fn is None or p <= 0.0:
            return t
        return t * mask_fn(site, t).to(t.dtype) / (1.0 - p)

    B, T, _ = x.shape
    x = torch.matmul(x, params["input_projection.weight"].t()) + params["input_projection.bias"]
    H = x.shape[-1]
    hd = H // HEADS
    valid = torch.ones(B, T, dtype=torch.bool) if lengths is None else \
        torch.arange(T).unsqueeze(0) < lengths.clamp(0, T).unsqueeze(1)
    if taps is not None:
        taps["valid"] = valid
    for k in range(layers):
        w = lambda n, k=k: params[f"transformer.layers.{k}.{n}"]   # noqa: E731
        site = SITE_TR + 4 * k
        qkv = torch.matmul(x, w("self_attn.in_proj_weight").t()) + w("self_attn.in_proj_bias")
        q, kk, v = (t.reshape(B, T, HEADS, hd).transpose(1, 2) for t in qkv.split(H, dim=-1))
        s = torch.matmul(q, kk.transpose(-1, -2)) / math.sqrt(hd)
        s = s.masked_fill(~valid[:, None, None, :], float("-inf"))
        smax = s.detach().amax(dim=-1, keepdim=True)
        smax = torch.where(torch.isfinite(smax), smax, torch.zeros_like(smax))
        e = torch.exp(s - smax)
        den = e.sum(dim=-1, keepdim=True)
        pr = e / torch.where(den > 0, den, torch.ones_like(den))     # a row with no valid key: zeros
        pr = drop(site + 0, pr)
        o = torch.matmul(pr, v).transpose(1, 2).reshape(B, T, H)
        a = drop(site + 1, torch.matmul(o, w("self_attn.out_proj.weight").t()) + w("self_attn.out_proj.bias"))
        y1 = _layer_norm(x + a, w("norm1.weight"), w("norm1.bias"), eps)
        pre = torch.matmul(y1, w("linear1.weight").t()) + w("linear1.bias")
        if taps is not None:
            taps[f"pre/{k}"] = pre.detach()
            taps[f"scale/{k}"] = (torch.matmul(y1.detach().abs(), w("linear1.weight").detach().abs().t())
                                  + w("linear1.bias").detach().abs())
        h = drop(site + 2, torch.relu(pre))
        f = drop(site + 3, torch.matmul(h, w("linear2.weight").t()) + w("linear2.bias"))
        x = _layer_norm(y1 + f, w("norm2.weight"), w("norm2.bias"), eps)
    vf = valid.unsqueeze(-1).to(x.dtype)
    pooled = (x * vf).sum(dim=1) / vf.sum(dim=1).clamp_min(1.0)
    return torch.matmul(pooled, params["projection.weight"].t()) + params["projection.bias"]


def run_oracle(case: Case, sd, x, lengths, gout, dtype, p: float = 0.0, mask_fn=None) -> Dict[str, torch.Tensor]:
    """Forward + backward of sum(out * gout) through stack_forward -> run_torch's keys plus the taps."""
    params = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    xin = x.detach().to(dtype).clone().requires_grad_(True)
    taps: dict = {}
    out = stack_forward(params, xin, lengths, case.layers, p=p if case.train else 0.0, mask_fn=mask_fn, taps=taps)
    (out * gout.to(dtype)).sum().backward()
    res = _collect(out, xin, params.items())
    res.update(taps)
    return res


def build_device(enc_mod, case: Case, sd, dropout: float = 0.0):
    """encoders.TransformerSequenceEncoder of the case on the GPU; a dim_feedforward other than torch's
    2048 is swapped in (the kernels take any)."""
    e = enc_mod.TransformerSequenceEncoder(case.cin, case.hidden, OUT_DIM, num_layers=case.layers, dropout=dropout)
    if case.ffn != 2048:
        layer = nn.TransformerEncoderLayer(d_model=case.hidden, nhead=4, dim_feedforward=case.ffn, dropout=dropout,
                                           batch_first=True)
        e.transformer = nn.TransformerEncoder(layer, num_layers=case.layers)
    e.load_state_dict(sd)
    return e.cuda().train(case.train)


def run_device(enc_mod, case: Case, sd, x, lengths, gout, need_dx: bool = True, dropout: float = 0.0,
               rng: Optional[Tuple[int, int]] = None) -> Dict[str, torch.Tensor]:
    """The same through encoders.TransformerSequenceEncoder on the GPU.  dropout: the layer stack's p (the
    module's final nn.Dropout, torch's own generator, is set to 0); rng: the module's Philox (seed, offset)."""
    e = build_device(enc_mod, case, sd, dropout)
    e.dropout_layer.p = 0.0
    if rng is not None:
        e._rng_state.copy_(torch.tensor(rng, dtype=torch.int64))
    xin = x.detach().to("cuda").clone().requires_grad_(need_dx)
    out = e(xin, None if lengths is None else lengths.cuda())
    (out * gout.cuda()).sum().backward()
    torch.cuda.synchronize()
    res = {"out": out.detach().cpu(), "dx": xin.grad.cpu() if need_dx else None}
    for k, p in e.named_parameters():
        res[f"grad/{k}"] = p.grad.cpu()
    return res


def compared_keys(ref):
    return [k for k in ref if k == "out" or k == "dx" or k.startswith("grad/")]


def check_preconditions(case: Case, ref64, ref32=None) -> None:
    """The case is well posed: no linear1 pre-activation of a valid token within 1e-6 (|y1| |W1|^T + |b1|)
    of the ReLU kink in float64 (ref64: run_oracle's result with its taps), and fp32 torch on the CPU
    within 1e-4 of float64 on every compared tensor (ref32: run_torch at float32; None where torch
    cannot run the case)."""
    valid = ref64["valid"]
    for k in range(case.layers):
        pre, scale = ref64[f"pre/{k}"][valid], ref64[f"scale/{k}"][valid]
        if pre.numel():
            margin = float((pre.abs() / scale).min())
            assert margin > 1e-6, (case.id, f"linear1 pre-activation of layer {k} in the kink band", margin)
    if ref32 is not None:
        for k in compared_keys(ref64):
            assert close(ref32[k], ref64[k], 1e-4), (case.id, k, diff_report(ref32[k], ref64[k], 1e-4))


def check_parity(case: Case, got, ref64, rtol: float = 1e-3) -> None:
    """close(got, float64, 1e-3) on the output, dx and every parameter gradient."""
    for k in compared_keys(ref64):
        if got[k] is None:
            continue
        print(f"{case.id} {k}: {diff_report(got[k], ref64[k], rtol)}")
        assert close(got[k], ref64[k], rtol), (case.id, k, diff_report(got[k], ref64[k], rtol))
