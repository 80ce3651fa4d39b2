"""Helpers of the TransformerSequenceEncoder tests: the reference's 'transformer' SequenceEncoder in plain
torch.nn (src/encoders.py:99-111, 177-206: the comparator, on the CPU in float64 or float32), the same
stack restated with explicit formulas and torch.matmul (the oracle: float64-capable, takes a dropout-mask
provider such as _philox.mask_provider, and gives a sample of length 0 the library's zeros instead of
torch's NaN), the parity cases and their preconditions, and the launch-envelope rule (the saved layout
restated, a device run that keeps the saved tensors, the device's ReLU gates, the per-token comparison)."""
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
                  mask_fn: Optional[Callable] = None, eps: float = 1e-5, taps: Optional[dict] = None,
                  relu_gate: Optional[dict] = None, hooks: Optional[dict] = None, live: Optional[dict] = None):
    """The encoder in formulas: sequence (B, T, cin) -> out (B, OUT_DIM).  mask_fn(site, tensor) -> the keep
    mask of a dropout site (row-major element order), applied as tensor * keep / (1 - p); None: no dropout.
    taps (optional dict) receives linear1's pre-activation and its rounding scale |y1| |W1|^T + |b1| per
    layer ("pre/k", "scale/k": (B, T, ffn)), the valid-step mask ("valid": (B, T) bool) and, detached and
    under the names of csrc/transformer.hip's TrLayerSaved, what the device saves per layer: "qkv/k"
    (B, T, 3H), "o/k" (B, T, H), "lse/k" (B, 4, T: row max + log of the row sum, -inf for a row with no valid
    key), "z1/k", "st1/k" (B, T, 2: mean, 1 / sqrt(var + eps)), "y1/k", "h/k" (after ReLU and dropout),
    "z2/k", "st2/k", "y2/k".
    relu_gate {layer: (sel, pos)} (both (B, T, ffn) bool): where sel is set h = pre * pos replaces relu(pre)
    (device_gates: the device's decision within rounding of the kink); elsewhere the oracle keeps its sign.
    hooks (tests/test_transformer_envelope_bite.py plants defects through them; none: the oracle as it is):
    "scores"(k, s) -> s before the softmax; "y1"(k, y1) -> y1; "layer_norm"(z, gamma, beta, eps) in place of
    _layer_norm; "drop_bwd"(site, t, keep) -> the factor the backward of that dropout site applies instead of
    keep / (1 - p), or None.  live (optional dict) receives, attached and with their gradients retained, the
    out_proj output before its dropout ("a/k") and the layer output ("y2/k")."""
    hooks = hooks or {}

    def drop(site, t):
        if mask_fn is None or p <= 0.0:
            return t
        keep = mask_fn(site, t).to(t.dtype)
        alt = hooks["drop_bwd"](site, t, keep) if "drop_bwd" in hooks else None
        if alt is None:
            return t * keep / (1.0 - p)
        planted = t * alt                                          # the honest value bit for bit, `alt` in the backward
        return (t * keep / (1.0 - p)).detach() + (planted - planted.detach())

    layer_norm = hooks.get("layer_norm", _layer_norm)

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
        if "scores" in hooks:
            s = hooks["scores"](k, s)
        smax = s.detach().amax(dim=-1, keepdim=True)
        smax = torch.where(torch.isfinite(smax), smax, torch.zeros_like(smax))
        e = torch.exp(s - smax)
        den = e.sum(dim=-1, keepdim=True)
        pr = e / torch.where(den > 0, den, torch.ones_like(den))     # a row with no valid key: zeros
        pr = drop(site + 0, pr)
        o = torch.matmul(pr, v).transpose(1, 2).reshape(B, T, H)
        a_pre = torch.matmul(o, w("self_attn.out_proj.weight").t()) + w("self_attn.out_proj.bias")
        if live is not None:
            a_pre.retain_grad()
            live[f"a/{k}"] = a_pre
        z1 = x + drop(site + 1, a_pre)
        y1 = layer_norm(z1, w("norm1.weight"), w("norm1.bias"), eps)
        if "y1" in hooks:
            y1 = hooks["y1"](k, y1)
        pre = torch.matmul(y1, w("linear1.weight").t()) + w("linear1.bias")
        if taps is not None:
            taps[f"pre/{k}"] = pre.detach()
            taps[f"scale/{k}"] = (torch.matmul(y1.detach().abs(), w("linear1.weight").detach().abs().t())
                                  + w("linear1.bias").detach().abs())
        act = torch.relu(pre)
        if relu_gate is not None and k in relu_gate:
            sel, pos = relu_gate[k]
            act = torch.where(sel, pre * pos.to(pre.dtype), act)
        h = drop(site + 2, act)
        z2 = y1 + drop(site + 3, torch.matmul(h, w("linear2.weight").t()) + w("linear2.bias"))
        y2 = layer_norm(z2, w("norm2.weight"), w("norm2.bias"), eps)
        if live is not None:
            y2.retain_grad()
            live[f"y2/{k}"] = y2
        if taps is not None:
            def stat(z):
                d = z.detach() - z.detach().mean(dim=-1, keepdim=True)
                return torch.cat([z.detach().mean(dim=-1, keepdim=True),
                                  1.0 / torch.sqrt((d * d).mean(dim=-1, keepdim=True) + eps)], dim=-1)
            lse = torch.where(den > 0, smax + torch.log(torch.where(den > 0, den, torch.ones_like(den))),
                              torch.full_like(den, float("-inf")))
            for name, t in (("qkv", qkv), ("o", o), ("lse", lse.squeeze(-1)), ("z1", z1), ("st1", stat(z1)), ("y1", y1),
                            ("h", h), ("z2", z2), ("st2", stat(z2)), ("y2", y2)):
                taps[f"{name}/{k}"] = t.detach()
        x = y2
    vf = valid.unsqueeze(-1).to(x.dtype)
    pooled = (x * vf).sum(dim=1) / vf.sum(dim=1).clamp_min(1.0)
    return torch.matmul(pooled, params["projection.weight"].t()) + params["projection.bias"]


def run_oracle(case: Case, sd, x, lengths, gout, dtype, p: float = 0.0, mask_fn=None, relu_gate=None, hooks=None,
               live=None) -> Dict[str, torch.Tensor]:
    """Forward + backward of sum(out * gout) through stack_forward -> run_torch's keys plus the taps."""
    params = {k: v.detach().to(dtype).clone().requires_grad_(True) for k, v in sd.items()}
    xin = x.detach().to(dtype).clone().requires_grad_(True)
    taps: dict = {}
    out = stack_forward(params, xin, lengths, case.layers, p=p if case.train else 0.0, mask_fn=mask_fn, taps=taps,
                        relu_gate=relu_gate, hooks=hooks, live=live)
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


# ------------------------------------------------------------------------------------------------------
# The launch envelope: tests/test_gpu_transformer_envelope.py and tests/test_transformer_envelope_bite.py
SAVED_NAMES = ("qkv", "o", "lse", "z1", "st1", "y1", "h", "z2", "st2", "y2")   # TrLayerSaved's order
LAYER_PARAMS = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight",
                "self_attn.out_proj.bias", "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias",
                "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias")   # the order of the ops' params
GATE_REL = 1e-5        # the kink band |pre| <= 1e-5 (|y1| |W1|^T + |b1|): _util.device_relu_gates' constant
SLICE_FLOOR = 1e-6     # every compared slice's maximum is at least this much of its tensor's
ORACLE_CAP = 2.5e-5    # the fp32 oracle's own worst slice error: a quarter of the comparison's cap


def saved_layout(B: int, T: int, H: int, F: int, layers: int):
    """csrc/transformer.hip's tr_saved() restated: ({"<name>/<layer>": (byte offset, shape)}, end offset).
    Every take is rounded up to 256 bytes; the rng snapshot (two uint64) comes first, then the ten fp32
    buffers per layer in TrLayerSaved's order."""
    shapes = {"qkv": (B, T, 3 * H), "o": (B, T, H), "lse": (B, HEADS, T), "z1": (B, T, H), "st1": (B, T, 2),
              "y1": (B, T, H), "h": (B, T, F), "z2": (B, T, H), "st2": (B, T, 2), "y2": (B, T, H)}
    lay, off = {}, 0

    def take(nbytes):
        nonlocal off
        off = (off + 255) & ~255
        at = off
        off += nbytes
        return at

    take(16)
    for k in range(layers):
        for name in SAVED_NAMES:
            lay[f"{name}/{k}"] = (take(4 * math.prod(shapes[name])), shapes[name])
    return lay, off


def saved_views(saved: torch.Tensor, B: int, T: int, H: int, F: int, layers: int):
    """float32 views by name of the bytes torch.ops.mmfusion.transformer_encoder_fwd returns (on the host).
    The restated layout is tied to the library's: its end + 256 must be
    mmf_transformer_encoder_saved_bytes(B, T, H, F, layers), and `saved` must hold at least that."""
    import mmf_native
    saved_bytes = mmf_native.lib().mmf_transformer_encoder_saved_bytes(B, T, H, F, layers)
    lay, end = saved_layout(B, T, H, F, layers)
    assert end + 256 == saved_bytes, (end + 256, saved_bytes, "the saved layout restated here is not the library's")
    assert saved.dtype == torch.uint8 and saved.numel() >= saved_bytes, (saved.dtype, saved.numel(), saved_bytes)
    host = saved.detach().cpu()
    return {key: host[at:at + 4 * math.prod(shape)].view(torch.float32).reshape(shape).clone()
            for key, (at, shape) in lay.items()}


def device_gates(case: Case, sd, x, lengths, h_dev: Dict[int, torch.Tensor], p: float = 0.0, mask_fn=None,
                 tag: str = ""):
    """The device's ReLU decisions for the linear1 pre-activations within rounding of zero, for
    stack_forward(relu_gate=...).  h_dev: layer -> the saved Drop(ReLU(linear1)) (B, T, ffn), whose sign the
    backward's gate reads.  Layer by layer in float64 (a layer's pre-activations depend on the gates of the
    layers before it): sel = |pre| <= 1e-5 (|y1| |W1|^T + |b1|), pos = h_dev > 0.  Asserted on the valid
    tokens: outside the band every element the device passed has pre > 0, and every kept element with pre > 0
    was passed -- a kernel that gets a clear sign wrong fails here.  -> (gates, {layer: elements in the band})."""
    params = {k: v.detach().double() for k, v in sd.items()}
    gates, counts = {}, {}
    for k in range(case.layers):
        taps: dict = {}
        with torch.no_grad():
            stack_forward(params, x.detach().double(), lengths, k + 1, p=p, mask_fn=mask_fn, taps=taps, relu_gate=gates)
        pre, scale, valid = taps[f"pre/{k}"], taps[f"scale/{k}"], taps["valid"].unsqueeze(-1)
        sel = pre.abs() <= GATE_REL * scale
        pos = h_dev[k].detach().cpu().reshape(pre.shape) > 0
        keep = torch.ones_like(sel) if mask_fn is None or p <= 0.0 else mask_fn(SITE_TR + 4 * k + 2, pre).bool()
        bad = valid & pos & ~sel & ~(pre > 0)
        assert not bool(bad.any()), (tag, k, int(bad.sum()), "the device passed a pre-activation float64 puts clearly <= 0")
        miss = valid & keep & ~sel & (pre > 0) & ~pos
        assert not bool(miss.any()), (tag, k, int(miss.sum()), "the device blocked a pre-activation float64 puts clearly > 0")
        gates[k] = (sel, pos)
        counts[k] = int((sel & valid).sum())
    print(f"{tag} linear1 pre-activations of valid tokens in the kink band, per layer: {counts}")
    return gates, counts


def gated_references(case: Case, sd, x, lengths, gout, h_dev, p, mask_fn, tag=""):
    """(float64 oracle, float32 oracle, band counts), both oracles under the masks and the device's gates."""
    gates, counts = device_gates(case, sd, x, lengths, h_dev, p, mask_fn, tag)
    r64 = run_oracle(case, sd, x, lengths, gout, torch.float64, p=p, mask_fn=mask_fn, relu_gate=gates)
    r32 = run_oracle(case, sd, x, lengths, gout, torch.float32, p=p, mask_fn=mask_fn, relu_gate=gates)
    return r64, r32, counts


def _k_third(t: torch.Tensor):
    H = t.shape[0] // 3
    return t[H:2 * H]


def envelope_slices(res: Dict[str, torch.Tensor], valid: torch.Tensor, layers: int):
    """{key: (tensor with the slices along dim 0, or whole, slice_dim)} of what the envelope rule compares:
    every saved forward tensor one slice per valid token ((B, T, X) -> the rows t < len_b of (B T, X); lse one
    slice per (sample, head) over the valid queries), out one slice per sample, dx one slice per valid token,
    every parameter gradient one slice -- in_proj_bias without its K third (mathematically zero, on its own
    in compare_envelope)."""
    rows = valid.reshape(-1)
    out = {}
    for k in range(layers):
        for name in SAVED_NAMES:
            t = res[f"{name}/{k}"]
            if name == "lse":
                out[f"lse/{k}"] = (torch.where(valid[:, None, :], t, torch.zeros_like(t)).reshape(-1, t.shape[-1]), 0)
            else:
                out[f"{name}/{k}"] = (t.reshape(rows.numel(), -1)[rows], 0)
    out["out"] = (res["out"], 0)
    out["dx"] = (res["dx"].reshape(rows.numel(), -1)[rows], 0)
    for key in res:
        if not key.startswith("grad/"):
            continue
        t = res[key]
        if key.endswith("in_proj_bias"):
            H = t.shape[0] // 3
            t = torch.cat([t[:H], t[2 * H:]])
        out[key] = (t, None)
    return out


def check_conditions(ref64, ref32, layers: int, tag: str = ""):
    """The CPU-side conditions of the envelope rule, from the oracles alone: every compared slice's maximum is
    at least 1e-6 of its tensor's (exactly zero slices excepted), and the fp32 oracle's own worst slice error
    is at most 2.5e-5.  -> (worst fp32 slice error, smallest slice maximum / tensor maximum)."""
    from _util import sliced_errors
    valid = ref64["valid"]
    s64, s32 = envelope_slices(ref64, valid, layers), envelope_slices(ref32, valid, layers)
    worst, floor = 0.0, 1.0
    for key, (t64, sdim) in s64.items():
        _, e32 = sliced_errors(s32[key][0], t64, s32[key][0], sdim)
        worst = max(worst, float(e32.max()))
        assert float(e32.max()) <= ORACLE_CAP, (tag, key, float(e32.max()), "the fp32 oracle itself nears the cap")
        if sdim is not None:
            m = t64.double().abs().reshape(t64.shape[0], -1).amax(dim=1)
            m = m[m > 0] / float(m.max())
            floor = min(floor, float(m.min()))
            assert float(m.min()) >= SLICE_FLOOR, (tag, key, float(m.min()), "a slice far below its tensor's maximum")
    print(f"{tag} conditions: fp32 oracle worst slice error {worst:.3e} (<= {ORACLE_CAP:g}), smallest slice maximum "
          f"{floor:.3e} of its tensor's (>= {SLICE_FLOOR:g})")
    return worst, floor


def compare_envelope(got, ref64, ref32, layers: int, tag: str, c: float, cap: float):
    """The envelope rule: _util.close_sliced(got, float64, fp32 oracle, c, cap) on envelope_slices, every padded
    dx row exactly 0.0, the K third of every in_proj_bias gradient under _util.zero_grad_bound.
    -> (violations, largest e_dev / max(e_32, 2^-24), largest e_dev); prints one line per tensor."""
    from _util import EPS32, close_sliced, sliced_ratio, sliced_report, zero_grad_bound
    valid = ref64["valid"]
    sg, s64, s32 = (envelope_slices(r, valid, layers) for r in (got, ref64, ref32))
    bad, worst, worst_e = [], 0.0, 0.0
    for key, (t64, sdim) in s64.items():
        g, t32 = sg[key][0], s32[key][0]
        ratio, e_dev = sliced_ratio(g, t64, t32, slice_dim=sdim)
        print(f"{tag} {key}: ratio {ratio:.2f}, e_dev {e_dev:.3e}")
        worst, worst_e = max(worst, ratio), max(worst_e, e_dev)
        if not close_sliced(g, t64, t32, slice_dim=sdim, c=c, cap=cap):
            bad.append(f"{key}: " + sliced_report(g, t64, t32, slice_dim=sdim, c=c, cap=cap))
    pad = got["dx"][~valid]
    if pad.numel() and not float(pad.abs().max()) == 0.0:
        bad.append(f"dx: a padded row is not exactly 0.0 (max {float(pad.abs().max()):.3e})")
    scale = max(float(ref64[k].abs().max()) for k in ref64 if k.startswith("grad/"))
    for key in ref64:
        if key.endswith("in_proj_bias"):
            g, own = float(_k_third(got[key]).abs().max()), float(_k_third(ref32[key]).abs().max())
            bound = zero_grad_bound(_k_third(ref32[key]), scale, c)
            print(f"{tag} {key}[K third]: max|got| {g:.3e}, fp32 oracle {own:.3e}, 2^-24 S {EPS32 * scale:.3e}, "
                  f"ratio {g / max(own, EPS32 * scale):.2f}")
            if not g <= bound:
                bad.append(f"{key}[K third]: max|got| {g:.3e} > {bound:.3e}")
    print(f"{tag} worst ratio {worst:.2f}, largest e_dev {worst_e:.3e}")
    return bad, worst, worst_e


def old_rule(got, ref, rtol: float = 1e-3) -> bool:
    """What tests/test_gpu_transformer_encoder.py looks at: close(., 1e-3) on out, dx and the gradients."""
    return all(close(got[k], ref[k], rtol) for k in compared_keys(ref))


def run_device_saved(enc_mod, nat, case: Case, sd, x, lengths, gout, dropout: float = 0.0,
                     rng: Optional[Tuple[int, int]] = None):
    """run_device's computation with the layer stack called directly -- input_projection, then
    torch.ops.mmfusion.transformer_encoder_fwd / _bwd, then projection -- under the library's launch profile:
    (run_device's keys plus the saved views "<name>/<layer>", the launch records)."""
    e = build_device(enc_mod, case, sd, dropout)
    if rng is not None:
        e._rng_state.copy_(torch.tensor(rng, dtype=torch.int64))
    layers, p, eps = e._stack()
    params = [q for lyr in layers for q in
              (lyr.self_attn.in_proj_weight, lyr.self_attn.in_proj_bias, lyr.self_attn.out_proj.weight,
               lyr.self_attn.out_proj.bias, lyr.linear1.weight, lyr.linear1.bias, lyr.linear2.weight, lyr.linear2.bias,
               lyr.norm1.weight, lyr.norm1.bias, lyr.norm2.weight, lyr.norm2.bias)]
    lens = None if lengths is None else lengths.to(device="cuda", dtype=torch.int64).contiguous()
    xin = x.detach().to("cuda").clone().requires_grad_(True)
    B, T, H, F = case.B, case.T, case.hidden, case.ffn
    nat.profile_begin()
    try:
        xp = nat.f32c(e.input_projection(nat.f32c(xin)))
        with torch.no_grad():
            pooled, saved, _ = torch.ops.mmfusion.transformer_encoder_fwd(
                xp.detach(), lens, e._rng_state, [q.detach() for q in params], bool(e.transformer.training), float(p),
                float(eps))
        pooled = pooled.requires_grad_(True)
        out = e.projection(pooled)
        (out * gout.cuda()).sum().backward()
        with torch.no_grad():
            dxp, *grads = torch.ops.mmfusion.transformer_encoder_bwd(
                xp.detach(), lens, [q.detach() for q in params], saved, pooled.grad.contiguous(),
                bool(e.transformer.training), float(p), float(eps), True)
        xp.backward(dxp)
        torch.cuda.synchronize()
    finally:
        _, launches = nat.profile_end()
    res = {"out": out.detach().cpu(), "dx": xin.grad.cpu()}
    for name in ("input_projection", "projection"):
        for leaf in ("weight", "bias"):
            res[f"grad/{name}.{leaf}"] = getattr(getattr(e, name), leaf).grad.cpu()
    for i, g in enumerate(grads):
        res[f"grad/transformer.layers.{i // len(LAYER_PARAMS)}.{LAYER_PARAMS[i % len(LAYER_PARAMS)]}"] = g.cpu()
    res.update(saved_views(saved, B, T, H, F, case.layers))
    return res, launches


# ---- the envelope cases and their restated launch arithmetic
C, CAP = 64.0, 1e-4
P_DROP, RNG = 0.1, (0x2468ACE01357, 3)


def _case(B, T, H, F, layers, lengths, seed=0):
    return Case(B, T, 8, H, ffn=F, layers=layers, lengths=lengths, seed=seed)


ENVELOPE_CASES = {
    "tr_long_64slabs": _case(2, 1020, 256, 2048, 2, (1020, 515)),
    "tr_default_ffn": _case(3, 37, 64, 2048, 1, (37, 20, 1)),
    "tr_ragged_h252": _case(3, 47, 252, 100, 1, (47, 46, 3)),
    "tr_h4": _case(3, 9, 4, 8, 1, (9, 5, 1)),
    "tr_h12": _case(2, 70, 12, 24, 1, (70, 33)),
    "tr_h48": _case(2, 70, 48, 64, 1, (70, 33)),
    "tr_generic_rows": _case(2, 70, 20, 30, 1, (70, 33)),
    "tr_scalar_epi_wide": _case(2, 70, 256, 2046, 1, (70, 33)),
    "tr_ffn_max": _case(2, 33, 64, 8192, 1, (33, 17)),
    "tr_chunk_edges": _case(5, 130, 64, 32, 1, (130, 129, 128, 64, 1)),
}
# In the cases above the shortest sample comes last, so the trailing rows of the (B T) row space are padding:
# the ragged last slab, LayerNorm chunk, reduce group and forward workgroup hold rows whose gradient is exactly
# zero and whose saved rows are not compared.  The *_tail cases are the same shapes with the lengths reversed,
# so that those tails hold valid tokens (tail_rows).
for _name in ("tr_long_64slabs", "tr_default_ffn", "tr_ragged_h252", "tr_h12", "tr_scalar_epi_wide", "tr_ffn_max",
              "tr_chunk_edges"):
    _c = ENVELOPE_CASES[_name]
    ENVELOPE_CASES[_name + "_tail"] = Case(_c.B, _c.T, _c.cin, _c.hidden, ffn=_c.ffn, layers=_c.layers,
                                           lengths=tuple(reversed(_c.lengths)), seed=_c.seed)

# ---- csrc/transformer.hip (wgrad_hint, ln_chunks, ln_group), csrc/capi_util.h (split_rows) and
# ---- csrc/gemm.hip (job_fast, job_small_slab) restated
LDS = "gemm_lds_kernel<{}, {}, 16, 3, 0>"     # fp32 MFMA at every matmul precision: the last argument is 0
GEN = "gemm_generic_kernel<{}, {}>"
LN_ROWS = 32


def wgrad_hint(M, N):
    return max(1, min(1024 // (-(-M // 128) * -(-N // 128)), 64))


def split_rows(rows, hint):
    kchunk = (-(-rows // hint) + 31) & ~31
    return -(-rows // kchunk), kchunk


def wgrad_plan(case):
    """One layer's weight gradients in plan order:
    [(label, M, N, hint, nsplit, kchunk, last slab's rows, kernel)].  Every operand is a 256-byte aligned
    (n, M) / (n, N) buffer, so the KR x KR job is on the LDS-DMA kernel when n, M and N are multiples of 4;
    otherwise on small_slab_kernel when nsplit M (N + 1) <= 2^20 (kchunk <= 256), else on the generic kernel."""
    n, H, F = case.B * case.T, case.hidden, case.ffn
    out = []
    for label, M, N in (("linear2", H, F), ("linear1", F, H), ("out_proj", H, H), ("in_proj", 3 * H, H)):
        hint = wgrad_hint(M, N)
        nsplit, kchunk = split_rows(n, hint)
        if n % 4 == 0 and M % 4 == 0 and N % 4 == 0:
            kern = LDS.format(1, 1)
        elif nsplit * M * (N + 1) <= (1 << 20) and kchunk <= 256:
            kern = "small_slab_kernel"
        else:
            kern = GEN.format(1, 1)
        out.append((label, M, N, hint, nsplit, kchunk, n - (nsplit - 1) * kchunk, kern))
    return out


def ln_plan(case):
    """(chunks, rows of the last chunk, chunks per group, groups, chunks of the last group, column blocks)."""
    n = case.B * case.T
    chunks = -(-n // LN_ROWS)
    group = 1
    while group * group < chunks:
        group += 1
    ngroup = -(-chunks // group)
    return chunks, n - (chunks - 1) * LN_ROWS, group, ngroup, chunks - (ngroup - 1) * group, -(-2 * case.hidden // 256)


def tail_rows(case):
    """How many rows of each ragged tail of the (B T) row space hold a valid token, as (valid, rows):
    {"slab/<weight gradient>": its last split-K slab, "ln_chunk": the last add_layernorm_bwd chunk, "ln_group":
    the last first-level reduce group, "ln_fwd": the last add_layernorm_fwd workgroup}."""
    n = case.B * case.T
    valid = (torch.arange(case.T).unsqueeze(0) < torch.tensor(case.lengths).unsqueeze(1)).reshape(-1)

    def tail(rows):
        return int(valid[n - rows:].sum()), rows
    out = {f"slab/{j[0]}": tail(j[6]) for j in wgrad_plan(case)}
    chunks, last, group, ngroup, _, _ = ln_plan(case)
    out["ln_chunk"] = tail(last)
    out["ln_group"] = tail(n - (ngroup - 1) * group * LN_ROWS)
    out["ln_fwd"] = tail((n - 1) % 4 + 1)
    return out

