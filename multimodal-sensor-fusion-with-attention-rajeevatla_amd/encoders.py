"""FrameEncoder with its attention pooling on the HIP path.

Mirrors src/encoders.py::FrameEncoder (:210-336) of the reference: the same
constructor (frame_dim, hidden_dim=256, output_dim=128,
temporal_pooling="attention", dropout=0.1), attributes and state_dict keys
(frame_processor.0.*, attention.*, projection.0.*, projection.3.*), the same
forward(frames, mask=None) and the same errors:

  * ValueError("Unknown pooling: ...") at construction (:246-247);
  * ValueError("Expected 3D frame tensor, got shape ...") (:275-278);
  * ValueError("Unknown pooling strategy: ...") at run time (:306-309);
  * RuntimeError("Attention layer not initialized.") from attention_pool (:330-331).

attention_pool (:313-336) -- scores = attention(frames), -inf where mask == 0,
softmax over frames, nan_to_num, weighted sum -- runs forward and backward as
the HIP kernels behind mmf_attention_pool_forward / _backward
(csrc/softmax_pool.hip).  The frame MLP and the projection are nn.Linear
layers on PyTorch-ROCm (encoders are outside the fused path), and the
'average' / 'max' pooling branches stay plain torch (:288-305).  
SequenceEncoder (src/encoders.py:34-166) mirrors the
reference's 'lstm' branch: the same constructor, parameter names
(rnn.weight_ih_l{k}, rnn.weight_hh_l{k}, rnn.bias_*, projection.*), forward
(sequence, lengths=None) and errors.  The recurrence runs as one persistent
HIP launch per layer (csrc/lstm.hip, mmf_lstm_forward / _backward); the
time-parallel input projection and weight gradients are rocBLAS GEMMs.
``encode_sequences`` batches the LSTMs of several modalities into the same
launches.  The recurrence's workgroups wait on each other: the library refuses
a grid that cannot be co-resident, every launch gets a fresh timeout word, and
a wait that gives up poisons its outputs with NaN; ``lstm_timed_out()`` /
``check_lstm_timeouts()`` report such launches (one stream sync per check).  SequenceEncoder(...,
encoder_type="transformer") itself raises NotImplementedError; TransformerSequenceEncoder (below)
serves that type.

GRUSequenceEncoder mirrors the reference's 'gru' branch (src/encoders.py:77-85, 135-166): the same
attributes, construction order and state_dict keys (rnn.*, projection.*), the same forward(sequence,
lengths=None) and errors.  ``GRU`` is nn.GRU's parameter layout without being an nn.RNNBase, and
``gru_layers`` runs every layer of several GRUs in one persistent launch (csrc/gru.hip,
mmf_gru_forward / _backward: the LSTM's plan and inter-workgroup exchange, csrc/recurrence.h, with
the GRU cell -- three gate rows, n depending on r inside the step, b_hn kept out of the input
projection, a backward whose carry is d z + W_hh^T [dr, dz, dn r]).  The recurrence is fp32 FMA at
every torch.get_float32_matmul_precision() setting, as the LSTM's.  GRU launches share the LSTM's
timeout reporting.  SequenceEncoder(..., encoder_type="gru") itself still raises
NotImplementedError, naming GRUSequenceEncoder; ``build_encoder`` returns the right class, and
``encode_sequences`` batches the encoders of each recurrence kind into shared launches.

ConvSequenceEncoder mirrors the reference's 'cnn' branch (src/encoders.py:87-97, 168-175:
Conv1d(k=3, pad=1) -> BatchNorm1d -> ReLU, twice, -> AdaptiveAvgPool1d(1) -> dropout -> Linear),
with the reference's state_dict keys (conv_net.{0,1,3,4}.*, projection.*) and initialisation.
``conv_net`` holds the parameters and buffers; the conv stack up to the pooled (B, hidden)
vector runs forward and backward as the HIP kernels behind mmf_conv_encoder_forward / _backward
(csrc/conv_encoder.hip: channels-last implicit GEMMs on the fp32 matrix cores, BatchNorm-1
applied while conv 2's input tile is staged, batch statistics from centred values, fixed-order
reductions, no inter-workgroup waits).  The matmuls are fp32 MFMA at every
torch.get_float32_matmul_precision() setting (more precise than "high" / "medium" ask for).
SequenceEncoder(..., encoder_type="cnn") itself still raises NotImplementedError, naming
ConvSequenceEncoder; ``build_encoder`` (the reference's factory, src/encoders.py:400-451) returns
the right class for a modality and its config.

TransformerSequenceEncoder mirrors the reference's 'transformer' branch (src/encoders.py:99-111,
177-206: input_projection -> post-norm nn.TransformerEncoder (4 heads, ReLU, dim_feedforward 2048)
with the key padding mask t >= lengths[b] -> mean over the valid steps -> dropout -> Linear), with
the reference's state_dict keys and initialisation.  ``transformer`` holds the parameters; the
layer stack and the pool run forward and backward behind mmf_transformer_encoder_forward /
_backward (csrc/transformer.hip: the library's fp32 MFMA GEMMs and flash attention chained through
residual + LayerNorm, masked-mean-pool and their backward kernels; statistics from centred values,
in-kernel Philox dropout at four sites per layer, fixed-order reductions, no inter-workgroup
waits).  input_projection, the final dropout and projection stay nn.Linear / nn.Dropout.  A sample
of length 0 gets a zero pooled vector and zero gradients (the reference returns NaN there).
SequenceEncoder(..., encoder_type="transformer") itself still raises NotImplementedError, naming
TransformerSequenceEncoder; ``build_encoder`` returns it for that type.
"""

from __future__ import annotations

import os
import sys
from typing import Any, Dict, List, Optional, Sequence, cast

import torch
import torch.nn as nn

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import mmf_native as _nat  # noqa: E402
import mmf_ops as _ops  # noqa: E402


def attention_pool(frames: torch.Tensor, attention: nn.Linear, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Learned-score softmax pooling over the frame axis (src/encoders.py:313-336) on HIP."""
    _nat.require_device(frames, "FrameEncoder input")
    frames = _nat.f32c(frames)
    m = None
    if mask is not None:
        m = mask.to(device=frames.device, dtype=torch.float32).contiguous()
        if m.shape != frames.shape[:2]:
            raise ValueError(f"mask shape {tuple(m.shape)} does not match frames {tuple(frames.shape[:2])}")
    pooled, _ = torch.ops.mmfusion.attention_pool_fwd(frames, attention.weight, attention.bias, m)
    return pooled


class FrameEncoder(nn.Module):
    """Frame-level features -> video-level embedding (src/encoders.py:210-310)."""

    temporal_pooling: str
    attention: Optional[nn.Linear]

    def __init__(self, frame_dim: int, hidden_dim: int = 256, output_dim: int = 128,
                 temporal_pooling: str = "attention", dropout: float = 0.1):
        super().__init__()
        cast_self = cast(Any, self)
        cast_self.temporal_pooling = temporal_pooling
        self.frame_processor = nn.Sequential(nn.Linear(frame_dim, hidden_dim), nn.ReLU(), nn.Dropout(dropout))
        cast_self.attention = None
        if temporal_pooling == "attention":
            cast_self.attention = nn.Linear(hidden_dim, 1)
        elif temporal_pooling not in ("average", "max"):
            raise ValueError(f"Unknown pooling: {temporal_pooling}")
        self.projection = nn.Sequential(nn.Linear(hidden_dim, hidden_dim), nn.ReLU(), nn.Dropout(dropout),
                                        nn.Linear(hidden_dim, output_dim))

    def forward(self, frames: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        if frames.dim() != 3:
            raise ValueError(f"Expected 3D frame tensor, got shape {frames.shape}")
        processed = self.frame_processor(frames)
        if mask is not None:
            mask = mask.to(device=processed.device, dtype=processed.dtype)
        if self.temporal_pooling == "attention":
            pooled = self.attention_pool(processed, mask)
        elif self.temporal_pooling == "average":
            if mask is None:
                pooled = processed.mean(dim=1)
            else:
                wts = mask.unsqueeze(-1)
                pooled = (processed * wts).sum(dim=1) / wts.sum(dim=1).clamp_min(1e-8)
        elif self.temporal_pooling == "max":
            if mask is None:
                pooled = processed.max(dim=1).values
            else:
                pooled = processed.masked_fill(mask.unsqueeze(-1) == 0, float("-inf")).max(dim=1).values
                pooled = torch.nan_to_num(pooled, nan=0.0, neginf=0.0)
        else:
            raise ValueError(f"Unknown pooling strategy: {self.temporal_pooling}")
        return self.projection(pooled)

    def attention_pool(self, frames: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
        if self.attention is None:
            raise RuntimeError("Attention layer not initialized.")
        return attention_pool(frames, self.attention, mask)


# ---------------------------------------------------------------------------
# LSTM, GRU and SequenceEncoder (LSTM) on the persistent HIP recurrence
# ---------------------------------------------------------------------------

_LSTM_TIMEOUT: Dict[int, torch.Tensor] = {}


def _timeout_acc(dev: torch.device) -> torch.Tensor:
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    t = _LSTM_TIMEOUT.get(idx)
    if t is None:
        t = torch.zeros(1, dtype=torch.int32, device=dev)
        _LSTM_TIMEOUT[idx] = t
    return t


def _record_timeout(flag: torch.Tensor) -> None:
    # device-side OR into the per-device accumulator: no host sync, graph-capturable
    _timeout_acc(flag.device).bitwise_or_(flag)


def _drain_op_flags() -> None:
    """Fold the timeout words of the eager LSTM / GRU operator launches (mmf_ops.LSTM_FLAGS)."""
    while _ops.LSTM_FLAGS:
        flag = _ops.LSTM_FLAGS.pop()
        if _ops.eager_tensor(flag):
            _record_timeout(flag)


def lstm_timed_out(device=None, reset: bool = True) -> bool:
    """True if any LSTM or GRU launch (both recurrences report here) on `device` since the last
    check gave up an inter-workgroup wait.  Such a launch also writes NaN into the values it never received, so its
    encodings / gradients are NaN, never silently wrong.  Reading syncs the stream;
    call it once per step (or per epoch) rather than per launch."""
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    _drain_op_flags()
    acc = _timeout_acc(dev)
    hit = bool(int(acc.item()))
    if reset:
        acc.zero_()
    return hit


def check_lstm_timeouts(device=None) -> None:
    """Raise RuntimeError if an LSTM or GRU launch timed out since the last check (see lstm_timed_out)."""
    if lstm_timed_out(device):
        raise RuntimeError("mmfusion LSTM / GRU recurrence: an inter-workgroup wait timed out (the grid was not "
                           "fully co-resident); the affected encodings / gradients are NaN")


class _Recurrent(nn.Module):
    """What LSTM and GRU share: torch's constructor arguments and attributes, the parameter names /
    shapes / registration order of nn.LSTM / nn.GRU (GATES * hidden rows per weight and bias) and its
    initialisation (uniform(-1/sqrt(hidden), 1/sqrt(hidden)) over the parameters in order), so the same
    seed gives the same weights and state dicts load either way -- but not an nn.RNNBase: TorchDynamo
    refuses to trace RNNBase modules at all ("Attempted to wrap RNN"), which would break the
    reference's torch.compile of its encoders (src/train.py:203-214)."""

    GATES: int            # gate rows per hidden unit
    KIND: str             # "LSTM" / "GRU" in the messages
    SUPPORTED: str        # what the constructor accepts

    def __init__(self, input_size: int, hidden_size: int, num_layers: int = 1, bias: bool = True,
                 batch_first: bool = False, dropout: float = 0.0, bidirectional: bool = False):
        super().__init__()
        if not bias or bidirectional:
            raise NotImplementedError(f"{self.KIND} path: {self.SUPPORTED}")
        if num_layers < 1:
            raise ValueError("num_layers must be >= 1")
        self.input_size, self.hidden_size, self.num_layers = input_size, hidden_size, num_layers
        self.bias, self.batch_first, self.dropout = bias, batch_first, float(dropout)
        self.bidirectional, self.proj_size = False, 0
        rows = self.GATES * hidden_size
        for k in range(num_layers):
            din = input_size if k == 0 else hidden_size
            self.register_parameter(f"weight_ih_l{k}", nn.Parameter(torch.empty(rows, din)))
            self.register_parameter(f"weight_hh_l{k}", nn.Parameter(torch.empty(rows, hidden_size)))
            self.register_parameter(f"bias_ih_l{k}", nn.Parameter(torch.empty(rows)))
            self.register_parameter(f"bias_hh_l{k}", nn.Parameter(torch.empty(rows)))
        self.reset_parameters()

    def reset_parameters(self) -> None:
        stdv = 1.0 / (self.hidden_size ** 0.5) if self.hidden_size > 0 else 0.0
        for w in self.parameters():
            nn.init.uniform_(w, -stdv, stdv)

    def extra_repr(self) -> str:
        s = f"{self.input_size}, {self.hidden_size}, num_layers={self.num_layers}"
        if self.batch_first:
            s += ", batch_first=True"
        if self.dropout:
            s += f", dropout={self.dropout}"
        return s

    def _run(self, input: torch.Tensor, hx) -> tuple:
        """-> the output sequence in the input's layout and the last state of every layer."""
        if hx is not None:
            raise NotImplementedError(f"{self.KIND} path: zero initial state only")
        if input.dim() != 3:
            raise ValueError(f"Expected 3-D input, got shape {tuple(input.shape)}")
        x = input if self.batch_first else input.transpose(0, 1)
        finals: list = []
        out = _recurrent_layers(self.KIND, [self], [x], finals)[0]
        return (out if self.batch_first else out.transpose(0, 1)), finals


class LSTM(_Recurrent):
    """nn.LSTM's layout (see _Recurrent; gate order i, f, g, o).  The recurrence runs on HIP
    (csrc/lstm.hip) through lstm_layers.  Supported: biased, unidirectional, no projection, zero
    initial state (the reference's configuration, src/encoders.py:68-76)."""

    GATES, KIND, SUPPORTED = 4, "LSTM", "biased, unidirectional, no projection"

    def __init__(self, input_size: int, hidden_size: int, num_layers: int = 1, bias: bool = True,
                 batch_first: bool = False, dropout: float = 0.0, bidirectional: bool = False, proj_size: int = 0):
        if proj_size:
            raise NotImplementedError(f"LSTM path: {self.SUPPORTED}")
        super().__init__(input_size, hidden_size, num_layers, bias, batch_first, dropout, bidirectional)

    def forward(self, input: torch.Tensor, hx=None):
        """-> output, (h_n, c_n) as nn.LSTM (zero initial state only).  c_n carries no gradient:
        the recurrence's backward takes d(h) only, which is all the encoders use."""
        out, finals = self._run(input, hx)
        return out, (torch.stack([h for h, _ in finals]), torch.stack([c for _, c in finals]).detach())


class GRU(_Recurrent):
    """nn.GRU's layout (see _Recurrent; weight_ih_l{k} (3H, in), weight_hh_l{k} (3H, H), bias_ih_l{k},
    bias_hh_l{k} (3H), gate order r, z, n).  The recurrence runs on HIP (csrc/gru.hip) through
    gru_layers, in fp32 FMA at every matmul-precision setting.  Supported: biased, unidirectional,
    zero initial state (the reference's configuration, src/encoders.py:78-84)."""

    GATES, KIND, SUPPORTED = 3, "GRU", "biased, unidirectional"

    def forward(self, input: torch.Tensor, hx=None):
        """-> output, h_n as nn.GRU (zero initial state only)."""
        out, finals = self._run(input, hx)
        return out, torch.stack(finals)


def _input_projection(r: nn.Module, x: torch.Tensor, k: int, bias: torch.Tensor) -> torch.Tensor:
    """Layer k's time-parallel x W_ih^T + bias on PyTorch-ROCm (autograd gives dx, dW_ih and the
    gradient of what was folded into `bias`): (B, T, in) -> (B, T, GATES * H)."""
    B, T = x.shape[:2]
    return torch.addmm(bias, _nat.f32c(x).reshape(B * T, -1), getattr(r, f"weight_ih_l{k}").t()).view(B, T, -1)


def _lstm_layer(rnns, xs, k: int):
    """xproj = x W_ih^T + b_ih + b_hh; -> every LSTM's h, the timeout word, the first LSTM's last (h, c)."""
    xproj = [_input_projection(r, x, k, getattr(r, f"bias_ih_l{k}") + getattr(r, f"bias_hh_l{k}"))
             for r, x in zip(rnns, xs)]
    hs, cs, _gates, flag = torch.ops.mmfusion.lstm_layer_fwd(
        xproj, [_nat.f32c(getattr(r, f"weight_hh_l{k}")) for r in rnns])
    return hs, flag, (hs[0][:, -1], cs[0][:, -1])


def _gru_layer(rnns, xs, k: int):
    """xproj = x W_ih^T + b_ih + [b_hr, b_hz, 0] (autograd also gives the r, z parts of db_hh); b_hn is
    multiplied by r inside the cell and goes to the kernel; -> every GRU's h, the timeout word, the
    first GRU's last h."""
    H = rnns[0].hidden_size
    xproj, b_hn = [], []
    for r, x in zip(rnns, xs):
        b_hh = getattr(r, f"bias_hh_l{k}")
        b = getattr(r, f"bias_ih_l{k}") + torch.cat((b_hh[:2 * H], b_hh.new_zeros(H)))
        xproj.append(_input_projection(r, x, k, b))
        b_hn.append(_nat.f32c(b_hh[2 * H:]))
    hs, _gates, flag = torch.ops.mmfusion.gru_layer_fwd(
        xproj, [_nat.f32c(getattr(r, f"weight_hh_l{k}")) for r in rnns], b_hn)
    return hs, flag, hs[0][:, -1]


# per recurrence kind: its layer, what its messages call the routine and the input, what it supports
_LAYERS = {"LSTM": (_lstm_layer, "lstm_layers", "SequenceEncoder input", "unidirectional, biased, no projection"),
           "GRU": (_gru_layer, "gru_layers", "GRUSequenceEncoder input", "unidirectional, biased")}


def _recurrent_layers(kind: str, rnns: Sequence[nn.Module], inputs: Sequence[torch.Tensor],
                      finals: Optional[list]) -> List[torch.Tensor]:
    """lstm_layers / gru_layers: every layer of all `rnns` as one persistent HIP launch per layer."""
    layer, name, what, supported = _LAYERS[kind]
    if len(rnns) == 0:
        return []
    H = rnns[0].hidden_size
    layers = rnns[0].num_layers
    for r in rnns:
        if not r.bias or r.bidirectional or getattr(r, "proj_size", 0):
            raise NotImplementedError(f"{kind} path: {supported}")
        if r.hidden_size != H or r.num_layers != layers:
            raise ValueError(f"{name}: all {kind}s need the same hidden_size and num_layers")
    B, T = inputs[0].shape[:2]
    for x in inputs:
        _nat.require_device(x, what)
        if x.shape[:2] != (B, T):
            raise ValueError(f"{name}: all sequences need the same (batch, seq_len)")
    cur = list(inputs)
    for k in range(layers):
        hs, flag, final = layer(rnns, cur, k)
        if _ops.eager_tensor(flag):
            _record_timeout(flag)
        if finals is not None:
            finals.append(final)
        cur = list(hs)
        if k + 1 < layers:
            cur = [torch.nn.functional.dropout(o, rnns[i].dropout, rnns[i].training) for i, o in enumerate(cur)]
    return cur


def lstm_layers(rnns: Sequence[nn.Module], inputs: Sequence[torch.Tensor],
                finals: Optional[List[tuple]] = None) -> List[torch.Tensor]:
    """Run several LSTM parameter sets (batch_first inputs, zero initial state) over their inputs on
    the HIP recurrence, every layer of all of them in one launch; returns each LSTM's top-layer
    output sequence (B, T, H).  Parameters are read by name, so an nn.LSTM serves as a parameter
    holder too.  Inter-layer dropout follows nn.LSTM (training only).  With `finals`, the first
    LSTM's last (h, c) of every layer is appended to it."""
    return _recurrent_layers("LSTM", rnns, inputs, finals)


def gru_layers(rnns: Sequence[nn.Module], inputs: Sequence[torch.Tensor],
               finals: Optional[List[torch.Tensor]] = None) -> List[torch.Tensor]:
    """lstm_layers' twin for GRU parameter sets (or nn.GRU modules); with `finals`, the first GRU's
    last h of every layer is appended to it."""
    return _recurrent_layers("GRU", rnns, inputs, finals)


def _final_state(out: torch.Tensor, lengths: Optional[torch.Tensor]) -> torch.Tensor:
    if lengths is None:
        return out[:, -1]
    idx = lengths.to(device=out.device, dtype=torch.int64) - 1
    if bool((idx < 0).any()) or bool((idx >= out.shape[1]).any()):
        raise RuntimeError("lengths must be in [1, seq_len]")
    return out[torch.arange(out.shape[0], device=out.device), idx]


class SequenceEncoder(nn.Module):
    """Time-series sequence -> fixed embedding (src/encoders.py:22-166), 'lstm' on the HIP path."""

    encoder_type: str
    hidden_dim: int
    output_dim: int
    rnn: Optional[LSTM]
    conv_net: Optional[nn.Module]
    pool: Optional[nn.Module]
    input_projection: Optional[nn.Linear]
    transformer: Optional[nn.TransformerEncoder]
    projection: nn.Module

    def __init__(self, input_dim: int, hidden_dim: int = 256, output_dim: int = 128, num_layers: int = 2,
                 encoder_type: str = "lstm", dropout: float = 0.1):
        super().__init__()
        cast_self = cast(Any, self)
        cast_self.encoder_type = encoder_type
        cast_self.hidden_dim = hidden_dim
        cast_self.output_dim = output_dim
        self.dropout_layer = nn.Dropout(dropout)
        cast_self.rnn = None
        cast_self.conv_net = None
        cast_self.pool = None
        cast_self.input_projection = None
        cast_self.transformer = None
        self.projection = nn.Identity()
        if encoder_type == "lstm":
            cast_self.rnn = LSTM(input_dim, hidden_dim, num_layers=num_layers, batch_first=True,
                                 dropout=dropout if num_layers > 1 else 0.0)
            self.projection = nn.Linear(hidden_dim, output_dim)
        elif encoder_type == "cnn":
            raise NotImplementedError("encoder_type 'cnn' is served by ConvSequenceEncoder (build_encoder returns it "
                                      "for encoder_type='cnn'), not by SequenceEncoder")
        elif encoder_type == "gru":
            raise NotImplementedError("encoder_type 'gru' is served by GRUSequenceEncoder (build_encoder returns it "
                                      "for encoder_type='gru'), not by SequenceEncoder")
        elif encoder_type == "transformer":
            raise NotImplementedError("encoder_type 'transformer' is not on the MI355X path as a SequenceEncoder: it "
                                      "is served by TransformerSequenceEncoder (build_encoder returns it for "
                                      "encoder_type='transformer')")
        else:
            raise ValueError(f"Unknown encoder type: {encoder_type}")

    def encode_final_state(self, final_state: torch.Tensor) -> torch.Tensor:
        return self.projection(self.dropout_layer(final_state))

    def forward(self, sequence: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        if sequence.dim() != 3:
            raise ValueError(f"Expected 3D input sequence, got shape {sequence.shape}")
        if self.rnn is None:
            raise RuntimeError("RNN module not initialized.")
        out = lstm_layers([self.rnn], [sequence])[0]
        return self.encode_final_state(_final_state(out, lengths))


class GRUSequenceEncoder(nn.Module):
    """The reference SequenceEncoder's 'gru' branch (src/encoders.py:77-85, 135-166) on the HIP path: the
    same attributes, construction order (the same seed gives the same weights) and state_dict
    (rnn.*, projection.*).  With `lengths` the final state is read from the output at lengths - 1
    (what packing computes), as the LSTM path does."""

    encoder_type: str
    hidden_dim: int
    output_dim: int
    rnn: Optional[GRU]
    conv_net: Optional[nn.Module]
    pool: Optional[nn.Module]
    input_projection: Optional[nn.Linear]
    transformer: Optional[nn.TransformerEncoder]
    projection: nn.Module

    def __init__(self, input_dim: int, hidden_dim: int = 256, output_dim: int = 128, num_layers: int = 2,
                 dropout: float = 0.1):
        super().__init__()
        cast_self = cast(Any, self)
        cast_self.encoder_type = "gru"
        cast_self.hidden_dim = hidden_dim
        cast_self.output_dim = output_dim
        self.dropout_layer = nn.Dropout(dropout)
        cast_self.conv_net = None
        cast_self.pool = None
        cast_self.input_projection = None
        cast_self.transformer = None
        self.projection = nn.Identity()   # (registered first, as in the reference: the module order)
        cast_self.rnn = GRU(input_dim, hidden_dim, num_layers=num_layers, batch_first=True,
                            dropout=dropout if num_layers > 1 else 0.0)
        self.projection = nn.Linear(hidden_dim, output_dim)

    def encode_final_state(self, final_state: torch.Tensor) -> torch.Tensor:
        return self.projection(self.dropout_layer(final_state))

    def forward(self, sequence: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        if sequence.dim() != 3:
            raise ValueError(f"Expected 3D input sequence, got shape {sequence.shape}")
        if self.rnn is None:
            raise RuntimeError("RNN module not initialized.")
        out = gru_layers([self.rnn], [sequence])[0]
        return self.encode_final_state(_final_state(out, lengths))


class ConvSequenceEncoder(nn.Module):
    """The reference SequenceEncoder's 'cnn' branch (src/encoders.py:87-97, 168-175) on the HIP path:
    the same attributes, construction order (the same seed gives the same weights) and state_dict.
    ``conv_net`` is the reference's nn.Sequential and only holds the parameters and buffers; the
    stack runs in csrc/conv_encoder.hip.  ``num_layers`` is accepted and ignored, as there."""

    encoder_type: str
    hidden_dim: int
    output_dim: int
    rnn: Optional[nn.Module]
    conv_net: Optional[nn.Module]
    pool: Optional[nn.Module]
    input_projection: Optional[nn.Linear]
    transformer: Optional[nn.TransformerEncoder]
    projection: nn.Module

    def __init__(self, input_dim: int, hidden_dim: int = 256, output_dim: int = 128, num_layers: int = 2,
                 dropout: float = 0.1):
        super().__init__()
        cast_self = cast(Any, self)
        cast_self.encoder_type = "cnn"
        cast_self.hidden_dim = hidden_dim
        cast_self.output_dim = output_dim
        self.dropout_layer = nn.Dropout(dropout)
        cast_self.rnn = None
        cast_self.input_projection = None
        cast_self.transformer = None
        cast_self.conv_net = nn.Sequential(
            nn.Conv1d(input_dim, hidden_dim, kernel_size=3, padding=1), nn.BatchNorm1d(hidden_dim), nn.ReLU(),
            nn.Conv1d(hidden_dim, hidden_dim, kernel_size=3, padding=1), nn.BatchNorm1d(hidden_dim), nn.ReLU())
        cast_self.pool = nn.AdaptiveAvgPool1d(1)
        self.projection = nn.Linear(hidden_dim, output_dim)

    def _stack(self):
        """(conv1, bn1, conv2, bn2) when conv_net is still the structure the kernels implement."""
        net = self.conv_net
        mods = list(net.children()) if isinstance(net, nn.Sequential) else []
        kinds = (nn.Conv1d, nn.BatchNorm1d, nn.ReLU, nn.Conv1d, nn.BatchNorm1d, nn.ReLU)
        ok = len(mods) == 6 and all(isinstance(m, k) for m, k in zip(mods, kinds))
        if ok:
            c1, b1, _, c2, b2, _ = mods
            for c in (c1, c2):
                ok = ok and (c.kernel_size, c.stride, c.padding, c.dilation, c.groups) == ((3,), (1,), (1,), (1,), 1)
                ok = ok and c.padding_mode == "zeros" and c.bias is not None
            for b in (b1, b2):
                ok = ok and b.affine and b.track_running_stats and b.running_mean is not None
            ok = ok and c1.out_channels == c2.in_channels == c2.out_channels == b1.num_features == b2.num_features
            ok = ok and b1.training == b2.training
            ok = ok and isinstance(self.pool, nn.AdaptiveAvgPool1d) and self.pool.output_size in (1, (1,))
        if not ok:
            raise NotImplementedError("ConvSequenceEncoder: the HIP path implements Conv1d(k=3, padding=1) -> "
                                      "BatchNorm1d -> ReLU, twice, -> AdaptiveAvgPool1d(1) only (there is no torch "
                                      "fallback)")
        return c1, b1, c2, b2

    @staticmethod
    def _track(bn: nn.BatchNorm1d, stat: torch.Tensor, n: int) -> None:
        """torch's running-statistics rule from the batch statistics the kernel returned (mean, biased
        variance): a few tiny device ops, no host sync."""
        with torch.no_grad():
            bn.num_batches_tracked.add_(1)
            if bn.momentum is None:
                f = 1.0 / bn.num_batches_tracked.to(torch.float32)   # cumulative moving average
            else:
                f = float(bn.momentum)
            mean, var = stat[0], stat[1] * (n / (n - 1))
            bn.running_mean.mul_(1.0 - f).add_(mean * f)
            bn.running_var.mul_(1.0 - f).add_(var * f)

    def forward(self, sequence: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        if sequence.dim() != 3:
            raise ValueError(f"Expected 3D input sequence, got shape {sequence.shape}")
        if self.conv_net is None or self.pool is None:
            raise RuntimeError("CNN modules not initialized.")
        c1, b1, c2, b2 = self._stack()
        _nat.require_device(sequence, "ConvSequenceEncoder input")
        x = _nat.f32c(sequence)
        B, T, _ = x.shape
        training = bool(b1.training)
        if training and B * T <= 1:
            raise ValueError("Expected more than 1 value per channel when training, got input size "
                             f"{torch.Size([B, c1.out_channels, T])}")
        # (Cout, Cin, 3) -> (Cout, 3, Cin): autograd permutes the gradient back to torch's layout
        w1 = c1.weight.permute(0, 2, 1).contiguous()
        w2 = c2.weight.permute(0, 2, 1).contiguous()
        pooled, _y1, _y2, stat1, stat2 = torch.ops.mmfusion.conv_encoder_fwd(
            x, w1, c1.bias, b1.weight, b1.bias, b1.running_mean, b1.running_var,
            w2, c2.bias, b2.weight, b2.bias, b2.running_mean, b2.running_var, training, float(b1.eps), float(b2.eps))
        if training:
            self._track(b1, stat1.detach(), B * T)
            self._track(b2, stat2.detach(), B * T)
        return self.projection(self.dropout_layer(pooled))


class TransformerSequenceEncoder(nn.Module):
    """The reference SequenceEncoder's 'transformer' branch (src/encoders.py:99-111, 177-206) on the HIP
    path: the same attributes, construction order (the same seed gives the same weights) and
    state_dict (input_projection.*, transformer.layers.{k}.*, projection.*).  ``transformer`` is the
    reference's nn.TransformerEncoder and only holds the parameters; the layer stack, the key padding
    mask from ``lengths`` and the mean over the valid steps run in csrc/transformer.hip.  A sample of
    length 0 encodes as projection(0) with zero gradients where the reference gives NaN."""

    encoder_type: str
    hidden_dim: int
    output_dim: int
    rnn: Optional[nn.Module]
    conv_net: Optional[nn.Module]
    pool: Optional[nn.Module]
    input_projection: Optional[nn.Linear]
    transformer: Optional[nn.TransformerEncoder]
    projection: nn.Module

    def __init__(self, input_dim: int, hidden_dim: int = 256, output_dim: int = 128, num_layers: int = 2,
                 dropout: float = 0.1):
        super().__init__()
        cast_self = cast(Any, self)
        cast_self.encoder_type = "transformer"
        cast_self.hidden_dim = hidden_dim
        cast_self.output_dim = output_dim
        self.dropout_layer = nn.Dropout(dropout)
        cast_self.rnn = None
        cast_self.conv_net = None
        cast_self.pool = None
        cast_self.input_projection = None
        cast_self.transformer = None
        self.projection = nn.Identity()   # (registered first, as in the reference: the module order)
        cast_self.input_projection = nn.Linear(input_dim, hidden_dim)
        nhead = 4 if hidden_dim % 4 == 0 else 1
        encoder_layer = nn.TransformerEncoderLayer(d_model=hidden_dim, nhead=nhead, dropout=dropout, batch_first=True)
        cast_self.transformer = nn.TransformerEncoder(encoder_layer, num_layers=num_layers)
        self.projection = nn.Linear(hidden_dim, output_dim)
        from attention import _new_rng_state   # the device Philox state of one module; torch's RNG untouched
        self.register_buffer("_rng_state", _new_rng_state(), persistent=False)

    def _stack(self):
        """(layers, dropout p, LayerNorm eps) when ``transformer`` is still the structure the kernels
        implement: post-norm ReLU layers with biases, 4 heads, batch_first, no final norm."""
        net = self.transformer
        layers = list(net.layers) if isinstance(net, nn.TransformerEncoder) else []
        ok = len(layers) >= 1 and net.norm is None
        p = eps = None
        for lyr in layers:
            ok = ok and isinstance(lyr, nn.TransformerEncoderLayer)
            if not ok:
                break
            att = lyr.self_attn
            act = lyr.activation
            relu = act is torch.nn.functional.relu or act is torch.relu or isinstance(act, nn.ReLU)
            ok = ok and not lyr.norm_first and relu
            ok = ok and isinstance(att, nn.MultiheadAttention) and att.batch_first and att._qkv_same_embed_dim
            ok = ok and att.num_heads == 4 and att.in_proj_bias is not None and att.out_proj.bias is not None
            ok = ok and att.bias_k is None and att.bias_v is None and not att.add_zero_attn
            ok = ok and lyr.linear1.bias is not None and lyr.linear2.bias is not None
            ok = ok and isinstance(lyr.norm1, nn.LayerNorm) and isinstance(lyr.norm2, nn.LayerNorm)
            ok = ok and lyr.norm1.elementwise_affine and lyr.norm2.elementwise_affine
            ok = ok and lyr.norm1.bias is not None and lyr.norm2.bias is not None
            if not ok:
                break
            ps = {float(att.dropout), float(lyr.dropout.p), float(lyr.dropout1.p), float(lyr.dropout2.p)}
            es = {float(lyr.norm1.eps), float(lyr.norm2.eps)}
            ok = ok and len(ps) == 1 and len(es) == 1
            ok = ok and (p is None or p == next(iter(ps))) and (eps is None or eps == next(iter(es)))
            p, eps = next(iter(ps)), next(iter(es))
            ok = ok and lyr.linear1.in_features == lyr.linear2.out_features == att.embed_dim == self.hidden_dim
            ok = ok and lyr.linear1.out_features == lyr.linear2.in_features
            ok = ok and lyr.linear1.out_features == layers[0].linear1.out_features
        if not ok:
            raise NotImplementedError("TransformerSequenceEncoder: the HIP path implements a stack of post-norm "
                                      "nn.TransformerEncoderLayer (4 heads, ReLU, biases, batch_first, equal dropout "
                                      "and eps, no final norm) only (there is no torch fallback)")
        return layers, p, eps

    def forward(self, sequence: torch.Tensor, lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        if sequence.dim() != 3:
            raise ValueError(f"Expected 3D input sequence, got shape {sequence.shape}")
        if self.input_projection is None or self.transformer is None:
            raise RuntimeError("Transformer modules not initialized.")
        layers, p, eps = self._stack()
        _nat.require_device(sequence, "TransformerSequenceEncoder input")
        x = _nat.f32c(self.input_projection(_nat.f32c(sequence)))
        lens = None
        if lengths is not None:
            lens = lengths.to(device=x.device, dtype=torch.int64).contiguous()
        params: List[torch.Tensor] = []
        for lyr in layers:
            att = lyr.self_attn
            params += [att.in_proj_weight, att.in_proj_bias, att.out_proj.weight, att.out_proj.bias,
                       lyr.linear1.weight, lyr.linear1.bias, lyr.linear2.weight, lyr.linear2.bias,
                       lyr.norm1.weight, lyr.norm1.bias, lyr.norm2.weight, lyr.norm2.bias]
        pooled, _saved, rng_next = torch.ops.mmfusion.transformer_encoder_fwd(
            x, lens, self._rng_state, params, bool(self.transformer.training), float(p), float(eps))
        self._rng_state.copy_(rng_next)     # the device Philox stream advanced by one call
        return self.projection(self.dropout_layer(pooled))


def build_encoder(modality: str, input_dim: int, output_dim: int,
                  encoder_config: Optional[Dict[str, Any]] = None) -> nn.Module:
    """The reference's factory (src/encoders.py:400-451): the config's ``type`` ('frame' /
    'sequence' / 'mlp') decides, else the modality name (video / frames -> FrameEncoder; imu /
    audio / mocap / accelerometer / imu_* -> sequence).  A sequence encoder with
    ``encoder_type == 'cnn'`` is a ConvSequenceEncoder, with 'gru' a GRUSequenceEncoder, with
    'transformer' a TransformerSequenceEncoder, any other a SequenceEncoder.  The MLP
    encoder (type 'mlp' and unknown modalities) is not on the MI355X path."""
    config: Dict[str, Any] = dict(encoder_config) if encoder_config else {}
    kind = config.pop("type", None)
    key = modality.lower()
    by_name = kind not in ("frame", "sequence", "mlp")
    if kind == "frame" or (by_name and key in ("video", "frames")):
        return FrameEncoder(frame_dim=input_dim, output_dim=output_dim, **config)
    if kind == "sequence" or (by_name and (key in ("imu", "audio", "mocap", "accelerometer") or key.startswith("imu_"))):
        if config.get("encoder_type", "lstm") == "cnn":
            config.pop("encoder_type")
            return ConvSequenceEncoder(input_dim=input_dim, output_dim=output_dim, **config)
        if config.get("encoder_type", "lstm") == "gru":
            config.pop("encoder_type")
            return GRUSequenceEncoder(input_dim=input_dim, output_dim=output_dim, **config)
        if config.get("encoder_type", "lstm") == "transformer":
            config.pop("encoder_type")
            return TransformerSequenceEncoder(input_dim=input_dim, output_dim=output_dim, **config)
        return SequenceEncoder(input_dim=input_dim, output_dim=output_dim, **config)
    # SimpleMLPEncoder (src/encoders.py:339-397) serves config 1's EarlyFusion CPU plumbing only
    raise NotImplementedError(f"encoder for modality '{modality}' ({kind or 'mlp'}) is not on the MI355X path")


def recurrence_kind(encoder: nn.Module) -> Optional[str]:
    """'lstm' / 'gru' for an encoder that runs on one of the persistent recurrences, else None."""
    if isinstance(encoder, GRUSequenceEncoder):
        return "gru"
    if isinstance(encoder, SequenceEncoder) and encoder.encoder_type == "lstm":
        return "lstm"
    return None


def encode_sequences(encoders: Dict[str, nn.Module], sequences: Dict[str, torch.Tensor],
                     lengths: Optional[torch.Tensor] = None) -> Dict[str, torch.Tensor]:
    """{m: encoders[m](sequences[m], lengths)} for SequenceEncoder ('lstm') and GRUSequenceEncoder
    modules, with every modality's layers of one recurrence kind sharing launches (the modalities of
    one chunk have the same (B, T)): one batched call per kind, results in the order of `sequences`."""
    names = list(sequences)
    for m in names:
        if sequences[m].dim() != 3:
            raise ValueError(f"Expected 3D input sequence, got shape {sequences[m].shape}")
    by_kind: Dict[str, List[str]] = {}
    for m in names:
        kind = recurrence_kind(encoders[m])
        if kind is None:
            raise TypeError(f"encode_sequences: encoder '{m}' ({type(encoders[m]).__name__}) is neither an LSTM "
                            "SequenceEncoder nor a GRUSequenceEncoder")
        if encoders[m].rnn is None:
            raise RuntimeError("RNN module not initialized.")
        by_kind.setdefault(kind, []).append(m)
    outs: Dict[str, torch.Tensor] = {}
    for kind, ms in by_kind.items():
        run = lstm_layers if kind == "lstm" else gru_layers
        for m, o in zip(ms, run([encoders[m].rnn for m in ms], [sequences[m] for m in ms])):
            outs[m] = o
    return {m: encoders[m].encode_final_state(_final_state(outs[m], lengths)) for m in names}
