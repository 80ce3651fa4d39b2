"""Uncertainty quantification on MI355X HIP kernels: MC dropout, ensembles, uncertainty-weighted
fusion and temperature scaling (src/uncertainty.py of the reference).

Constructors, ``forward`` signatures, return values and error messages are the reference's:

  * ``MCDropoutUncertainty(model, num_samples=10)``: ``forward(*args, **kwargs) -> (mean_logits
    (B, C), variance (B,))`` (src/uncertainty.py:19-71).  When ``model`` is this package's
    ``HybridFusion`` called as ``(modality_features, modality_mask=None)`` on float32 device
    tensors, the S train-mode forwards and the reduction are ONE C-ABI call
    (``mmf_hybrid_mc_forward``: S forwards of the plan the shapes select, each advancing the
    dropout offset on the device, then one ``mc_reduce_kernel`` launch) -- eager only, a ctypes
    call like the grad-sink forward's.  Any other module, other call forms, and every call traced
    by ``torch.compile`` take the generic loop: S module calls, each copied into its slot of a
    preallocated (S, B, C) stack, then ``torch.ops.mmfusion.mc_reduce``.  Both paths run the same
    kernels in the same order and give identical bits.  ``logits_stack`` holds the last call's
    samples (a buffer the next call with the same input signature overwrites).
  * ``EnsembleUncertainty(models).predict_with_uncertainty(inputs) -> (mean_probs, variance)``
    (:441-492), reduced by the same kernel.
  * ``UncertaintyWeightedFusion(epsilon=1e-6)`` (:286-362) on ``mmf_uncertainty_fusion_*``,
    differentiable with respect to the predictions and the uncertainties.
  * ``TemperatureScaling`` (:365-438): ``calibrate`` runs the reference's ``torch.optim.LBFGS``
    loop; its closure is one ``mmf_temperature_nll`` call (loss and d loss / dT, T read from the
    device) with ``temperature.grad`` assigned directly -- no autograd graph.

The variance is the population variance (``unbiased=False``) of the softmax outputs over the
samples, averaged over the classes, accumulated in Welford's form (csrc/uncertainty.hip).

The module is not named ``uncertainty`` for the reason calibration.py gives: the reference's own
``uncertainty`` module must keep resolving when this package sits ahead of ``src/`` on
``sys.path``.  ``CalibrationMetrics`` (ECE / MCE / NLL) is calibration.py; the reliability
diagram stays the reference's.  No CPU path exists: CPU tensors raise.
"""

from __future__ import annotations

import ctypes
import os
import sys
from typing import Any, Dict, List, Optional, Sequence, Tuple, cast

import torch
import torch.nn as nn

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import mmf_native as _nat  # noqa: E402
import mmf_ops as _ops  # noqa: E402
from attention import _precision  # noqa: E402
from fusion import HybridFusion, _check_mask  # noqa: E402


def _first_tensor(obj) -> Optional[torch.Tensor]:
    if torch.is_tensor(obj):
        return obj
    if isinstance(obj, dict):
        obj = list(obj.values())
    if isinstance(obj, (list, tuple)):
        for v in obj:
            t = _first_tensor(v)
            if t is not None:
                return t
    return None


def _stack_samples(call, count: int) -> torch.Tensor:
    """`count` calls of `call(i)` -> (count, B, C) float32 stack, each result copied into its slot."""
    stack = None
    for i in range(count):
        logits = call(i)
        if stack is None:
            _nat.require_device(logits, "model output")
            if logits.dim() != 2:
                raise RuntimeError(f"expected (batch_size, num_classes) logits, got shape {tuple(logits.shape)}")
            stack = torch.empty((count,) + tuple(logits.shape), dtype=torch.float32, device=logits.device)
        stack[i].copy_(logits)
    return stack


class MCDropoutUncertainty(nn.Module):
    """Monte Carlo dropout: ``num_samples`` train-mode forwards, mean logits and the variance of
    the softmax outputs (src/uncertainty.py:19-71)."""

    model: nn.Module
    num_samples: int

    def __init__(self, model: nn.Module, num_samples: int = 10):
        super().__init__()
        cast_self = cast(Any, self)
        cast_self.model = model
        cast_self.num_samples = num_samples
        cast_self.logits_stack = None

    def forward(self, *args, **kwargs) -> Tuple[torch.Tensor, torch.Tensor]:
        if self.num_samples < 1:
            raise RuntimeError("torch.cat(): expected a non-empty list of Tensors")
        first = _first_tensor(args) if args else _first_tensor(kwargs)
        if first is not None:
            _nat.require_device(first, "MCDropoutUncertainty input")
        was_training = self.model.training
        self.model.train()
        try:
            with torch.no_grad():
                fused = self._fused_inputs(args, kwargs)
                if fused is not None:
                    mean_logits, variance = self._fused(*fused)
                else:
                    stack = _stack_samples(lambda _: self.model(*args, **kwargs), self.num_samples)
                    cast(Any, self).logits_stack = stack
                    mean_logits, _, variance = torch.ops.mmfusion.mc_reduce(stack)
        finally:
            if not was_training:
                self.model.eval()
        return mean_logits, variance

    # ------------------------------------------------------------------ fused path
    def _fused_inputs(self, args, kwargs):
        """(features in modality order, mask or None) when the call is HybridFusion's
        ``(modality_features, modality_mask=None)`` on float32 device tensors in eager mode."""
        model = self.model
        if type(model) is not HybridFusion or torch.compiler.is_compiling() or not model.modality_names:
            return None
        kw = dict(kwargs)
        if len(args) > 2 or (len(args) > 0 and "modality_features" in kw) or (len(args) > 1 and "modality_mask" in kw):
            return None
        feats = args[0] if args else kw.pop("modality_features", None)
        mask = args[1] if len(args) > 1 else kw.pop("modality_mask", None)
        if kw or not isinstance(feats, dict):
            return None
        xs = []
        for name in model.modality_names:
            x = feats.get(name)
            if x is None or not _ops.eager_tensor(x) or x.dtype != torch.float32 or x.device.type != "cuda":
                return None
            xs.append(x)
        if any(x.device != xs[0].device for x in xs):
            return None
        if mask is not None and not _ops.eager_tensor(mask):
            return None
        return xs, mask

    def _fused(self, xs: List[torch.Tensor], mask: Optional[torch.Tensor]) -> Tuple[torch.Tensor, torch.Tensor]:
        model = cast(HybridFusion, self.model)
        L = _nat.lib()
        S = int(self.num_samples)
        B, dev = xs[0].size(0), xs[0].device
        M, C = model.num_modalities, model.num_classes
        if mask is None:
            mask = torch.ones(B, M, device=dev, dtype=torch.float32)
        else:
            mask = _check_mask(mask.to(device=dev, dtype=torch.float32), B, M, "HybridFusion")
        pairs, params, in_dims, _ = model._op_params(dev)
        p = float(model.dropout.p)
        key = (tuple(tuple(x.shape) for x in xs), S, _precision(), p, int(L.mmf_hybrid_plan_flags()),
               tuple(k for _, _, k in pairs), dev)
        cache = self.__dict__.setdefault("_mmf_mc_cache", {})
        hit = cache.get(key)
        if hit is None:
            seq, dims = model._shapes(xs, in_dims)
            idesc = _ops.hybrid_idesc(B, model.hidden_dim, model.num_heads, C, seq, dims,
                                      [(q, k) for q, k, _ in pairs], True, False, _precision())
            # (a copy: the shared descriptor's capacities belong to the forward operators)
            d = _nat.HybridDesc.from_buffer_copy(_ops.hybrid_desc(idesc, p))
            saved = torch.empty(L.mmf_hybrid_saved_bytes(ctypes.byref(d)), dtype=torch.uint8, device=dev)
            d.saved_capacity = saved.numel()
            stack = torch.empty(S, B, C, dtype=torch.float32, device=dev)
            fw = torch.empty(B, M, dtype=torch.float32, device=dev)
            if len(cache) >= 8:
                cache.clear()
            hit = cache[key] = (d, saved, stack, fw)
        d, saved, stack, fw = hit
        mean_logits = torch.empty(B, C, dtype=torch.float32, device=dev)
        variance = torch.empty(B, dtype=torch.float32, device=dev)
        xs = [_nat.f32c(x) for x in xs]
        mask = _nat.f32c(mask)
        pstruct = _ops._hybrid_params_struct(params, M, len(pairs))
        xarr = _nat.ptr_array([x.data_ptr() for x in xs])
        rc = L.mmf_hybrid_mc_forward(ctypes.byref(d), ctypes.byref(pstruct), ctypes.cast(xarr, ctypes.c_void_p),
                                     mask.data_ptr(), model._rng_state.data_ptr(), S, saved.data_ptr(),
                                     stack.data_ptr(), fw.data_ptr(), mean_logits.data_ptr(), None,
                                     variance.data_ptr(), _nat.stream_ptr(dev))
        _nat.check(rc, "MC dropout forward")
        cast(Any, self).logits_stack = stack
        return mean_logits, variance


class UncertaintyWeightedFusion(nn.Module):
    """Fuse modality predictions weighted by inverse uncertainty (src/uncertainty.py:286-362)."""

    epsilon: float

    def __init__(self, epsilon: float = 1e-6):
        super().__init__()
        cast_self = cast(Any, self)
        cast_self.epsilon = epsilon

    def forward(self, modality_predictions: Dict[str, torch.Tensor], modality_uncertainties: Dict[str, torch.Tensor],
                modality_mask: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        modality_names = list(modality_predictions.keys())
        if not modality_names:
            raise ValueError("No modality predictions supplied for fusion.")
        num_modalities = len(modality_names)
        device = next(iter(modality_predictions.values())).device
        logits_list, unc_list = [], []
        for modality in modality_names:
            if modality not in modality_uncertainties:
                raise KeyError(f"Missing uncertainty for modality '{modality}'.")
            logits_list.append(modality_predictions[modality].to(device))
            unc_list.append(modality_uncertainties[modality].to(device))
        _nat.require_device(logits_list[0], "UncertaintyWeightedFusion predictions")
        stacked = torch.stack(logits_list, dim=1)      # (B, M, C)
        uncertainty = torch.stack(unc_list, dim=1)     # (B, M)
        if stacked.dim() != 3 or uncertainty.shape != stacked.shape[:2]:
            raise RuntimeError("UncertaintyWeightedFusion: predictions must be (batch_size, num_classes) and "
                               f"uncertainties (batch_size,), got {tuple(stacked.shape)} and {tuple(uncertainty.shape)}")
        mask = _check_mask(modality_mask.to(device=device, dtype=torch.float32), stacked.size(0), num_modalities,
                           "UncertaintyWeightedFusion")
        fused, weights = torch.ops.mmfusion.uncertainty_fusion_fwd(_nat.f32c(stacked), _nat.f32c(uncertainty),
                                                                   _nat.f32c(mask), float(self.epsilon))
        return fused, weights.detach()


class TemperatureScaling(nn.Module):
    """Post-hoc calibration by one temperature, P = softmax(logits / T) (src/uncertainty.py:365-438)."""

    temperature: nn.Parameter

    def __init__(self):
        super().__init__()
        self.temperature = nn.Parameter(torch.ones(1))

    def forward(self, logits: torch.Tensor) -> torch.Tensor:
        return logits / self.temperature

    def calibrate(self, logits: torch.Tensor, labels: torch.Tensor, lr: float = 0.01, max_iter: int = 50) -> None:
        """Learn T on a validation set: the reference's LBFGS loop, its closure one
        ``mmf_temperature_nll`` launch pair on the device (no autograd graph)."""
        logits = logits.detach()
        labels = labels.detach().to(dtype=torch.long)
        _nat.require_device(logits, "TemperatureScaling logits")
        if logits.dim() != 2:
            raise RuntimeError(f"expected (N, num_classes) logits, got shape {tuple(logits.shape)}")

        if logits.device != self.temperature.device:
            temp_param = self.temperature
            if temp_param.device.type == "meta":
                new_value = torch.ones(temp_param.shape, device=logits.device, dtype=temp_param.dtype)
            else:
                new_value = temp_param.detach().to(device=logits.device)
            self.temperature = nn.Parameter(new_value)

        self.temperature.data = torch.ones_like(self.temperature.data)
        logits = _nat.f32c(logits)
        labels = labels.to(logits.device).contiguous()

        optimizer = torch.optim.LBFGS([self.temperature], lr=lr, max_iter=max_iter)

        def closure():
            optimizer.zero_grad()
            loss, dtemp = torch.ops.mmfusion.temperature_nll(logits, labels, self.temperature.detach())
            self.temperature.grad = dtemp.to(self.temperature.dtype)
            return loss

        optimizer.step(closure)
        self.temperature.data = self.temperature.data.clamp(min=1e-3)


class EnsembleUncertainty:
    """Uncertainty as the variance across an ensemble's predictions (src/uncertainty.py:441-492)."""

    models: List[nn.Module]
    num_models: int

    def __init__(self, models: Sequence[nn.Module]):
        self.models = list(models)
        self.num_models = len(self.models)

    def predict_with_uncertainty(self, inputs) -> Tuple[torch.Tensor, torch.Tensor]:
        """-> (mean softmax over the models (B, C), variance (B,))."""
        if self.num_models == 0:
            raise ValueError("Ensemble must contain at least one model.")
        first = _first_tensor(inputs)
        if first is not None:
            _nat.require_device(first, "EnsembleUncertainty input")

        def run(i: int) -> torch.Tensor:
            model = self.models[i]
            was_training = model.training
            model.eval()
            try:
                return model(inputs)
            finally:
                if was_training:
                    model.train()

        with torch.no_grad():
            stack = _stack_samples(run, self.num_models)
            _, mean_probs, variance = torch.ops.mmfusion.mc_reduce(stack)
        return mean_probs, variance
