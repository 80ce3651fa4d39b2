"""Evaluation on the HIP path: the missing-modality robustness sweep (src/eval.py:312-458) and the
standard evaluation (src/eval.py:39-309, 534-611 with src/uncertainty.py:84-283).

The reference's ``evaluate_missing_modalities`` (switched on by ``evaluation.missing_modality_test``)
scores the model under every one of the 2^M - 1 modality subsets: accuracy and macro-F1 per subset,
then a per-modality importance from those.  It walks the dataloader once per subset and runs the
whole model each time, although only the mask differs.

For ``HybridFusion`` a 0/1 pattern that is constant over the batch reaches the logits only through
constants (include/mmfusion.h, mmf_hybrid_sweep_forward): one shared pass under the all-present mask
serves every pattern, and a small per-(pattern, sample) tail -- aggregate by selection, gating
softmax, weighted sum, classifier -- is all that is left per pattern (``hybrid_mask_sweep``).  The
predictions never leave the device: ``torch.ops.mmfusion.confusion_accumulate`` counts them into
one confusion matrix per subset, read back once at the end.

The standard evaluation follows the same rule.  The reference's ``evaluate_model`` reads the device
five times per batch (``loss.item()`` and four ``.cpu()``, src/eval.py:81-94) and the
``CalibrationMetrics`` chain bins the confidences on the host.  Here
``torch.ops.mmfusion.eval_accumulate`` turns each batch's logits and labels into every statistic
accuracy / macro-F1 / loss / NLL / ECE / MCE need, in a device state (``EvalAccumulator``) that
``result()`` reads once; ``evaluate_model``, ``measure_inference_latency``, ``attention_matrix`` /
``generate_attention_visualization``, ``reliability_diagram`` and ``standard_evaluation`` restate
the reference's "Standard Evaluation" section over it.

This is a separate module name (not ``eval``) so that the reference's own ``eval`` keeps resolving
under ``mmf_launch``, for the reason ``calibration.py`` gives.
"""

from __future__ import annotations

import itertools
import json
import os
import sys
from collections.abc import Mapping
from collections.abc import Sequence as _SequenceABC
from pathlib import Path
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

import mmf_native as _nat  # noqa: E402
import mmf_ops as _ops  # noqa: E402
from fusion import HybridFusion, _precision  # noqa: E402

# the sweep's limits (csrc/mmf_internal.h SWEEP_MAX_*): the tail kernel's LDS tile and class loop
MAX_HIDDEN, MAX_CLASSES = 256, 1024


def sweep_supported(model: HybridFusion) -> bool:
    """Whether ``hybrid_mask_sweep`` serves this model: ``HybridFusion.forward`` takes hidden_dim up
    to 1024, the sweep's tail up to 256 (and 1024 classes).  ``evaluate_missing_modalities`` runs
    the per-subset loop for the others."""
    return model.hidden_dim <= MAX_HIDDEN and model.num_classes <= MAX_CLASSES


def modality_subsets(num_modalities: int) -> List[Tuple[int, ...]]:
    """The non-empty index subsets in the reference's order (src/eval.py:342-348):
    ``itertools.combinations`` by size 1..M."""
    out: List[Tuple[int, ...]] = []
    for size in range(1, num_modalities + 1):
        out.extend(itertools.combinations(range(num_modalities), size))
    return out


def _pattern_rows(patterns, num_modalities: int) -> List[List[int]]:
    rows = patterns.tolist() if hasattr(patterns, "tolist") else [list(r) for r in patterns]
    for r in rows:
        if len(r) != num_modalities:
            raise ValueError(f"a modality pattern has {len(r)} entries for {num_modalities} modalities")
        for v in r:
            if v != 0 and v != 1:
                raise ValueError(f"modality patterns are 0/1 (fractional masks are out of scope), got {v!r}")
    return [[int(v) for v in r] for r in rows]


def hybrid_mask_sweep(model: HybridFusion, modality_features: Dict[str, torch.Tensor], patterns,
                      return_weights: bool = False):
    """Logits (S, B, C) of ``model`` in eval mode under S 0/1 modality patterns (S, M), each applied
    to the whole batch as the reference's missing-modality test does (features of an absent modality
    zeroed, mask column 0: src/eval.py:394-404); with ``return_weights`` also the fusion weights
    (S, B, M).  One shared pass, one tail launch; the library takes up to 1024 patterns, hidden_dim
    up to 256 and 1024 classes (``sweep_supported``).  Inference only: the results never require
    grad.  Carries ``HybridFusion.forward``'s errors."""
    if not model.modality_names:
        raise ValueError("No modalities configured for HybridFusion.")
    M = model.num_modalities
    rows = _pattern_rows(patterns, M)
    if not rows:
        raise ValueError("hybrid_mask_sweep needs at least one pattern")
    feats = []
    for name in model.modality_names:
        if name not in modality_features:
            raise KeyError(f"Missing features for modality '{name}' in HybridFusion forward pass.")
        feats.append(modality_features[name])
    ref = feats[0]
    _nat.require_device(ref, "HybridFusion input")
    device = ref.device
    with torch.no_grad():
        feats = [_nat.f32c(x.detach().to(device)) for x in feats]
        pairs, params, in_dims, _ = model._op_params(device)
        seq, dims = model._shapes(feats, in_dims)
        idesc = _ops.hybrid_idesc(ref.size(0), model.hidden_dim, model.num_heads, model.num_classes, seq, dims,
                                  [(q, k) for q, k, _ in pairs], False, False, _precision())
        logits, weights = torch.ops.mmfusion.hybrid_mask_sweep(
            idesc, float(model.dropout.p), [v for r in rows for v in r], feats, [p.detach() for p in params],
            bool(return_weights))
    return (logits, weights) if return_weights else logits


def metrics_from_confusion(counts) -> Dict[str, float]:
    """{"accuracy", "f1_macro"} of one confusion matrix counts[label, pred], on the host in float64.
    Macro-F1 as ``sklearn.metrics.f1_score(average="macro", zero_division=0)``: the mean over the
    classes that occur in the labels or the predictions of 2 tp / (2 tp + fp + fn)."""
    c = np.asarray(counts.detach().cpu().numpy() if isinstance(counts, torch.Tensor) else counts, dtype=np.float64)
    if c.ndim != 2 or c.shape[0] != c.shape[1]:
        raise ValueError(f"a confusion matrix is (C, C), got {c.shape}")
    total = c.sum()
    tp = np.diag(c)
    support, predicted = c.sum(axis=1), c.sum(axis=0)
    seen = (support + predicted) > 0
    if total == 0 or not seen.any():
        return {"accuracy": 0.0, "f1_macro": 0.0}
    f1 = 2.0 * tp[seen] / (support[seen] + predicted[seen])   # 2 tp + fp + fn = row sum + column sum
    return {"accuracy": float(tp.sum() / total), "f1_macro": float(f1.mean())}


def modality_importance(results: Dict[str, Any], modality_names: Sequence[str]) -> Dict[str, float]:
    """src/eval.py:427-458: mean accuracy of the combinations whose NAME contains the modality's name
    minus the mean of the others (the reference's substring test: "imu" also matches "imu_hand+..."),
    normalised by the sum of absolute values."""
    importance: Dict[str, float] = {}
    for modality in modality_names:
        with_scores, without_scores = [], []
        for combo_name, metrics in results["all_combinations"].items():
            (with_scores if modality in combo_name else without_scores).append(metrics["accuracy"])
        if with_scores and without_scores:
            importance[modality] = float(np.mean(with_scores) - np.mean(without_scores))
        else:
            importance[modality] = 0.0
    total = sum(abs(v) for v in importance.values())
    if total > 0:
        importance = {k: v / total for k, v in importance.items()}
    return importance


def _fusion_of(model: nn.Module) -> Tuple[Optional[HybridFusion], bool]:
    """(the HybridFusion the fast path sweeps, whether `model` encodes first) or (None, False): any
    other module, and a HybridFusion beyond the sweep's limits, take the per-subset loop."""
    from harness import MultimodalFusionModel
    if type(model) is HybridFusion:
        fusion, encodes = model, False
    elif type(model) is MultimodalFusionModel and type(model.fusion_model) is HybridFusion:
        fusion, encodes = model.fusion_model, True
    else:
        return None, False
    return (fusion, encodes) if sweep_supported(fusion) else (None, False)


def evaluate_missing_modalities(model: nn.Module, dataloader, modality_names: Sequence[str],
                                device="cuda") -> Dict[str, Any]:
    """The reference's ``evaluate_missing_modalities`` (src/eval.py:312-374): accuracy and macro-F1
    under every non-empty modality subset -- ``full_modalities``, ``single_modalities`` (by name),
    ``all_combinations`` (by ``"+".join(names)``, in the reference's order) -- and
    ``modality_importance``.  Batches are ``(features, labels, mask)``; the batch's own mask is
    ignored, as in the reference.  The dataloader is walked once (batches outside, patterns inside);
    the predictions are counted on the device and read back once at the end.

    A ``harness.MultimodalFusionModel`` over this package's ``HybridFusion`` is encoded once per
    batch and swept (``hybrid_mask_sweep``); a ``HybridFusion`` takes the batch's features as the
    encoded ones.  Any other module is called once per subset on features zeroed as the reference
    zeroes them, its logits copied into a preallocated stack; both paths count with the same kernel."""
    names = list(modality_names)
    M = len(names)
    if M < 1:
        raise ValueError("evaluate_missing_modalities needs at least one modality name")
    model.eval()
    model.to(device)
    subsets = modality_subsets(M)
    S = len(subsets)
    patterns = [[1 if m in sub else 0 for m in range(M)] for sub in subsets]
    fusion, encodes = _fusion_of(model)
    if fusion is not None and fusion.num_modalities != M:
        fusion = None   # (the mask the reference would build has another width: let the model raise as it does there)
    counts: Optional[torch.Tensor] = None
    bad: Optional[torch.Tensor] = None
    stack: Optional[torch.Tensor] = None
    with torch.no_grad():
        for batch in dataloader:
            features, labels, _mask = batch
            features = {k: v.to(device) for k, v in features.items()}
            labels = labels.to(device=device, dtype=torch.int64).contiguous()
            B = labels.size(0)
            if fusion is not None:
                encoded = model.encode(features) if encodes else features
                logits = hybrid_mask_sweep(fusion, encoded, patterns)
            else:
                # the reference's loop (src/eval.py:394-408): features zeroed by POSITION in the batch's dict
                keys = list(features.keys())
                for s, sub in enumerate(subsets):
                    mask = torch.zeros(B, M, device=device)
                    mask[:, list(sub)] = 1
                    feats = {k: (v if i in sub else torch.zeros_like(v)) for i, (k, v) in enumerate(zip(keys, features.values()))}
                    out = model(feats, mask)
                    out = out[0] if isinstance(out, tuple) else out
                    if stack is None or stack.shape[1:] != out.shape:
                        stack = torch.empty((S,) + tuple(out.shape), dtype=torch.float32, device=out.device)
                    stack[s].copy_(out)
                assert stack is not None
                logits = stack
            _nat.require_device(logits, "missing-modality logits")
            if counts is None:
                C = logits.size(-1)
                counts = torch.zeros(S, C, C, dtype=torch.int64, device=logits.device)
                bad = torch.zeros(1, dtype=torch.int64, device=logits.device)
            torch.ops.mmfusion.confusion_accumulate(logits.contiguous(), labels.to(logits.device), counts, bad)
    if counts is None or bad is None:
        raise ValueError("evaluate_missing_modalities: the dataloader is empty")
    host = torch.cat([counts.reshape(-1), bad]).cpu()   # the one host read
    if int(host[-1]) != 0:
        raise ValueError(f"evaluate_missing_modalities: {int(host[-1])} label entries outside [0, {counts.size(1)})")
    per = host[:-1].reshape(counts.shape).numpy()
    results: Dict[str, Any] = {"full_modalities": {}, "single_modalities": {}, "all_combinations": {}}
    for s, sub in enumerate(subsets):
        metrics = metrics_from_confusion(per[s])
        results["all_combinations"]["+".join(names[i] for i in sub)] = metrics
        if len(sub) == 1:
            results["single_modalities"][names[sub[0]]] = metrics
        if len(sub) == M:
            results["full_modalities"] = metrics
    results["modality_importance"] = modality_importance(results, names)
    return results


# ============================================================================ standard evaluation
# the accumulate kernel's limits (include/mmfusion.h, mmf_eval_accumulate)
EVAL_MAX_CLASSES, EVAL_MAX_BINS, EVAL_MAX_BATCH = 1024, 256, 1 << 24


def metrics_from_state(words, num_classes: int, num_bins: int) -> Dict[str, Any]:
    """The evaluation state (include/mmfusion.h's layout, 8-byte words as an int64 array on the
    host) as metrics, in float64: ``accuracy``, ``f1_macro`` (``metrics_from_confusion``), ``loss``
    (the mean over calls of each call's mean cross-entropy, src/eval.py:84-86, 104), ``nll``
    (src/uncertainty.py:191), ``ece`` / ``mce`` (src/uncertainty.py:109-171: empty bins skipped, MCE 0
    when every bin is empty), ``num_samples``, ``confusion`` (C, C) int64, ``per_class_accuracy`` (C)
    and ``bins`` = {``count`` int64, ``accuracy``, ``confidence``} per bin (0 for an empty bin, as
    the reliability diagram draws it).  Raises ValueError when labels outside [0, C) were counted or
    the state holds no sample."""
    C, nb = int(num_classes), int(num_bins)
    w = np.ascontiguousarray(words.detach().cpu().numpy() if isinstance(words, torch.Tensor) else words, dtype=np.int64)
    head = _ops.EVAL_HEAD_WORDS
    if w.ndim != 1 or w.size != _ops.eval_state_words(C, nb):
        raise ValueError(f"the evaluation state of {C} classes and {nb} bins is {_ops.eval_state_words(C, nb)} words, "
                         f"got {w.shape}")
    f = w.view(np.float64)
    samples, correct, bad, calls = (int(v) for v in w[:4])
    if bad != 0:
        raise ValueError(f"evaluation: {bad} label entries outside [0, {C})")
    if samples == 0 or calls == 0:
        raise ValueError("evaluation: no samples were accumulated")
    confusion = w[head:head + C * C].reshape(C, C).copy()
    base = head + C * C
    count = w[base:base + nb].copy()
    bin_correct = w[base + nb:base + 2 * nb].astype(np.float64)
    conf_sum = f[base + 2 * nb:base + 3 * nb]
    filled = count > 0
    denom = np.where(filled, count, 1).astype(np.float64)
    bin_acc = np.where(filled, bin_correct / denom, 0.0)
    bin_conf = np.where(filled, conf_sum / denom, 0.0)
    gap = np.abs(bin_acc - bin_conf)
    support = confusion.sum(axis=1)
    per_class = np.where(support > 0, np.diag(confusion) / np.maximum(support, 1), 0.0)
    out: Dict[str, Any] = {"accuracy": correct / samples}
    out["f1_macro"] = metrics_from_confusion(confusion)["f1_macro"]
    out["loss"] = float(f[5]) / calls
    out["nll"] = float(f[6]) / samples
    out["ece"] = float(((count / samples) * gap)[filled].sum())
    out["mce"] = float(gap[filled].max()) if filled.any() else 0.0
    out["num_samples"] = samples
    out["confusion"] = confusion
    out["per_class_accuracy"] = per_class
    out["bins"] = {"count": count, "accuracy": bin_acc, "confidence": bin_conf}
    return out


class EvalAccumulator:
    """Accuracy / macro-F1 / loss / NLL / ECE / MCE of a stream of (logits, labels) batches,
    accumulated on the device: ``update`` is ``torch.ops.mmfusion.eval_accumulate`` (two launches, no
    host read) and ``result`` the one host read.  ``num_bins`` equal-width confidence bins between
    the float32 edges of ``torch.linspace(0, 1, num_bins + 1)``, the reference's
    (src/uncertainty.py:109)."""

    def __init__(self, num_classes: int, num_bins: int = 15, device="cuda"):
        C, nb = int(num_classes), int(num_bins)
        if not 1 <= C <= EVAL_MAX_CLASSES:
            raise ValueError(f"EvalAccumulator: num_classes {C} outside 1..{EVAL_MAX_CLASSES}")
        if not 1 <= nb <= EVAL_MAX_BINS:
            raise ValueError(f"EvalAccumulator: num_bins {nb} outside 1..{EVAL_MAX_BINS}")
        self.num_classes, self.num_bins = C, nb
        self.device = torch.device(device)
        self.edges = torch.linspace(0.0, 1.0, steps=nb + 1).to(self.device)   # (made on the host: the reference's bits)
        self.state = torch.zeros(_ops.eval_state_words(C, nb), dtype=torch.int64, device=self.device)

    def update(self, logits: torch.Tensor, labels: torch.Tensor, temperature=None, keep_predictions: bool = False):
        """Adds one batch: logits (B, C), labels (B).  ``temperature`` (a float or a one-element
        tensor) divides the logits on the device.  With ``keep_predictions`` returns the batch's
        (predictions int64 (B), confidences float32 (B)) on the device."""
        _nat.require_device(logits, "evaluation logits")
        if logits.dim() != 2 or logits.size(1) != self.num_classes:
            raise ValueError(f"EvalAccumulator: logits are (B, {self.num_classes}), got {tuple(logits.shape)}")
        if logits.size(0) > EVAL_MAX_BATCH:
            raise ValueError(f"EvalAccumulator: a batch of {logits.size(0)} rows is over {EVAL_MAX_BATCH}")
        dev = logits.device
        if dev != self.state.device:
            raise ValueError(f"EvalAccumulator: the state is on {self.state.device}, the logits on {dev}")
        logits = _nat.f32c(logits.detach())
        labels = labels.detach().to(device=dev, dtype=torch.int64).reshape(-1).contiguous()
        if labels.numel() != logits.size(0):
            raise ValueError(f"EvalAccumulator: {labels.numel()} labels for {logits.size(0)} rows")
        if temperature is not None:
            temperature = torch.as_tensor(temperature, dtype=torch.float32).detach().reshape(-1).to(dev).contiguous()
            if temperature.numel() != 1:
                raise ValueError("EvalAccumulator: the temperature is one number")
        preds = conf = None
        if keep_predictions:
            preds = torch.empty(logits.size(0), dtype=torch.int64, device=dev)
            conf = torch.empty(logits.size(0), dtype=torch.float32, device=dev)
        torch.ops.mmfusion.eval_accumulate(logits, labels, self.edges, temperature, self.state, preds, conf)
        return (preds, conf) if keep_predictions else None

    def result(self) -> Dict[str, Any]:
        """``metrics_from_state`` of the state: the one host read."""
        return metrics_from_state(self.state.cpu(), self.num_classes, self.num_bins)


def _evaluate(model: nn.Module, dataloader, device, num_bins: int, temperature, keep: bool, keep_logits: bool):
    """The walk of src/eval.py:60-100 -> (EvalAccumulator.result(), predictions tuple or None)."""
    model.eval()
    model.to(device)
    acc: Optional[EvalAccumulator] = None
    preds_l: List[torch.Tensor] = []
    conf_l: List[torch.Tensor] = []
    labels_l: List[torch.Tensor] = []
    logits_l: List[torch.Tensor] = []
    with torch.no_grad():
        for batch in dataloader:
            features, labels, mask = batch
            features = {k: v.to(device) for k, v in features.items()}
            labels = labels.to(device)
            mask = mask.to(device)
            out = model(features, mask)
            logits = out[0] if isinstance(out, tuple) else out   # (LateFusion: (logits, per-modality logits))
            _nat.require_device(logits, "evaluation logits")
            logits = _nat.f32c(logits.detach())
            if acc is None:
                acc = EvalAccumulator(logits.size(-1), num_bins, logits.device)
            kept = acc.update(logits, labels, temperature, keep_predictions=keep)
            if keep:
                preds_l.append(kept[0])
                conf_l.append(kept[1])
                labels_l.append(labels.to(logits.device))
                if keep_logits:
                    logits_l.append(logits)
    if acc is None:
        raise ValueError("evaluate_model: the dataloader is empty")
    result = acc.result()   # the one host read of the metrics
    predictions = None
    if keep:
        predictions = (torch.cat(preds_l).cpu(), torch.cat(labels_l).cpu(), torch.cat(conf_l).cpu())
        if keep_logits:
            predictions = (*predictions, torch.cat(logits_l).cpu())
    return result, predictions


_METRIC_KEYS = ("accuracy", "f1_macro", "loss", "num_samples", "ece", "mce", "nll")


def evaluate_model(model: nn.Module, dataloader, device="cuda", return_predictions: bool = False,
                   include_logits: bool = False, num_bins: int = 15, temperature=None):
    """The reference's ``evaluate_model`` (src/eval.py:39-130) with the ``CalibrationMetrics`` chain
    over its output (src/uncertainty.py:84-192) folded in: -> ``{"accuracy", "f1_macro", "loss",
    "num_samples", "ece", "mce", "nll"}``, and with ``return_predictions`` also ``(preds, labels,
    confidences[, logits])`` as CPU tensors, each copied once after the last batch.  Batches are
    ``(features, labels, mask)``; a model that returns a tuple contributes its first element.  Every
    statistic is accumulated on the device (``EvalAccumulator``) and read back once; ``temperature``
    divides the logits first (temperature scaling, src/uncertainty.py:431-435).  ``loss`` is the mean
    over batches of each batch's mean cross-entropy, ``nll`` the mean over samples, as in the
    reference.  An empty dataloader raises ValueError (the reference fails in ``torch.cat``)."""
    result, predictions = _evaluate(model, dataloader, device, num_bins, temperature, return_predictions,
                                    return_predictions and include_logits)
    metrics = {k: result[k] for k in _METRIC_KEYS}
    return (metrics, predictions) if return_predictions else metrics


# ------------------------------------------------------------------ latency (src/eval.py:133-228)
def _parse_latency_batch(batch: Any):
    """(features, labels, mask) of a mapping or of a sequence that starts with one, else None."""
    if isinstance(batch, Mapping):
        return dict(batch), None, None
    if isinstance(batch, _SequenceABC) and batch:
        first = batch[0]
        if isinstance(first, Mapping):
            return dict(first), (batch[1] if len(batch) > 1 else None), (batch[2] if len(batch) > 2 else None)
    return None


def _infer_batch_size(labels: Any, features) -> Optional[int]:
    if hasattr(labels, "shape"):
        return int(labels.shape[0])
    for tensor in features.values():
        if hasattr(tensor, "shape"):
            return int(tensor.shape[0])
    return None


def measure_inference_latency(model: nn.Module, dataloader, device="cuda", warmup: int = 1) -> Tuple[float, float]:
    """Per-sample inference latency (mean, std over batches, in ms) as the reference's
    ``measure_inference_latency`` (src/eval.py:166-228) parses, skips and warns, but timed with a
    pair of device events around the model call: the call only enqueues work, so ``perf_counter``
    around it would time the launches.  The events are read after the last batch (one
    synchronisation).  Each of the first ``warmup`` usable batches is run once untimed before its
    timed run (kernel loading and the allocator's first blocks are no part of the latency).
    ``(0.0, 0.0)`` when no batch could be timed."""
    model.eval()
    model.to(device)
    timed: List[Tuple[Any, Any, int]] = []
    warmed = 0
    with torch.no_grad():
        for batch in dataloader:
            parsed = _parse_latency_batch(batch)
            if parsed is None:
                print("  Warning: Unable to parse batch for latency measurement, skipping.")
                continue
            features, labels, mask = parsed
            batch_size = _infer_batch_size(labels, features)
            if batch_size is None or batch_size == 0:
                print("  Warning: Unable to infer batch size for latency measurement, skipping.")
                continue
            if not features:
                print("  Warning: Empty feature dict encountered during latency measurement, skipping.")
                continue
            try:
                features = {k: v.to(device) for k, v in features.items()}
            except AttributeError:
                print("  Warning: Non-tensor feature encountered, skipping batch for latency measurement.")
                continue
            if mask is None:
                mask = torch.ones(batch_size, max(1, len(features)), device=device,
                                  dtype=next(iter(features.values())).dtype)
            else:
                mask = mask.to(device)
            try:
                if warmed < warmup:
                    model(features, mask)
                    warmed += 1
                start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                model(features, mask)
                end.record()
            except TypeError:
                print("  Warning: Model call failed during latency measurement, skipping batch.")
                continue
            timed.append((start, end, batch_size))
    if not timed:
        return 0.0, 0.0
    timed[-1][1].synchronize()
    arr = np.asarray([s.elapsed_time(e) / n for s, e, n in timed], dtype=np.float64)
    return float(arr.mean()), float(arr.std(ddof=0))


# ------------------------------------------------------------------ plots (src/eval.py:231-309, src/uncertainty.py:195-283)
def _figure(figsize):
    """A figure on the Agg canvas, without touching pyplot's global backend."""
    from matplotlib.backends.backend_agg import FigureCanvasAgg
    from matplotlib.figure import Figure
    fig = Figure(figsize=figsize)
    FigureCanvasAgg(fig)
    return fig, fig.add_subplot(111)


def attention_matrix(model: nn.Module, features: Dict[str, torch.Tensor], mask: torch.Tensor,
                     modality_names: Sequence[str]) -> Optional[np.ndarray]:
    """The (M, M) float32 matrix of src/eval.py:256-291: entry [q, k] is the mean of the attention
    map ``"<q>_to_<k>"`` that ``model(features, mask, return_attention=True)`` returns (0 where
    there is none).  The per-pair means are taken on the device and read back together.  None in the
    reference's cases: no names, a model that raises ValueError / TypeError, no attention maps."""
    names = list(modality_names)
    if not names:
        return None
    with torch.no_grad():
        try:
            _, info = model(features, mask, return_attention=True)
        except (ValueError, TypeError):
            return None
    maps = info.get("attention_maps", {}) if isinstance(info, Mapping) else {}
    if not maps:
        return None
    cells, means = [], []
    for key, weights in maps.items():
        if "_to_" not in key:
            continue
        query_mod, key_mod = key.split("_to_", 1)
        if query_mod not in names or key_mod not in names:
            continue
        cells.append((names.index(query_mod), names.index(key_mod)))
        means.append(weights.detach().float().mean())
    matrix = np.zeros((len(names), len(names)), dtype=np.float32)
    counts = np.zeros_like(matrix)
    if means:
        host = torch.stack(means).cpu().numpy()   # the one host read
        for (q, k), v in zip(cells, host):
            matrix[q, k] += v
            counts[q, k] += 1
    return np.divide(matrix, np.where(counts == 0, 1.0, counts), out=np.zeros_like(matrix), where=counts != 0)


def _is_hybrid(model: nn.Module) -> bool:
    return isinstance(model, HybridFusion) or isinstance(getattr(model, "fusion_model", None), HybridFusion)


def generate_attention_visualization(model: nn.Module, dataloader, modality_names: Sequence[str], save_path,
                                     device="cuda") -> Optional[Path]:
    """The reference's cross-modal attention heat map (src/eval.py:231-309) of the dataloader's first
    batch, saved to ``save_path``; None when there is nothing to draw: no names, a model without a
    ``HybridFusion`` (the reference asks its config for ``fusion_type == "hybrid"``), an empty
    dataloader, or ``attention_matrix`` returning None."""
    names = list(modality_names)
    if not names or not _is_hybrid(model):
        return None
    try:
        features, _, mask = next(iter(dataloader))
    except StopIteration:
        return None
    features = {k: v.to(device) for k, v in features.items()}
    matrix = attention_matrix(model, features, mask.to(device), names)
    if matrix is None:
        return None
    fig, ax = _figure((6, 5))
    im = ax.imshow(matrix, cmap="magma", aspect="equal")
    ax.set_xticks(range(len(names)))
    ax.set_yticks(range(len(names)))
    ax.set_xticklabels(names, rotation=45, ha="right")
    ax.set_yticklabels(names)
    ax.set_xlabel("Key Modality")
    ax.set_ylabel("Query Modality")
    ax.set_title("Cross-Modal Attention Heatmap")
    fig.colorbar(im, ax=ax, shrink=0.8)
    save_path = Path(save_path)
    save_path.parent.mkdir(parents=True, exist_ok=True)
    fig.tight_layout()
    fig.savefig(save_path, dpi=300)
    return save_path


def reliability_diagram(bins: Dict[str, Any], save_path) -> Path:
    """The reference's reliability diagram (src/uncertainty.py:195-283) from accumulated bins
    (``EvalAccumulator.result()["bins"]``): one bar per bin at its accuracy, the diagonal, and the
    ECE of the bins in the corner."""
    count = np.asarray(bins["count"], dtype=np.float64)
    accuracy = np.asarray(bins["accuracy"], dtype=np.float64)
    confidence = np.asarray(bins["confidence"], dtype=np.float64)
    nb = count.size
    if nb < 1 or accuracy.shape != (nb,) or confidence.shape != (nb,):
        raise ValueError("reliability_diagram: bins holds count, accuracy and confidence of one length")
    edges = np.linspace(0.0, 1.0, nb + 1)
    centers = (edges[:-1] + edges[1:]) / 2
    total = count.sum()
    ece = float((count / total * np.abs(accuracy - confidence))[count > 0].sum()) if total > 0 else 0.0
    fig, ax = _figure((6, 5))
    ax.bar(centers, accuracy, width=1.0 / nb, alpha=0.7, edgecolor="black", label="Accuracy")
    ax.plot([0, 1], [0, 1], "--", color="gray", label="Perfect Calibration")
    ax.set_xlim(0, 1)
    ax.set_ylim(0, 1)
    ax.set_xlabel("Confidence")
    ax.set_ylabel("Accuracy")
    ax.set_title("Reliability Diagram")
    ax.text(0.02, 0.95, f"ECE: {ece:.3f}", transform=ax.transAxes, fontsize=10, verticalalignment="top")
    ax.legend(loc="lower right")
    fig.tight_layout()
    save_path = Path(save_path)
    save_path.parent.mkdir(parents=True, exist_ok=True)
    fig.savefig(save_path, dpi=300, bbox_inches="tight")
    return save_path


def save_results_json(results: Dict[str, Any], output_path) -> Path:
    """src/eval.py:461-469."""
    output_path = Path(output_path)
    output_path.parent.mkdir(parents=True, exist_ok=True)
    with open(output_path, "w") as f:
        json.dump(results, f, indent=2)
    return output_path


def _fusion_type(model: nn.Module) -> str:
    fusion = getattr(model, "fusion_model", model)
    name = type(fusion).__name__
    return name[:-len("Fusion")].lower() if name.endswith("Fusion") and len(name) > len("Fusion") else name


def standard_evaluation(model: nn.Module, dataloader, modality_names: Sequence[str], num_bins: int = 15,
                        output_dir=None, dataset_name: Optional[str] = None, fusion_type: Optional[str] = None,
                        device="cuda") -> Tuple[Dict[str, Any], Dict[str, Any]]:
    """The reference's "Standard Evaluation" section (src/eval.py:534-611, 642-656) ->
    ``(standard_results, uncertainty_results)`` with the reference's keys: ``evaluate_model`` with the
    calibration metrics, the reliability diagram, the attention heat map of a hybrid model and the
    inference latency.  With ``output_dir`` the plots go to ``calibration.png`` / ``attention_viz.png``
    there and the dicts to ``evaluation_results.json`` / ``uncertainty.json``; without it nothing is
    written and ``calibration_plot`` is None.  ``fusion_type`` defaults to the fusion module's
    (``"hybrid"`` for ``HybridFusion``).  ECE and MCE use ``num_bins`` (the reference scores them with
    15 bins whatever ``evaluation.num_calibration_bins`` says and uses the setting for the plot alone)."""
    fusion_type = _fusion_type(model) if fusion_type is None else str(fusion_type)
    result, _ = _evaluate(model, dataloader, device, num_bins, None, False, False)
    out_dir = None if output_dir is None else Path(output_dir)
    calibration_plot = attention_plot = None
    if out_dir is not None:
        calibration_plot = reliability_diagram(result["bins"], out_dir / "calibration.png")
        if fusion_type == "hybrid":
            attention_plot = generate_attention_visualization(model, dataloader, list(modality_names),
                                                              out_dir / "attention_viz.png", device)
    latency_mean_ms, latency_std_ms = measure_inference_latency(model, dataloader, device)
    standard_results: Dict[str, Any] = {
        "dataset": dataset_name,
        "fusion_type": fusion_type,
        "test_accuracy": result["accuracy"],
        "test_f1_macro": result["f1_macro"],
        "test_loss": result["loss"],
        "ece": result["ece"],
        "mce": result["mce"],
        "nll": result["nll"],
        "inference_ms_mean": latency_mean_ms,
        "inference_ms_std": latency_std_ms,
    }
    if attention_plot is not None:
        standard_results["attention_plot"] = str(attention_plot)
    uncertainty_results: Dict[str, Any] = {
        "dataset": dataset_name,
        "fusion_type": fusion_type,
        "ece": result["ece"],
        "mce": result["mce"],
        "nll": result["nll"],
        "num_bins": int(num_bins),
        "calibration_plot": None if calibration_plot is None else str(calibration_plot),
    }
    if out_dir is not None:
        save_results_json(standard_results, out_dir / "evaluation_results.json")
        save_results_json(uncertainty_results, out_dir / "uncertainty.json")
    return standard_results, uncertainty_results
