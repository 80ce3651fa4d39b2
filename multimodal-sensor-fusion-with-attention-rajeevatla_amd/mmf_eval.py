"""Missing-modality robustness evaluation (src/eval.py:312-458) on the HIP path.

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

This is a separate module name (not ``eval``) so that the reference's own ``eval`` keeps resolving
under ``mmf_launch``, for the reason ``calibration.py`` gives.
"""

from __future__ import annotations

import itertools
import os
import sys
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
