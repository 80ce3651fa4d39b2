"""Helpers of the missing-modality sweep tests: the shape cases, every 0/1 pattern, the float64
oracle per pattern (computed once per case and shared), the model builders and the fixture."""
from __future__ import annotations

import functools
import itertools
from typing import Dict, List, Tuple

import numpy as np
import torch

from _util import load_fixture
from cases import HybridCase, hybrid_inputs, hybrid_state

# name: (case, what it reaches).  Smallest shapes that reach the edges of the sweep's kernels.
CASES: Dict[str, HybridCase] = {c.name: c for c in [
    # 80 rows (16 patterns x 5 samples), the single-key plan
    HybridCase("m4_2d", ["a", "b", "c", "d"], {"a": 12, "b": 20, "c": 16, "d": 8}, {"a": 0, "b": 0, "c": 0, "d": 0},
               batch=5, hidden=32, heads=4, classes=7, seed=101),
    # mixed key lengths, PAMAP2's class count
    HybridCase("m3_mixed_l", ["a", "b", "c"], {"a": 12, "b": 20, "c": 16}, {"a": 5, "b": 1, "c": 9},
               batch=3, hidden=64, heads=4, classes=25, seed=102),
    # 288 rows: several tail tiles with a ragged last one
    HybridCase("m5_2d", ["a", "b", "c", "d", "e"], {"a": 12, "b": 20, "c": 16, "d": 8, "e": 24},
               {"a": 0, "b": 0, "c": 0, "d": 0, "e": 0}, batch=9, hidden=64, heads=4, classes=11, seed=103),
    # long keys, H at the tail's upper size
    HybridCase("m3_long", ["a", "b", "c"], {"a": 12, "b": 20, "c": 16}, {"a": 130, "b": 130, "c": 130},
               batch=2, hidden=256, heads=4, classes=5, seed=104),
    # head_dim > 64
    HybridCase("m2_wide", ["a", "b"], {"a": 12, "b": 20}, {"a": 4, "b": 4},
               batch=3, hidden=256, heads=1, classes=5, seed=105),
    # 16 heads: the general (non-pooled) plan -- attended rows (B, Lq, H) pooled by the sweep, and the
    # 2-D query's (B, 1, H) rows read in place
    HybridCase("m3_general", ["a", "b", "c"], {"a": 12, "b": 20, "c": 16}, {"a": 5, "b": 0, "c": 3},
               batch=3, hidden=128, heads=16, classes=5, seed=107),
    # L a multiple of 128 under the pooled plan: the L-mean of P_m from the projection's column sums
    HybridCase("m2_l128", ["a", "b"], {"a": 12, "b": 20}, {"a": 128, "b": 256},
               batch=2, hidden=32, heads=4, classes=3, seed=108),
    # a query with fewer pairs than the others
    HybridCase("m3_deleted", ["a", "b", "c"], {"a": 12, "b": 20, "c": 16}, {"a": 0, "b": 0, "c": 0},
               batch=4, hidden=32, heads=4, classes=6, seed=106, deleted=["b_to_a"]),
]}
WEIGHT_CASES = ("m4_2d", "m3_mixed_l")


def all_patterns(num_modalities: int) -> List[Tuple[int, ...]]:
    """Every 0/1 pattern, the all-zero one first."""
    return list(itertools.product((0, 1), repeat=num_modalities))


def case_inputs(case: HybridCase) -> Dict[str, torch.Tensor]:
    feats, _, _ = hybrid_inputs(case)
    return {m: torch.from_numpy(v) for m, v in feats.items()}


@functools.lru_cache(maxsize=None)
def oracle_sweep(name: str):
    """(logits (S, B, C), fusion weights (S, B, M)) of oracle/hybrid_cpu.py in float64 under every
    pattern, the absent modalities' features zeroed as the reference zeroes them.  Cached: the tests
    share it and must not modify it."""
    from oracle.hybrid_cpu import hybrid_forward
    case = CASES[name]
    sd = hybrid_state(case.names, case.dims, case.hidden, case.classes, case.seed, case.deleted)
    params = {k: torch.from_numpy(v).double() for k, v in sd.items()}
    feats = {m: v.double() for m, v in case_inputs(case).items()}
    logits, weights = [], []
    with torch.no_grad():
        for pat in all_patterns(len(case.names)):
            mask = torch.tensor(pat, dtype=torch.float64).repeat(case.batch, 1)
            x = {m: (v if pat[i] else torch.zeros_like(v)) for i, (m, v) in enumerate(feats.items())}
            lg, info = hybrid_forward(params, case.names, x, mask, case.heads)
            logits.append(lg)
            weights.append(info["fusion_weights"])
    return torch.stack(logits), torch.stack(weights)


def build_hybrid(fusion, case: HybridCase, dev="cuda"):
    model = fusion.HybridFusion({m: case.dims[m] for m in case.names}, hidden_dim=case.hidden,
                                num_classes=case.classes, num_heads=case.heads, dropout=0.1)
    for key in case.deleted:
        del model.attention_modules[key]
    sd = hybrid_state(case.names, case.dims, case.hidden, case.classes, case.seed, case.deleted)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return model.to(dev).eval()


@functools.lru_cache(maxsize=None)
def fixture():
    return load_fixture("missing_modalities_ref")


def fixture_names(fx) -> List[str]:
    return [str(n) for n in fx["modality_names"]]


def fixture_model(fusion, fx, dev="cuda"):
    dim, hidden, heads, classes = (int(v) for v in fx["dims"])
    model = fusion.HybridFusion({n: dim for n in fixture_names(fx)}, hidden_dim=hidden, num_classes=classes,
                                num_heads=heads, dropout=0.1)
    model.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("sd/")}, strict=True)
    return model.to(dev).eval()


def fixture_batches(fx, dev="cpu"):
    """The fixture's samples as (features, labels, mask) batches of its recorded sizes."""
    names = fixture_names(fx)
    lo = 0
    out = []
    for n in (int(v) for v in fx["batches"]):
        feats = {m: torch.from_numpy(fx[f"x/{m}"][lo:lo + n]).to(dev) for m in names}
        out.append((feats, torch.from_numpy(fx["labels"][lo:lo + n]).to(dev), torch.ones(n, len(names), device=dev)))
        lo += n
    return out


def confusion_of(logits: np.ndarray, labels: np.ndarray) -> np.ndarray:
    """(S, C, C) counts[s, label, argmax] on the host."""
    S, _, C = logits.shape
    counts = np.zeros((S, C, C), np.int64)
    for s in range(S):
        np.add.at(counts[s], (labels, logits[s].argmax(axis=1)), 1)
    return counts


def top2_margin(logits) -> float:
    """The smallest top-2 gap of any row over max|logits|."""
    t = torch.as_tensor(logits).double()
    top = t.topk(2, dim=-1).values
    return float((top[..., 0] - top[..., 1]).min() / t.abs().max())
