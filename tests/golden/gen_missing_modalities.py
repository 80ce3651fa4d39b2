"""Generate the missing-modality parity fixture from the REFERENCE's HybridFusion on the CPU.

Generation-time tool (never run by a test): it imports ``fusion`` from the reference checkout given
with ``--reference`` (nothing of it is copied) and writes ``missing_modalities_ref.npz`` next to this
file.  Only inputs and recorded results are stored.

The reference's ``src/eval.py`` needs omegaconf and Lightning to import, so the walk over the
subsets of its ``evaluate_missing_modalities`` (src/eval.py:342-424) is made here: for every
``itertools.combinations`` subset by size 1..M, per batch a 0/1 mask column per available modality,
the other modalities' features replaced by zeros, ``argmax`` of ``model(features, mask)``, then
accuracy and ``sklearn.metrics.f1_score(average="macro", zero_division=0)`` over all batches, and the
importance of src/eval.py:427-458 (mean accuracy of the combinations whose name contains the
modality's name minus the mean of the others, normalised by the sum of absolute values).

Case: modalities imu_hand, imu_chest, imu_ankle, heart_rate, encoded dim 32, hidden 32, 4 heads,
7 classes, the reference module's own initial parameters under SEED, 40 samples in batches of
16 / 16 / 8.  Labels: the full-modality argmax with a quarter of them redrawn.

Margin: every stored row's top-2 logit gap is at least MARGIN = 1e-2 of max|logits| (ten times the
fp32 parity bound 1e-3), under every subset, so a device within the bound cannot legitimately
predict another class.  An untrained model's logits are close together, so the 40 samples are the
first of CANDIDATES seeded draws that meet the margin under every subset (against the largest
|logit| of ALL candidates, which is at least that of the kept ones).

Accuracy is stored as the float64 ratio correct / N; the reference's ``.float().mean()`` rounds the
same ratio to float32 (asserted here to agree within 1e-7).

Run:  python tests/golden/gen_missing_modalities.py --reference <path to the reference checkout>
"""

from __future__ import annotations

import argparse
import itertools
import sys
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
NAMES = ["imu_hand", "imu_chest", "imu_ankle", "heart_rate"]
DIM, HIDDEN, HEADS, CLASSES = 32, 32, 4, 7
N, BATCHES = 40, (16, 16, 8)
SEED, CANDIDATES, MARGIN = 2026, 400, 1e-2


def subset_logits(model, feats, subset):
    """One batch under one subset, as src/eval.py:394-407."""
    B = next(iter(feats.values())).size(0)
    mask = torch.zeros(B, len(NAMES))
    for idx in subset:
        mask[:, idx] = 1
    feats = dict(feats)
    for i, name in enumerate(list(feats.keys())):
        if i not in subset:
            feats[name] = torch.zeros_like(feats[name])
    return model(feats, mask)


def top2_gap(logits: torch.Tensor) -> torch.Tensor:
    top = logits.topk(2, dim=-1).values
    return top[..., 0] - top[..., 1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference checkout (holds src/fusion.py)")
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.reference) / "src"))
    import fusion as ref_fusion
    from sklearn.metrics import f1_score

    torch.set_num_threads(1)
    torch.manual_seed(SEED)
    model = ref_fusion.HybridFusion({n: DIM for n in NAMES}, hidden_dim=HIDDEN, num_classes=CLASSES, num_heads=HEADS,
                                    dropout=0.1).eval()
    M = len(NAMES)
    subsets = [s for k in range(1, M + 1) for s in itertools.combinations(range(M), k)]
    rng = np.random.default_rng(SEED)
    cand = {n: torch.from_numpy(rng.standard_normal((CANDIDATES, DIM)).astype(np.float32)) for n in NAMES}
    with torch.no_grad():
        all_logits = torch.stack([subset_logits(model, cand, s) for s in subsets])   # (15, CANDIDATES, 7)
    floor = MARGIN * float(all_logits.abs().max())
    ok = (top2_gap(all_logits) >= 1.5 * floor).all(dim=0)   # (1.5: room for the batched re-evaluation's rounding)
    keep = torch.nonzero(ok).flatten()[:N]
    assert keep.numel() == N, f"only {int(ok.sum())} of {CANDIDATES} candidates meet the margin"
    feats = {n: cand[n][keep].contiguous() for n in NAMES}

    # the reference's walk: subsets outside, batches inside
    edges = np.cumsum((0,) + BATCHES)
    logits = torch.empty(len(subsets), N, CLASSES)
    with torch.no_grad():
        for si, s in enumerate(subsets):
            for lo, hi in zip(edges[:-1], edges[1:]):
                logits[si, lo:hi] = subset_logits(model, {n: v[lo:hi] for n, v in feats.items()}, s)
    assert float(top2_gap(logits).min()) >= MARGIN * float(logits.abs().max()), "margin lost"

    labels = logits[-1].argmax(dim=1).numpy().astype(np.int64)
    redraw = rng.random(N) < 0.25
    labels = np.where(redraw, rng.integers(0, CLASSES, size=N), labels).astype(np.int64)

    names, acc, f1 = [], [], []
    for si, s in enumerate(subsets):
        preds = logits[si].argmax(dim=1)
        a32 = (preds == torch.from_numpy(labels)).float().mean().item()
        a = float((preds.numpy() == labels).sum()) / N
        assert abs(a - a32) < 1e-7
        names.append("+".join(NAMES[i] for i in s))
        acc.append(a)
        f1.append(float(f1_score(labels, preds.numpy(), average="macro", zero_division=0)))
    importance = {}
    for m in NAMES:
        w = [a for n, a in zip(names, acc) if m in n]
        wo = [a for n, a in zip(names, acc) if m not in n]
        importance[m] = float(np.mean(w) - np.mean(wo)) if w and wo else 0.0
    total = sum(abs(v) for v in importance.values())
    if total > 0:
        importance = {k: v / total for k, v in importance.items()}

    out = {f"sd/{k}": v.detach().numpy() for k, v in model.state_dict().items()}
    out.update({f"x/{n}": feats[n].numpy() for n in NAMES})
    out.update({"labels": labels, "modality_names": np.asarray(NAMES), "subset_names": np.asarray(names),
                "batches": np.asarray(BATCHES, np.int64), "logits": logits.numpy(),
                "accuracy": np.asarray(acc, np.float64), "f1_macro": np.asarray(f1, np.float64),
                "importance": np.asarray([importance[m] for m in NAMES], np.float64),
                "dims": np.asarray([DIM, HIDDEN, HEADS, CLASSES], np.int64)})
    np.savez_compressed(HERE / "missing_modalities_ref.npz", **out)
    print(f"wrote missing_modalities_ref.npz: accuracy full {acc[-1]:.4f}, min {min(acc):.4f}; "
          f"min gap / max|logit| {float(top2_gap(logits).min()) / float(logits.abs().max()):.4f}")


if __name__ == "__main__":
    main()
