"""Generate the standard-evaluation parity fixture from the REFERENCE's HybridFusion and
CalibrationMetrics on the CPU.

Generation-time tool (never run by a test): it imports ``fusion`` and ``uncertainty`` from the
reference checkout given with ``--reference`` (nothing of them is copied) and writes
``eval_metrics_ref.npz`` next to this file.  Only inputs and recorded results are stored.

The reference's ``src/eval.py`` needs omegaconf and Lightning to import, so the walk of its
``evaluate_model`` (src/eval.py:70-104) is made here: per batch ``logits = model(features, mask)``,
``F.cross_entropy(logits, labels).item()`` summed and divided by the number of batches, ``softmax``
and ``torch.max`` for the confidences and predictions; then accuracy,
``sklearn.metrics.f1_score(average="macro", zero_division=0)`` and the reference's own
``CalibrationMetrics.expected_calibration_error`` / ``maximum_calibration_error`` (15 bins) /
``negative_log_likelihood`` over the concatenated tensors, as src/eval.py:552-558 calls them.

Case: modalities imu_hand, imu_chest, imu_ankle, heart_rate, encoded dim 32, hidden 32, 4 heads,
7 classes, the reference module's own initial parameters under SEED with ``classifier.3.weight``
multiplied by SPREAD (an untrained model's logits are close together: every confidence would sit
near 1 / 7 in one bin), 40 samples in batches of 16 / 16 / 8.  Labels: the argmax with 40 % redrawn.

Margins, asserted here and again by tests/test_gpu_eval_metrics.py: every row's top-2 logit gap is
at least 1e-2 of max|logits| and every confidence at least 1e-3 of max|logits| from every bin edge
(ten times / once the fp32 parity bound 1e-3 on the logits: d conf <= d z / 2, so a device within
the bound predicts the same class and fills the same bin); at least 5 bins are populated and at
least 3 of them hold both right and wrong predictions.  The 40 samples are the first of CANDIDATES
seeded draws that meet 1.5 times the two margins.

Accuracy is stored as the float64 ratio correct / N; the reference's ``.float().mean()`` rounds the
same ratio to float32 (asserted here to agree within 1e-7).

Run:  python tests/golden/gen_eval_metrics.py --reference <path to the reference checkout>
"""

from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
NAMES = ["imu_hand", "imu_chest", "imu_ankle", "heart_rate"]
DIM, HIDDEN, HEADS, CLASSES = 32, 32, 4, 7
N, BATCHES, BINS = 40, (16, 16, 8), 15
SEED, CANDIDATES, SPREAD = 2027, 400, 100.0
GAP, EDGE = 1e-2, 1e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference checkout (holds src/fusion.py)")
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.reference) / "src"))
    import fusion as ref_fusion
    from sklearn.metrics import f1_score
    from uncertainty import CalibrationMetrics

    from _evalmetrics import edges64, fixture_margins

    torch.set_num_threads(1)
    torch.manual_seed(SEED)
    model = ref_fusion.HybridFusion({n: DIM for n in NAMES}, hidden_dim=HIDDEN, num_classes=CLASSES, num_heads=HEADS,
                                    dropout=0.1).eval()
    with torch.no_grad():
        model.classifier[3].weight.mul_(SPREAD)
    M = len(NAMES)
    rng = np.random.default_rng(SEED)
    cand = {n: torch.from_numpy(rng.standard_normal((CANDIDATES, DIM)).astype(np.float32)) for n in NAMES}
    with torch.no_grad():
        lg = model(cand, torch.ones(CANDIDATES, M)).double()
    scale = float(lg.abs().max())
    top = lg.topk(2, dim=1).values
    conf = torch.softmax(lg, dim=1).max(dim=1).values.numpy()
    edge_dist = np.abs(conf[:, None] - edges64(BINS)[None, :]).min(axis=1)
    ok = ((top[:, 0] - top[:, 1]).numpy() >= 1.5 * GAP * scale) & (edge_dist >= 1.5 * EDGE * scale)
    keep = np.flatnonzero(ok)[:N]
    assert keep.size == N, f"only {int(ok.sum())} of {CANDIDATES} candidates meet the margins"
    feats = {n: cand[n][keep].contiguous() for n in NAMES}

    # the reference's walk (src/eval.py:70-104)
    bounds = np.cumsum((0,) + BATCHES)
    all_logits, all_preds, all_conf = [], [], []
    with torch.no_grad():
        for lo, hi in zip(bounds[:-1], bounds[1:]):
            all_logits.append(model({n: v[lo:hi] for n, v in feats.items()}, torch.ones(hi - lo, M)))
    logits = torch.cat(all_logits)
    labels = logits.argmax(dim=1).numpy().astype(np.int64)
    redraw = rng.random(N) < 0.4
    labels = np.where(redraw, rng.integers(0, CLASSES, size=N), labels).astype(np.int64)
    labels_t = torch.from_numpy(labels)
    total_loss, num_batches = 0.0, 0
    for lo, hi, lgb in zip(bounds[:-1], bounds[1:], all_logits):
        total_loss += F.cross_entropy(lgb, labels_t[lo:hi]).item()
        num_batches += 1
        confidences, preds = torch.max(F.softmax(lgb, dim=1), dim=1)
        all_preds.append(preds)
        all_conf.append(confidences)
    preds, confidences = torch.cat(all_preds), torch.cat(all_conf)
    a32 = (preds == labels_t).float().mean().item()
    accuracy = float((preds.numpy() == labels).sum()) / N
    assert abs(accuracy - a32) < 1e-7
    f1 = float(f1_score(labels, preds.numpy(), average="macro", zero_division=0))
    ece = CalibrationMetrics.expected_calibration_error(confidences, preds, labels_t, num_bins=BINS)
    mce = CalibrationMetrics.maximum_calibration_error(confidences, preds, labels_t, num_bins=BINS)
    nll = CalibrationMetrics.negative_log_likelihood(logits, labels_t)

    m = fixture_margins(logits.numpy(), labels, BINS)
    assert m["gap"] >= GAP and m["edge"] >= EDGE, m
    assert m["populated"] >= 5 and m["mixed"] >= 3, m

    out = {f"sd/{k}": v.detach().numpy() for k, v in model.state_dict().items()}
    out.update({f"x/{n}": feats[n].numpy() for n in NAMES})
    out.update({"labels": labels, "modality_names": np.asarray(NAMES), "batches": np.asarray(BATCHES, np.int64),
                "logits": logits.numpy(), "preds": preds.numpy().astype(np.int64),
                "confidences": confidences.numpy(), "num_bins": np.asarray([BINS], np.int64),
                "accuracy": np.asarray([accuracy], np.float64), "f1_macro": np.asarray([f1], np.float64),
                "loss": np.asarray([total_loss / num_batches], np.float64), "ece": np.asarray([ece], np.float64),
                "mce": np.asarray([mce], np.float64), "nll": np.asarray([nll], np.float64),
                "dims": np.asarray([DIM, HIDDEN, HEADS, CLASSES], np.int64)})
    np.savez_compressed(HERE / "eval_metrics_ref.npz", **out)
    print(f"wrote eval_metrics_ref.npz: accuracy {accuracy:.4f}, f1 {f1:.4f}, loss {total_loss / num_batches:.4f}, "
          f"ece {ece:.4f}, mce {mce:.4f}, nll {nll:.4f}; margins {m}; max|logit| {scale:.3f}")


if __name__ == "__main__":
    main()
