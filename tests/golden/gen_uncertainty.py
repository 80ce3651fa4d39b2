"""Generate the uncertainty parity fixture by running the REFERENCE's src/uncertainty.py on the CPU.

Generation-time tool (never run by a test): it imports the reference checkout given with
``--reference`` (its ``src/`` directory holds ``uncertainty.py``; nothing of it is copied) and
writes ``uncertainty_ref.npz`` next to this file.  Only inputs and recorded results are stored.

  1. ``TemperatureScaling.calibrate`` (src/uncertainty.py:393-438, LBFGS lr 0.01, max_iter 50):
     N = 512 samples, C = 11 classes; logits = 3 * (N(0, 1) + 3 * onehot(noisy label)), i.e.
     well-separated logits scaled by 3, so the model is over-confident and T moves away from 1;
     labels from the same seeded generator.  Stored: logits, labels, the learned T and the
     reference's mean NLL at that T.
  2. ``UncertaintyWeightedFusion.forward`` (:305-362) at B = 6, M = 3, C = 5 with mask rows: all
     ones, one modality absent, fractional entries, all zero (the 1 / M fallback), two absent, all
     ones.  Stored: predictions, uncertainties, mask, the upstream gradient, fused logits, fusion
     weights and autograd's gradients of sum(fused * upstream) in the predictions and the
     uncertainties.

Run:  python tests/golden/gen_uncertainty.py --reference <path to the reference checkout>
"""

from __future__ import annotations

import argparse
import sys
from pathlib import Path

import numpy as np
import torch
import torch.nn.functional as F

HERE = Path(__file__).resolve().parent
CAL_N, CAL_C, CAL_SEED = 512, 11, 2024
UWF_B, UWF_M, UWF_C, UWF_SEED = 6, 3, 5, 2025
UWF_MASK = [[1, 1, 1], [1, 0, 1], [0.5, 1, 0.25], [0, 0, 0], [0, 1, 0], [1, 1, 1]]
UWF_NAMES = ["imu", "video", "hr"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="the reference checkout (holds src/uncertainty.py)")
    args = ap.parse_args()
    sys.path.insert(0, str(Path(args.reference) / "src"))
    import uncertainty as ref_unc

    torch.set_num_threads(1)
    out = {}

    rng = np.random.default_rng(CAL_SEED)
    labels = rng.integers(0, CAL_C, size=CAL_N)
    # a fifth of the samples point at another class: confident and wrong
    shown = np.where(rng.random(CAL_N) < 0.2, rng.integers(0, CAL_C, size=CAL_N), labels)
    logits = rng.standard_normal((CAL_N, CAL_C))
    logits[np.arange(CAL_N), shown] += 3.0
    logits = (3.0 * logits).astype(np.float32)
    ts = ref_unc.TemperatureScaling()
    ts.calibrate(torch.from_numpy(logits), torch.from_numpy(labels))
    T = float(ts.temperature.detach()[0])
    with torch.no_grad():
        nll = float(F.cross_entropy(torch.from_numpy(logits) / ts.temperature, torch.from_numpy(labels)))
        nll1 = float(F.cross_entropy(torch.from_numpy(logits), torch.from_numpy(labels)))
    out.update({"cal/logits": logits, "cal/labels": labels.astype(np.int64), "cal/temperature": np.asarray([T]),
                "cal/nll": np.asarray([nll]), "cal/nll_at_1": np.asarray([nll1])})
    print(f"calibrate: T = {T:.6f}, NLL {nll1:.6f} -> {nll:.6f}")

    rng = np.random.default_rng(UWF_SEED)
    preds = rng.standard_normal((UWF_B, UWF_M, UWF_C)).astype(np.float32)
    unc = (0.05 + rng.random((UWF_B, UWF_M))).astype(np.float32)
    upstream = rng.standard_normal((UWF_B, UWF_C)).astype(np.float32)
    mask = np.asarray(UWF_MASK, np.float32)
    pt = {n: torch.from_numpy(preds[:, j].copy()).requires_grad_(True) for j, n in enumerate(UWF_NAMES)}
    ut = {n: torch.from_numpy(unc[:, j].copy()).requires_grad_(True) for j, n in enumerate(UWF_NAMES)}
    fused, weights = ref_unc.UncertaintyWeightedFusion()(pt, ut, torch.from_numpy(mask))
    (fused * torch.from_numpy(upstream)).sum().backward()
    out.update({"uwf/predictions": preds, "uwf/uncertainties": unc, "uwf/mask": mask, "uwf/upstream": upstream,
                "uwf/fused": fused.detach().numpy(), "uwf/weights": weights.detach().numpy(),
                "uwf/dpredictions": np.stack([pt[n].grad.numpy() for n in UWF_NAMES], axis=1),
                "uwf/duncertainties": np.stack([ut[n].grad.numpy() for n in UWF_NAMES], axis=1)})
    assert np.all(out["uwf/duncertainties"][3] == 0) and np.allclose(out["uwf/weights"][3], 1.0 / UWF_M)
    np.savez_compressed(HERE / "uncertainty_ref.npz", **out)
    print("wrote uncertainty_ref.npz")


if __name__ == "__main__":
    main()
