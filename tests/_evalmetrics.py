"""Helpers of the standard-evaluation tests (mmf_eval_accumulate, mmf_eval.EvalAccumulator and
evaluate_model): a float64 oracle of the whole chain of src/eval.py:84-104 and
src/uncertainty.py:109-192 (argmax, softmax confidence, cross-entropy, binning by the float32
edges, the state the device accumulates and the metrics from it), a seeded case builder whose cases
meet the edge precondition by construction, ``check_preconditions`` and the bounds.

Bounds.  The device sums C terms exp(z - max z) in fp32: each term carries expf's rounding and the
subtraction's, and the strided partial sums plus the 6-step butterfly add at most C / 64 + 6 more
roundings to any term's path; 1 / s adds one.  (C + 8) 2^-23 covers that for a confidence (<= 1).
The cross-entropy max z + log s - z[label] is of the size of the logits, so its bound is the same
number times max(1, max|logit|).

Edge precondition.  A confidence changes bin only across an INTERIOR edge: both the oracle's and the
device's confidences are 1 / s with s >= 1 (the maximum's own term is exp(0) = 1), so neither can
leave (0, 1], and the outer edges 0 and 1 bound closed ends that nothing crosses -- with C = 1 every
confidence IS the edge 1.  The precondition therefore asks every oracle confidence to be at least
4 (C + 4) 2^-24 (twice the confidence bound, rounded up) from every interior edge.
"""
from __future__ import annotations

import functools
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from _util import load_fixture

HEAD_WORDS = 8   # include/mmfusion.h: the state's counters and sums before the confusion matrix


def conf_bound(C: int) -> float:
    return (C + 8) * 2.0 ** -23


def ce_bound(C: int, logits) -> float:
    return conf_bound(C) * max(1.0, float(np.abs(np.asarray(logits, dtype=np.float64)).max()))


def edge_margin(C: int) -> float:
    return 4 * (C + 4) * 2.0 ** -24


def edges64(num_bins: int) -> np.ndarray:
    """The reference's float32 edges (src/uncertainty.py:109), widened."""
    return torch.linspace(0.0, 1.0, steps=num_bins + 1).numpy().astype(np.float64)


def bins_of(conf: np.ndarray, num_bins: int) -> np.ndarray:
    """The bin of every confidence (-1: none, as for a NaN): lo <= c < hi, the last bin closed."""
    e = edges64(num_bins)
    out = np.full(conf.shape, -1, np.int64)
    for b in range(num_bins):
        with np.errstate(invalid="ignore"):
            inside = (conf >= e[b]) & ((conf < e[b + 1]) | ((b == num_bins - 1) & (conf <= e[b + 1])))
        out[inside] = b
    return out


def oracle_rows(logits: np.ndarray, labels: np.ndarray, num_bins: int) -> Dict[str, np.ndarray]:
    """Per row in float64, from the float32 logits as given: preds (torch.argmax's rule), conf (the
    softmax's maximum), ce (lse - z[label]; 0 for a label outside [0, C)), bin, valid, nan."""
    z = torch.from_numpy(np.array(logits, dtype=np.float64))   # (a copy: the cases are read-only)
    B, C = z.shape
    y = np.asarray(labels, dtype=np.int64)
    probs = torch.softmax(z, dim=1)
    nan = torch.isnan(probs).any(dim=1).numpy()
    preds = torch.argmax(z, dim=1).numpy()
    conf = np.where(nan, np.nan, probs.max(dim=1).values.numpy())
    valid = (y >= 0) & (y < C)
    yc = torch.from_numpy(np.where(valid, y, 0))
    ce = (torch.logsumexp(z, dim=1) - z.gather(1, yc[:, None])[:, 0]).numpy()
    ce = np.where(nan, np.nan, ce)
    return {"preds": preds, "conf": conf, "ce": np.where(valid, ce, 0.0), "bin": bins_of(conf, num_bins),
            "valid": valid, "nan": nan & valid}


def oracle_state(calls: Sequence[Tuple[np.ndarray, np.ndarray]], num_bins: int) -> Dict[str, np.ndarray]:
    """What the device state holds after the calls [(logits, labels), ...], in float64 / int64."""
    C = calls[0][0].shape[1]
    st = {"samples": 0, "correct": 0, "bad": 0, "calls": 0, "nan_rows": 0, "loss_sum": 0.0, "nll_sum": 0.0,
          "confusion": np.zeros((C, C), np.int64), "bin_count": np.zeros(num_bins, np.int64),
          "bin_correct": np.zeros(num_bins, np.int64), "bin_conf_sum": np.zeros(num_bins, np.float64)}
    for logits, labels in calls:
        if logits.shape[0] == 0:
            continue
        r = oracle_rows(logits, labels, num_bins)
        v = r["valid"]
        y = np.asarray(labels, dtype=np.int64)
        hit = v & (r["preds"] == y)
        st["samples"] += int(v.sum())
        st["correct"] += int(hit.sum())
        st["bad"] += int((~v).sum())
        st["calls"] += 1
        st["nan_rows"] += int(r["nan"].sum())
        st["loss_sum"] += float(r["ce"][v].sum()) / logits.shape[0]
        st["nll_sum"] += float(r["ce"][v].sum())
        np.add.at(st["confusion"], (y[v], r["preds"][v]), 1)
        inb = v & (r["bin"] >= 0)
        np.add.at(st["bin_count"], r["bin"][inb], 1)
        np.add.at(st["bin_correct"], r["bin"][inb & hit], 1)
        np.add.at(st["bin_conf_sum"], r["bin"][inb], r["conf"][inb])
    return st


def oracle_metrics(logits: np.ndarray, labels: np.ndarray, num_bins: int, batches: Optional[Sequence[int]] = None):
    """accuracy / loss / nll / ece / mce of the reference's chain in float64 over all rows (every
    label valid): loss over the given batch sizes (one batch when None), the bins as
    src/uncertainty.py:113-129 walks them."""
    r = oracle_rows(logits, labels, num_bins)
    y = np.asarray(labels, dtype=np.int64)
    N = y.size
    sizes = [N] if batches is None else [int(b) for b in batches]
    lo, loss = 0, 0.0
    for n in sizes:
        loss += float(r["ce"][lo:lo + n].mean())
        lo += n
    hit = r["preds"] == y
    ece, mce = 0.0, 0.0
    for b in range(num_bins):
        inside = r["bin"] == b
        if not inside.any():
            continue
        gap = abs(float(hit[inside].mean()) - float(r["conf"][inside].mean()))
        ece += inside.sum() / N * gap
        mce = max(mce, gap)
    return {"accuracy": float(hit.sum()) / N, "loss": loss / len(sizes), "nll": float(r["ce"].mean()),
            "ece": float(ece), "mce": float(mce)}


def state_fields(words: np.ndarray, C: int, num_bins: int) -> Dict[str, np.ndarray]:
    """A device state (int64 words on the host) taken apart by include/mmfusion.h's layout."""
    w = np.ascontiguousarray(words, dtype=np.int64)
    assert w.shape == (HEAD_WORDS + C * C + 3 * num_bins,), w.shape
    f = w.view(np.float64)
    base = HEAD_WORDS + C * C
    return {"samples": int(w[0]), "correct": int(w[1]), "bad": int(w[2]), "calls": int(w[3]), "nan_rows": int(w[4]),
            "loss_sum": float(f[5]), "nll_sum": float(f[6]), "reserved": int(w[7]),
            "confusion": w[HEAD_WORDS:base].reshape(C, C), "bin_count": w[base:base + num_bins],
            "bin_correct": w[base + num_bins:base + 2 * num_bins],
            "bin_conf_sum": f[base + 2 * num_bins:base + 3 * num_bins]}


def build_state(C: int, num_bins: int, **fields) -> np.ndarray:
    """The inverse of state_fields for hand-built states."""
    w = np.zeros(HEAD_WORDS + C * C + 3 * num_bins, np.int64)
    f = w.view(np.float64)
    base = HEAD_WORDS + C * C
    for i, k in enumerate(("samples", "correct", "bad", "calls", "nan_rows")):
        w[i] = fields.get(k, 0)
    f[5], f[6] = fields.get("loss_sum", 0.0), fields.get("nll_sum", 0.0)
    w[HEAD_WORDS:base] = np.asarray(fields.get("confusion", np.zeros((C, C))), np.int64).reshape(-1)
    w[base:base + num_bins] = fields.get("bin_count", 0)
    w[base + num_bins:base + 2 * num_bins] = fields.get("bin_correct", 0)
    f[base + 2 * num_bins:base + 3 * num_bins] = fields.get("bin_conf_sum", 0.0)
    return w


def check_preconditions(logits: np.ndarray, labels: np.ndarray, num_bins: int) -> Dict[str, np.ndarray]:
    """Asserts what the exact comparisons need and returns the oracle's rows: finite logits, labels
    in range, no exact tie at the top, every confidence edge_margin(C) from every interior edge."""
    C = logits.shape[1]
    assert np.isfinite(logits).all() and logits.dtype == np.float32
    assert ((labels >= 0) & (labels < C)).all()
    r = oracle_rows(logits, labels, num_bins)
    if C > 1:
        top = np.sort(logits.astype(np.float64), axis=1)[:, -2:]
        assert (top[:, 1] > top[:, 0]).all(), "an exact tie at the top: the argmax is not decided by the values"
    inner = edges64(num_bins)[1:-1]
    if inner.size:
        dist = np.abs(r["conf"][:, None] - inner[None, :]).min()
        assert dist >= edge_margin(C), f"a confidence lies {dist:.3e} from an edge, under {edge_margin(C):.3e}"
    assert (r["bin"] >= 0).all()
    return r


@functools.lru_cache(maxsize=None)
def case(B: int, C: int, num_bins: int, seed: int = 0) -> Tuple[np.ndarray, np.ndarray]:
    """Seeded (logits (B, C) float32, labels (B) int64): normal logits scaled so the confidences
    spread over the bins, the first B of 8 B + 64 candidate rows that stand twice edge_margin(C)
    from every interior edge; the labels are the argmax with 40 % redrawn.  Cached and shared: the
    tests must not modify the arrays."""
    rng = np.random.default_rng(1000 * B + 10 * C + num_bins + 7919 * seed)
    n = 8 * B + 64
    scale = 2.0 + 2.0 * np.log2(max(C, 2)) / 10.0
    cand = (rng.standard_normal((n, C)) * scale).astype(np.float32)
    conf = torch.softmax(torch.from_numpy(cand.astype(np.float64)), dim=1).max(dim=1).values.numpy()
    inner = edges64(num_bins)[1:-1]
    ok = np.ones(n, bool)
    if inner.size:
        ok = np.abs(conf[:, None] - inner[None, :]).min(axis=1) >= 2 * edge_margin(C)
    keep = np.flatnonzero(ok)[:B]
    assert keep.size == B, f"only {int(ok.sum())} of {n} candidates clear the edges"
    logits = np.ascontiguousarray(cand[keep])
    labels = logits.argmax(axis=1).astype(np.int64)
    redraw = rng.random(B) < 0.4
    labels = np.where(redraw, rng.integers(0, C, size=B), labels).astype(np.int64)
    logits.setflags(write=False)
    labels.setflags(write=False)
    return logits, labels


@functools.lru_cache(maxsize=None)
def fixture():
    return load_fixture("eval_metrics_ref")


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
    lo, out = 0, []
    for n in (int(v) for v in fx["batches"]):
        feats = {m: torch.from_numpy(fx[f"x/{m}"][lo:lo + n]).to(dev) for m in names}
        out.append((feats, torch.from_numpy(fx["labels"][lo:lo + n]).to(dev), torch.ones(n, len(names), device=dev)))
        lo += n
    return out


def fixture_margins(logits: np.ndarray, labels: np.ndarray, num_bins: int) -> Dict[str, float]:
    """The margins the fixture's generator asserts and the GPU test asserts again: the smallest
    top-2 gap and the smallest distance of a confidence from ANY edge, both over max|logit|; the
    populated bins and those holding both right and wrong predictions."""
    lg = np.asarray(logits, dtype=np.float64)
    r = oracle_rows(np.asarray(logits, dtype=np.float32), labels, num_bins)
    top = np.sort(lg, axis=1)[:, -2:]
    scale = float(np.abs(lg).max())
    hit = r["preds"] == labels
    populated = [b for b in range(num_bins) if (r["bin"] == b).any()]
    mixed = [b for b in populated if hit[r["bin"] == b].any() and (~hit[r["bin"] == b]).any()]
    return {"gap": float((top[:, 1] - top[:, 0]).min()) / scale,
            "edge": float(np.abs(r["conf"][:, None] - edges64(num_bins)[None, :]).min()) / scale,
            "populated": len(populated), "mixed": len(mixed)}
