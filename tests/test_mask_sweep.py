"""The missing-modality sweep without a GPU: the subset order, the host metrics against hand-made
confusion matrices, sklearn and the reference fixture, the importance formula, host-side validation
of the new C-ABI entry points (error codes before any launch) and the operators' fake kernels."""
import ctypes
import itertools

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from _sweep import confusion_of, fixture, fixture_names, top2_margin

EINVAL, ELIMIT = 1, 2


@pytest.fixture(scope="module")
def ev(pkg_on_path):
    import mmf_eval
    return mmf_eval


@pytest.fixture(scope="module")
def nat(pkg_on_path):
    import mmf_native
    try:
        mmf_native.lib()
    except RuntimeError as e:
        pytest.fail(f"libmmfusion.so not built: {e}")
    return mmf_native


# ------------------------------------------------------------------ subsets
def test_subsets_in_the_reference_order(ev):
    want = [s for k in range(1, 5) for s in itertools.combinations(range(4), k)]
    assert ev.modality_subsets(4) == want and len(want) == 15
    assert ev.modality_subsets(1) == [(0,)]
    fx = fixture()
    names = fixture_names(fx)
    assert ["+".join(names[i] for i in s) for s in ev.modality_subsets(4)] == [str(n) for n in fx["subset_names"]]


# ------------------------------------------------------------------ metrics
def test_metrics_on_hand_made_matrices(ev):
    # 3 classes; class 2 occurs in neither labels nor predictions: left out of the macro mean
    c = np.array([[3, 1, 0], [2, 4, 0], [0, 0, 0]])
    m = ev.metrics_from_confusion(c)
    assert m["accuracy"] == pytest.approx(7 / 10, abs=1e-15)
    f0, f1 = 2 * 3 / (2 * 3 + 2 + 1), 2 * 4 / (2 * 4 + 1 + 2)
    assert m["f1_macro"] == pytest.approx((f0 + f1) / 2, abs=1e-15)
    # class 2 predicted but never true: counts as 0 in the mean
    c = np.array([[3, 0, 1], [0, 4, 0], [0, 0, 0]])
    m = ev.metrics_from_confusion(c)
    assert m["f1_macro"] == pytest.approx((2 * 3 / (2 * 3 + 0 + 1) + 1.0 + 0.0) / 3, abs=1e-15)
    assert m["accuracy"] == pytest.approx(7 / 8, abs=1e-15)
    # a torch tensor, one class, and no sample at all
    assert ev.metrics_from_confusion(torch.tensor([[5]])) == {"accuracy": 1.0, "f1_macro": 1.0}
    assert ev.metrics_from_confusion(np.zeros((3, 3), np.int64)) == {"accuracy": 0.0, "f1_macro": 0.0}
    with pytest.raises(ValueError):
        ev.metrics_from_confusion(np.zeros((2, 3)))


def test_metrics_agree_with_sklearn_when_importable(ev):
    sk = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(5)
    for C in (2, 5, 9):
        labels = rng.integers(0, C - 1, size=60)      # the last class never true
        preds = rng.integers(0, C, size=60)
        counts = np.zeros((C, C), np.int64)
        np.add.at(counts, (labels, preds), 1)
        m = ev.metrics_from_confusion(counts)
        assert m["f1_macro"] == pytest.approx(sk.f1_score(labels, preds, average="macro", zero_division=0), abs=1e-12)
        assert m["accuracy"] == pytest.approx(sk.accuracy_score(labels, preds), abs=1e-12)


def test_metrics_reproduce_the_fixture(ev):
    fx = fixture()
    assert fx["logits"].shape == (15, 40, 7)
    assert top2_margin(fx["logits"]) >= 1e-2   # the precondition of every argmax comparison below and on the device
    counts = confusion_of(fx["logits"], fx["labels"])
    for s in range(15):
        m = ev.metrics_from_confusion(counts[s])
        assert m["accuracy"] == pytest.approx(float(fx["accuracy"][s]), abs=1e-12)
        assert m["f1_macro"] == pytest.approx(float(fx["f1_macro"][s]), abs=1e-12)


# ------------------------------------------------------------------ importance
def test_importance_reproduces_the_fixture(ev):
    fx = fixture()
    names = fixture_names(fx)
    results = {"all_combinations": {str(n): {"accuracy": float(a)} for n, a in zip(fx["subset_names"], fx["accuracy"])}}
    imp = ev.modality_importance(results, names)
    assert list(imp) == names
    for i, n in enumerate(names):
        assert imp[n] == pytest.approx(float(fx["importance"][i]), abs=1e-12)
    assert sum(abs(v) for v in imp.values()) == pytest.approx(1.0, abs=1e-12)


def test_importance_uses_the_reference_substring_test(ev):
    combos = {"imu": 0.5, "imu_hand": 0.9, "imu+imu_hand": 0.7}
    results = {"all_combinations": {k: {"accuracy": v} for k, v in combos.items()}}
    imp = ev.modality_importance(results, ["imu", "imu_hand"])
    # "imu" is a substring of every name: nothing is "without" it, so its importance is 0
    raw_hand = (0.9 + 0.7) / 2 - 0.5
    assert imp["imu"] == 0.0 and imp["imu_hand"] == pytest.approx(raw_hand / abs(raw_hand), abs=1e-15)
    # all zero: no normalisation
    flat = {"all_combinations": {k: {"accuracy": 0.5} for k in ("a", "b", "a+b")}}
    assert ev.modality_importance(flat, ["a", "b"]) == {"a": 0.0, "b": 0.0}


# ------------------------------------------------------------------ the module's errors without a device
def test_sweep_carries_the_forward_errors(ev, pkg_on_path):
    import fusion
    hf = fusion.HybridFusion({"a": 4, "b": 6}, hidden_dim=8, num_classes=3, num_heads=2).eval()
    feats = {"a": torch.zeros(2, 4), "b": torch.zeros(2, 6)}
    with pytest.raises(KeyError, match="Missing features for modality 'b'"):
        ev.hybrid_mask_sweep(hf, {"a": feats["a"]}, [[1, 1]])
    with pytest.raises(RuntimeError, match="ROCm device"):
        ev.hybrid_mask_sweep(hf, feats, [[1, 1]])
    with pytest.raises(ValueError, match="0/1"):
        ev.hybrid_mask_sweep(hf, feats, [[1, 0.5]])
    with pytest.raises(ValueError, match="entries for 2 modalities"):
        ev.hybrid_mask_sweep(hf, feats, [[1, 0, 1]])
    empty = fusion.HybridFusion({}, hidden_dim=8, num_classes=3, num_heads=2)
    with pytest.raises(ValueError, match="No modalities configured"):
        ev.hybrid_mask_sweep(empty, {}, [[]])


def test_models_beyond_the_sweep_limits_take_the_generic_path(ev, pkg_on_path):
    import fusion
    import harness
    ok = fusion.HybridFusion({"a": 4, "b": 6}, hidden_dim=256, num_classes=1024, num_heads=4)
    assert ev.sweep_supported(ok) and ev._fusion_of(ok) == (ok, False)
    wrapped = harness.MultimodalFusionModel({"a": torch.nn.Identity(), "b": torch.nn.Identity()}, ok, 4, layer_norm=False)
    assert ev._fusion_of(wrapped) == (ok, True)
    for kw in ({"hidden_dim": 512, "num_classes": 5}, {"hidden_dim": 64, "num_classes": 1025}):
        big = fusion.HybridFusion({"a": 4, "b": 6}, num_heads=4, **kw)
        assert not ev.sweep_supported(big) and ev._fusion_of(big) == (None, False)
        wrapped = harness.MultimodalFusionModel({"a": torch.nn.Identity(), "b": torch.nn.Identity()}, big, 4, layer_norm=False)
        assert ev._fusion_of(wrapped) == (None, False)
    assert ev._fusion_of(torch.nn.Linear(3, 2)) == (None, False)


# ------------------------------------------------------------------ host validation of the C-ABI
def _desc(nat, **kw):
    d = nat.HybridDesc()
    d.batch, d.num_modalities, d.hidden, d.num_heads, d.num_classes = 4, 3, 32, 4, 5
    for m in range(3):
        d.seq_len[m] = 0
        d.in_dim[m] = 16
    pairs = [(q, k) for q in range(3) for k in range(3) if q != k]
    d.num_pairs = len(pairs)
    for g, (q, k) in enumerate(pairs):
        d.pair_q[g], d.pair_k[g] = q, k
    d.dropout, d.training, d.return_attention = 0.1, 0, 0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_sweep_validation_with_null_buffers(nat):
    """Every refusal comes before a launch: the buffers are null and no device is needed."""
    L = nat.lib()

    def call(d, pats, S=None):
        flat = [v for r in pats for v in r]
        arr = (ctypes.c_uint8 * max(1, len(flat)))(*flat)
        return L.mmf_hybrid_sweep_forward(ctypes.byref(d), None, None, ctypes.cast(arr, ctypes.c_void_p),
                                          len(pats) if S is None else S, None, None, None, None, None)

    ones = [[1, 1, 1]]
    assert call(_desc(nat, training=1), ones) == EINVAL and b"training" in L.mmf_last_error()
    assert call(_desc(nat, return_attention=1), ones) == EINVAL and b"return_attention" in L.mmf_last_error()
    assert call(_desc(nat), [], 0) == EINVAL and b"num_patterns" in L.mmf_last_error()
    assert call(_desc(nat), [[1, 2, 0]]) == EINVAL and b"entries are 0 or 1" in L.mmf_last_error()
    assert call(_desc(nat), ones * 1025) == ELIMIT and b"1025 patterns" in L.mmf_last_error()
    assert call(_desc(nat, num_classes=1025), ones) == ELIMIT and b"1025 classes" in L.mmf_last_error()
    assert call(_desc(nat, hidden=512), ones) == ELIMIT and b"hidden_dim 512" in L.mmf_last_error()
    # within the limits: the null pointers are refused
    assert call(_desc(nat), ones * 1024) == EINVAL and b"null argument" in L.mmf_last_error()
    assert L.mmf_hybrid_sweep_forward(ctypes.byref(_desc(nat)), None, None, None, 1, None, None, None, None,
                                      None) == EINVAL and b"null patterns" in L.mmf_last_error()


def test_sweep_workspace_grows_with_the_patterns(nat):
    L = nat.lib()
    d = _desc(nat)
    small, large = (L.mmf_hybrid_sweep_workspace_bytes(ctypes.byref(d), S) for S in (1, 1024))
    assert 0 < small < large
    assert L.mmf_hybrid_sweep_workspace_bytes(ctypes.byref(d), 0) == 0
    assert L.mmf_hybrid_sweep_workspace_bytes(ctypes.byref(d), 1025) == 0
    assert L.mmf_hybrid_sweep_workspace_bytes(ctypes.byref(_desc(nat, training=1)), 4) == 0
    # sequence inputs keep their L-means in the workspace
    seq = _desc(nat)
    for m in range(3):
        seq.seq_len[m] = 8
    assert L.mmf_hybrid_sweep_workspace_bytes(ctypes.byref(seq), 1) > small


def test_confusion_validation_with_null_buffers(nat):
    L = nat.lib()
    assert L.mmf_confusion_accumulate(0, 2, 5, None, None, None, None, None) == EINVAL
    assert L.mmf_confusion_accumulate(3, -1, 5, None, None, None, None, None) == EINVAL
    assert L.mmf_confusion_accumulate(3, 2, 0, None, None, None, None, None) == EINVAL
    assert b"bad shape" in L.mmf_last_error()
    assert L.mmf_confusion_accumulate(3, 2, 5, None, None, None, None, None) == EINVAL
    assert b"null argument" in L.mmf_last_error()
    assert L.mmf_confusion_accumulate(3, 0, 5, None, None, None, None, None) == 0   # an empty batch: nothing to do


# ------------------------------------------------------------------ fake kernels
def test_fake_kernels_shapes_and_dtypes(ev, pkg_on_path):
    import mmf_ops
    idesc = mmf_ops.hybrid_idesc(4, 32, 4, 5, [0, 6, 0], [12, 20, 16], [(q, k) for q in range(3) for k in range(3) if q != k],
                                 False, False, 0)
    pats = [1, 1, 1, 0, 1, 0, 0, 0, 0, 1, 0, 1, 1, 1, 0]   # S = 5
    with FakeTensorMode(), torch.device("cuda"):
        xs = [torch.randn(4, 12), torch.randn(4, 6, 20), torch.randn(4, 16)]
        params = [torch.randn(3, requires_grad=True)]
        lg, fw = torch.ops.mmfusion.hybrid_mask_sweep(idesc, 0.1, pats, xs, params, True)
        assert lg.shape == (5, 4, 5) and fw.shape == (5, 4, 3)
        assert all(t.dtype == torch.float32 and t.device.type == "cuda" for t in (lg, fw))
        lg, fw = torch.ops.mmfusion.hybrid_mask_sweep(idesc, 0.1, pats, xs, params, False)
        assert lg.shape == (5, 4, 5) and fw.shape == (0,)
        counts = torch.zeros(5, 5, 5, dtype=torch.int64)
        bad = torch.zeros(1, dtype=torch.int64)
        out = torch.ops.mmfusion.confusion_accumulate(lg, torch.zeros(4, dtype=torch.int64), counts, bad)
        assert out is None and counts.shape == (5, 5, 5) and counts.dtype == torch.int64
