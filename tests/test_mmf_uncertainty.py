"""mmf_uncertainty without a GPU: the module surface of the reference's src/uncertainty.py
(constructors, attributes, error messages, state_dict keys), the "no CPU path" errors, host-side
validation of the new C-ABI entry points (error codes before any launch) and the fake kernels of
the new torch operators."""
import ctypes

import pytest
import torch
import torch.nn as nn
from torch._subclasses.fake_tensor import FakeTensorMode

EINVAL, ELIMIT = 1, 2


@pytest.fixture(scope="module")
def unc(pkg_on_path):
    import mmf_uncertainty
    return mmf_uncertainty


@pytest.fixture(scope="module")
def nat(pkg_on_path):
    import mmf_native
    try:
        mmf_native.lib()
    except RuntimeError as e:
        pytest.fail(f"libmmfusion.so not built: {e}")
    return mmf_native


# ------------------------------------------------------------------ module surface
def test_module_surface(unc):
    model = nn.Linear(4, 3)
    mc = unc.MCDropoutUncertainty(model)
    assert mc.model is model and mc.num_samples == 10
    assert unc.MCDropoutUncertainty(model, num_samples=3).num_samples == 3
    assert unc.MCDropoutUncertainty(model, 5).num_samples == 5
    assert list(mc.state_dict()) == ["model.weight", "model.bias"]   # the wrapped model is a submodule
    assert unc.UncertaintyWeightedFusion().epsilon == 1e-6
    assert unc.UncertaintyWeightedFusion(epsilon=1e-3).epsilon == 1e-3
    ts = unc.TemperatureScaling()
    assert list(ts.state_dict()) == ["temperature"]
    assert isinstance(ts.temperature, nn.Parameter) and ts.temperature.shape == (1,)
    assert float(ts.temperature.detach()) == 1.0 and ts.temperature.dtype == torch.float32
    x = torch.randn(3, 5)
    with torch.no_grad():
        ts.temperature.fill_(2.0)
    assert torch.equal(ts(x), x / 2.0)   # forward is logits / T, on any device
    ens = unc.EnsembleUncertainty([model, nn.Linear(4, 3)])
    assert ens.num_models == 2 and ens.models[0] is model
    assert not isinstance(ens, nn.Module)
    assert not hasattr(unc, "CalibrationMetrics")   # calibration.py's, untouched


def test_reference_errors(unc):
    with pytest.raises(ValueError, match="Ensemble must contain at least one model."):
        unc.EnsembleUncertainty([]).predict_with_uncertainty(torch.zeros(2, 4))
    uwf = unc.UncertaintyWeightedFusion()
    with pytest.raises(ValueError, match="No modality predictions supplied for fusion."):
        uwf({}, {}, torch.ones(2, 0))
    with pytest.raises(KeyError, match="Missing uncertainty for modality 'b'."):
        uwf({"a": torch.zeros(2, 3), "b": torch.zeros(2, 3)}, {"a": torch.zeros(2)}, torch.ones(2, 2))


def test_cpu_tensors_raise(unc, pkg_on_path):
    import fusion
    with pytest.raises(RuntimeError, match="ROCm device"):
        unc.MCDropoutUncertainty(nn.Linear(4, 3), 2)(torch.zeros(2, 4))
    hf = fusion.HybridFusion({"a": 4, "b": 6}, hidden_dim=8, num_classes=3, num_heads=2).eval()
    mc = unc.MCDropoutUncertainty(hf, 2)
    with pytest.raises(RuntimeError, match="ROCm device"):
        mc({"a": torch.zeros(2, 4), "b": torch.zeros(2, 6)})
    assert not hf.training   # the mode is restored when the call raises
    with pytest.raises(RuntimeError, match="ROCm device"):
        unc.EnsembleUncertainty([nn.Linear(4, 3)]).predict_with_uncertainty(torch.zeros(2, 4))
    with pytest.raises(RuntimeError, match="ROCm device"):
        unc.UncertaintyWeightedFusion()({"a": torch.zeros(2, 3)}, {"a": torch.ones(2)}, torch.ones(2, 1))
    ts = unc.TemperatureScaling()
    with pytest.raises(RuntimeError, match="ROCm device"):
        ts.calibrate(torch.zeros(4, 3), torch.zeros(4, dtype=torch.long))


def test_mc_dropout_needs_a_sample(unc):
    with pytest.raises(RuntimeError, match="non-empty list"):
        unc.MCDropoutUncertainty(nn.Linear(4, 3), 0)(torch.zeros(2, 4))


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
    d.dropout, d.training, d.return_attention = 0.1, 1, 0
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def test_mc_reduce_limits_cpu(nat):
    """Error codes before any launch (no pointer is dereferenced; no GPU needed)."""
    L = nat.lib()
    assert L.mmf_mc_reduce(4, 2, 1025, None, None, None, None, None) == ELIMIT
    assert b"1025 classes" in L.mmf_last_error()
    assert L.mmf_mc_reduce(0, 2, 5, None, None, None, None, None) == EINVAL
    assert b"samples" in L.mmf_last_error()
    assert L.mmf_mc_reduce(4, 2, 0, None, None, None, None, None) == EINVAL
    assert L.mmf_mc_reduce(4, -1, 5, None, None, None, None, None) == EINVAL
    assert L.mmf_mc_reduce(4, 2, 1024, None, None, None, None, None) == EINVAL   # within the limit: null stack
    assert L.mmf_mc_reduce(4, 0, 5, None, None, None, None, None) == 0           # an empty batch: nothing to do


def test_hybrid_mc_forward_validation_cpu(nat):
    L = nat.lib()
    buf = (ctypes.c_float * 4096)()
    host = ctypes.addressof(buf)
    params = nat.HybridParams()
    xs = nat.ptr_array([host] * 3)
    rng = (ctypes.c_uint64 * 2)()

    def call(d, samples):
        return L.mmf_hybrid_mc_forward(ctypes.byref(d), ctypes.byref(params), ctypes.cast(xs, ctypes.c_void_p), host,
                                       ctypes.addressof(rng), samples, host, host, host, host, host, host, None)

    assert call(_desc(nat), 0) == EINVAL and b"samples" in L.mmf_last_error()
    assert call(_desc(nat), -3) == EINVAL
    assert call(_desc(nat, training=0), 4) == EINVAL and b"training" in L.mmf_last_error()
    assert call(_desc(nat, return_attention=1), 4) == EINVAL and b"return_attention" in L.mmf_last_error()
    assert call(_desc(nat, num_classes=1025), 4) == ELIMIT and b"1025 classes" in L.mmf_last_error()
    # the buffer contract, as mmf_hybrid_forward checks it: no capacity declared -> refused before a launch
    d = _desc(nat)
    d.plan_flags = L.mmf_hybrid_plan_flags()
    assert call(d, 4) == EINVAL and b"saved buffer too small" in L.mmf_last_error()
    d.saved_capacity = L.mmf_hybrid_saved_bytes(ctypes.byref(d))
    d.plan_flags = L.mmf_hybrid_plan_flags() ^ 1
    assert call(d, 4) == EINVAL and b"plan switches" in L.mmf_last_error()
    assert rng[1] == 0   # nothing ran


def test_temperature_nll_validation_cpu(nat):
    L = nat.lib()
    assert L.mmf_temperature_nll_workspace_bytes(1) >= 8
    assert L.mmf_temperature_nll_workspace_bytes(10 ** 7) == L.mmf_temperature_nll_workspace_bytes(10 ** 8)
    assert L.mmf_temperature_nll(8, 1025, None, None, None, None, None, None, None) == ELIMIT
    assert b"1025 classes" in L.mmf_last_error()
    assert L.mmf_temperature_nll(0, 5, None, None, None, None, None, None, None) == EINVAL
    assert L.mmf_temperature_nll(8, 0, None, None, None, None, None, None, None) == EINVAL
    assert L.mmf_temperature_nll(8, 5, None, None, None, None, None, None, None) == EINVAL   # null arguments


def test_uncertainty_fusion_limits_cpu(nat):
    L = nat.lib()
    for fn, nargs in ((L.mmf_uncertainty_fusion_forward, 3), (L.mmf_uncertainty_fusion_backward, 4)):
        def call(B, M, C):
            return fn(B, M, C, None, None, None, 1e-6, *([None] * nargs))
        assert call(2, 65, 5) == ELIMIT and b"64 modalities" in L.mmf_last_error()
        assert call(2, 0, 5) == EINVAL
        assert call(2, 3, 0) == EINVAL
        assert call(-1, 3, 5) == EINVAL
        assert call(0, 3, 5) == 0
    assert L.mmf_uncertainty_fusion_forward(2, 64, 5, None, None, None, 1e-6, None, None, None) == EINVAL


# ------------------------------------------------------------------ fake kernels
def test_fake_kernels_shapes_and_dtypes(unc, pkg_on_path):
    import fusion
    import mmf_ops  # noqa: F401
    with FakeTensorMode(), torch.device("cuda"):
        ml, mp, var = torch.ops.mmfusion.mc_reduce(torch.randn(7, 4, 11))
        assert ml.shape == (4, 11) and mp.shape == (4, 11) and var.shape == (4,)
        assert all(t.dtype == torch.float32 and t.device.type == "cuda" for t in (ml, mp, var))
        temp = torch.ones(1, requires_grad=True)
        loss, dtemp = torch.ops.mmfusion.temperature_nll(torch.randn(9, 5), torch.zeros(9, dtype=torch.int64), temp)
        assert loss.shape == () and dtemp.shape == (1,) and loss.dtype == torch.float32 and loss.requires_grad
        stacked = torch.randn(4, 3, 5, requires_grad=True)
        u = torch.rand(4, 3, requires_grad=True)
        fused, w = torch.ops.mmfusion.uncertainty_fusion_fwd(stacked, u, torch.ones(4, 3), 1e-6)
        assert fused.shape == (4, 5) and w.shape == (4, 3) and fused.requires_grad
        ds, du = torch.ops.mmfusion.uncertainty_fusion_bwd(stacked, u, torch.ones(4, 3), 1e-6, torch.randn(4, 5))
        assert ds.shape == (4, 3, 5) and du.shape == (4, 3) and du.dtype == torch.float32
        # the modules run end to end through the fake kernels
        uwf = unc.UncertaintyWeightedFusion()
        preds = {k: torch.randn(4, 5, requires_grad=True) for k in ("a", "b", "c")}
        fused, w = uwf(preds, {k: torch.rand(4) for k in preds}, torch.ones(4, 3))
        assert fused.shape == (4, 5) and w.shape == (4, 3) and fused.requires_grad
        dims = {"a": 12, "b": 20}
        hf = fusion.HybridFusion(dims, hidden_dim=32, num_classes=5, num_heads=4, dropout=0.1).eval()
        feats = {k: torch.randn(4, d) for k, d in dims.items()}
        mean_logits, variance = unc.MCDropoutUncertainty(hf, 3)(feats, torch.ones(4, 2))   # (fake tensors: the generic loop)
        assert mean_logits.shape == (4, 5) and variance.shape == (4,) and not hf.training
        probs, variance = unc.EnsembleUncertainty([hf, hf]).predict_with_uncertainty(feats)
        assert probs.shape == (4, 5) and variance.shape == (4,)
