"""GPU tests of the missing-modality sweep (mmf_eval, mmf_hybrid_sweep_forward,
mmf_confusion_accumulate): the reference fixture, float64 parity per pattern over the shape cases
of tests/_sweep.py, precision "medium", selection under NaN inputs, the confusion kernel alone, the
full model's fast path against its generic path, reruns, and one shared pass per call.

Bounds: 1e-3 of max|reference| is the project's fp32 bound (tests/test_gpu_parity.py) against the
float64 oracle; the sweep against the device's own per-pattern forward gets 2e-3, the triangle bound
of two results each within 1e-3 of the oracle; "medium" gets tests/test_gpu_bf16.py's LOGIT_RTOL."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from _sweep import (CASES, WEIGHT_CASES, all_patterns, build_hybrid, case_inputs, fixture, fixture_batches,
                    fixture_model, fixture_names, oracle_sweep, top2_margin)
from _util import close, diff_report

pytestmark = pytest.mark.gpu
RTOL, RTOL_DEVICE, LOGIT_RTOL = 1e-3, 2e-3, 3e-2


@pytest.fixture(scope="module")
def mods(pkg_on_path):
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible")
    import fusion
    import mmf_eval
    import mmf_native
    mmf_native.lib()
    prev = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision("highest")
    yield fusion, mmf_eval, mmf_native
    torch.set_float32_matmul_precision(prev)


def _cuda(feats):
    return {m: v.cuda() for m, v in feats.items()}


# ------------------------------------------------------------------ the reference fixture
def test_reference_fixture_through_hybrid_fusion(mods):
    fusion, ev, _ = mods
    fx = fixture()
    names = fixture_names(fx)
    assert top2_margin(fx["logits"]) >= 1e-2   # ten times the parity bound: the device's argmax cannot differ
    model = fixture_model(fusion, fx)
    subsets = ev.modality_subsets(len(names))
    patterns = [[1 if m in s else 0 for m in range(len(names))] for s in subsets]
    feats = {m: torch.from_numpy(fx[f"x/{m}"]).cuda() for m in names}
    logits = ev.hybrid_mask_sweep(model, feats, patterns)
    assert logits.shape == (15, 40, 7) and not logits.requires_grad
    for s in range(15):
        assert close(logits[s], fx["logits"][s], RTOL), (str(fx["subset_names"][s]), diff_report(logits[s], fx["logits"][s], RTOL))
    res = ev.evaluate_missing_modalities(model, fixture_batches(fx), names)
    assert list(res) == ["full_modalities", "single_modalities", "all_combinations", "modality_importance"]
    assert list(res["all_combinations"]) == [str(n) for n in fx["subset_names"]]
    for s, key in enumerate(res["all_combinations"]):
        m = res["all_combinations"][key]
        assert set(m) == {"accuracy", "f1_macro"}
        assert m["accuracy"] == pytest.approx(float(fx["accuracy"][s]), abs=1e-12), key
        assert m["f1_macro"] == pytest.approx(float(fx["f1_macro"][s]), abs=1e-12), key
    assert res["full_modalities"] == res["all_combinations"]["+".join(names)]
    assert list(res["single_modalities"]) == names
    assert all(res["single_modalities"][n] == res["all_combinations"][n] for n in names)
    for i, n in enumerate(names):
        assert res["modality_importance"][n] == pytest.approx(float(fx["importance"][i]), abs=1e-12)
    assert not model.training


# ------------------------------------------------------------------ parity per pattern
@pytest.mark.parametrize("name", list(CASES))
def test_parity_per_pattern(mods, name):
    fusion, ev, _ = mods
    case = CASES[name]
    M = len(case.names)
    pats = all_patterns(M)
    ref_logits, ref_weights = oracle_sweep(name)
    model = build_hybrid(fusion, case)
    feats = _cuda(case_inputs(case))
    want_w = name in WEIGHT_CASES
    out = ev.hybrid_mask_sweep(model, feats, pats, return_weights=want_w)
    logits, weights = out if want_w else (out, None)
    assert logits.shape == (len(pats), case.batch, case.classes)
    torch.cuda.synchronize()
    with torch.no_grad():
        for s, pat in enumerate(pats):
            assert close(logits[s], ref_logits[s], RTOL), (name, pat, diff_report(logits[s], ref_logits[s], RTOL))
            mask = torch.tensor(pat, dtype=torch.float32, device="cuda").repeat(case.batch, 1)
            x = {m: (v if pat[i] else torch.zeros_like(v)) for i, (m, v) in enumerate(feats.items())}
            own = model(x, mask)
            assert close(logits[s], own, RTOL_DEVICE), (name, pat, diff_report(logits[s], own, RTOL_DEVICE))
            if want_w:
                assert close(weights[s], ref_weights[s], RTOL), (name, pat, diff_report(weights[s], ref_weights[s], RTOL))
    # the all-zero pattern: classifier(0) for every sample, weights 1 / M
    assert pats[0] == (0,) * M
    assert torch.equal(logits[0], logits[0][:1].expand_as(logits[0]))
    if want_w:
        assert torch.equal(weights[0], torch.ones_like(weights[0]) / M)


def test_precision_medium(mods):
    fusion, ev, _ = mods
    name = "m4_2d"
    case = CASES[name]
    ref_logits, _ = oracle_sweep(name)
    model = build_hybrid(fusion, case)
    torch.set_float32_matmul_precision("medium")
    try:
        logits = ev.hybrid_mask_sweep(model, _cuda(case_inputs(case)), all_patterns(len(case.names)))
    finally:
        torch.set_float32_matmul_precision("highest")
    for s in range(logits.size(0)):
        assert close(logits[s], ref_logits[s], LOGIT_RTOL), (s, diff_report(logits[s], ref_logits[s], LOGIT_RTOL))


# ------------------------------------------------------------------ selection, not multiplication
def test_absent_modalities_are_never_read(mods):
    fusion, ev, _ = mods
    case = CASES["m4_2d"]
    pats = all_patterns(4)
    model = build_hybrid(fusion, case)
    feats = _cuda(case_inputs(case))
    clean = ev.hybrid_mask_sweep(model, feats, pats)
    bad = 2
    dirty_feats = dict(feats)
    dirty_feats[case.names[bad]] = torch.full_like(feats[case.names[bad]], float("nan"))
    dirty = ev.hybrid_mask_sweep(model, dirty_feats, pats)
    assert bool(torch.isfinite(clean).all())
    for s, pat in enumerate(pats):
        if pat[bad]:
            assert bool(torch.isnan(dirty[s]).all()), pat
        else:
            assert bool(torch.isfinite(dirty[s]).all()) and torch.equal(dirty[s], clean[s]), pat


# ------------------------------------------------------------------ the confusion kernel alone
def _conf(logits, labels):
    S, B, C = logits.shape
    counts = torch.zeros(S, C, C, dtype=torch.int64, device="cuda")
    bad = torch.zeros(1, dtype=torch.int64, device="cuda")
    torch.ops.mmfusion.confusion_accumulate(logits.cuda().contiguous(), labels.cuda(), counts, bad)
    return counts, bad


@pytest.mark.parametrize("C", [1, 7, 300])
def test_confusion_accumulate(mods, C):
    S, B = 3, 37
    g = torch.Generator().manual_seed(C)
    logits = torch.randn(S, B, C, generator=g)
    if C > 1:
        logits[0, 0, :] = 0.5                       # every class ties: index 0
        logits[0, 1, C - 1] = logits[0, 1, 1] = 9.0   # a tie between two maxima: the lower index
        logits[1, 2, C // 2] = float("nan")           # a NaN counts as the maximum
        logits[1, 3, :] = float("nan")                # all NaN: the first
        logits[2, 4, C - 1] = float("inf")
        logits[2, 5, :] = float("-inf")
    labels = torch.randint(0, C, (B,), generator=g)
    preds = logits.argmax(dim=2)                      # torch.argmax on the CPU
    want = torch.zeros(S, C, C, dtype=torch.int64)
    for s in range(S):
        want[s] = torch.bincount(labels * C + preds[s], minlength=C * C).reshape(C, C)
    counts, bad = _conf(logits, labels)
    assert torch.equal(counts.cpu(), want) and int(bad) == 0
    assert int(counts.sum()) == S * B
    # a second call accumulates
    torch.ops.mmfusion.confusion_accumulate(logits.cuda(), labels.cuda(), counts, bad)
    assert torch.equal(counts.cpu(), 2 * want) and int(bad) == 0
    # labels out of range are counted apart and touch no count
    off = labels.clone()
    off[0], off[5] = -1, C
    counts2, bad2 = _conf(logits, off)
    keep = torch.ones(B, dtype=torch.bool)
    keep[0] = keep[5] = False
    want2 = torch.zeros_like(want)
    for s in range(S):
        want2[s] = torch.bincount(labels[keep] * C + preds[s][keep], minlength=C * C).reshape(C, C)
    assert torch.equal(counts2.cpu(), want2) and int(bad2) == 2 * S


# ------------------------------------------------------------------ the full model
class _Plain(nn.Module):
    """A thin wrapper: not a MultimodalFusionModel, so evaluate_missing_modalities takes the generic path."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, features, mask=None):
        return self.inner(features, mask)


def _config(fusion_type):
    enc = {"imu_hand": {"type": "sequence", "input_dim": 9, "encoder_type": "lstm", "num_layers": 1, "hidden_dim": 64},
           "imu_chest": {"type": "sequence", "input_dim": 6, "encoder_type": "lstm", "num_layers": 1, "hidden_dim": 64},
           "video": {"type": "frame", "input_dim": 24, "hidden_dim": 32}}
    return {"dataset": {"modalities": list(enc), "num_classes": 6},
            "model": {"fusion_type": fusion_type, "hidden_dim": 32, "output_dim": 32, "num_heads": 4, "dropout": 0.1,
                      "layer_norm": True, "encoders": enc}}


def _samples(n, seed):
    g = torch.Generator().manual_seed(seed)
    return {"imu_hand": torch.randn(n, 10, 9, generator=g), "imu_chest": torch.randn(n, 10, 6, generator=g),
            "video": torch.randn(n, 5, 24, generator=g)}


def test_full_model_fast_path_equals_generic_path(mods):
    _, ev, _ = mods
    from harness import MultimodalFusionModel
    torch.manual_seed(11)
    model = MultimodalFusionModel.from_config(_config("hybrid")).cuda().eval()
    names = list(model.encoders)
    subsets = ev.modality_subsets(3)
    patterns = [[1 if m in s else 0 for m in range(3)] for s in subsets]

    def generic_logits(feats):
        out = []
        with torch.no_grad():
            for s in subsets:
                mask = torch.zeros(feats[names[0]].size(0), 3, device="cuda")
                mask[:, list(s)] = 1
                out.append(model({m: (v if i in s else torch.zeros_like(v)) for i, (m, v) in enumerate(feats.items())}, mask))
        return torch.stack(out)

    # an untrained model's logits lie close together: keep the first 8 of 48 seeded samples whose top-2
    # gap is >= 1.5e-2 of max|logits| under every subset ON THE GENERIC PATH (the code under test is not asked)
    cand = _cuda(_samples(48, 21))
    lg = generic_logits(cand)
    top = lg.topk(2, dim=-1).values
    ok = ((top[..., 0] - top[..., 1]) >= 1.5e-2 * lg.abs().max()).all(dim=0)
    keep = torch.nonzero(ok).flatten()[:8]
    assert keep.numel() == 8, int(ok.sum())
    feats = {m: v[keep].contiguous() for m, v in cand.items()}
    labels = generic_logits(feats)[-1].argmax(dim=1)
    labels[::3] = (labels[::3] + 1) % 6
    batches = [({m: v[lo:lo + 4] for m, v in feats.items()}, labels[lo:lo + 4], torch.ones(4, 3)) for lo in (0, 4)]

    # the precondition, on the generic path's logits of the very batches: 1e-2 is five times the 2e-3 bound
    gl = torch.cat([generic_logits(b[0]) for b in batches], dim=1)
    assert top2_margin(gl.cpu()) >= 1e-2
    with torch.no_grad():
        fl = torch.cat([ev.hybrid_mask_sweep(model.fusion_model, model.encode(b[0]), patterns) for b in batches], dim=1)
    assert close(fl, gl, RTOL_DEVICE), diff_report(fl, gl, RTOL_DEVICE)

    fast = ev.evaluate_missing_modalities(model, batches, names)
    generic = ev.evaluate_missing_modalities(_Plain(model), batches, names)
    assert list(fast["all_combinations"]) == ["+".join(names[i] for i in s) for s in subsets]
    assert fast == generic   # identical counts give identical floats
    want_full = float((gl[-1].argmax(dim=1) == labels).double().mean())
    assert fast["full_modalities"]["accuracy"] == pytest.approx(want_full, abs=1e-12)


def test_late_fusion_model_runs_the_generic_path(mods):
    _, ev, _ = mods
    from harness import MultimodalFusionModel
    torch.manual_seed(12)
    model = MultimodalFusionModel.from_config(_config("late")).cuda().eval()
    names = list(model.encoders)
    feats = _samples(8, 22)
    labels = torch.arange(8) % 6
    batches = [({m: v[lo:lo + 4] for m, v in feats.items()}, labels[lo:lo + 4], torch.ones(4, 3)) for lo in (0, 4)]
    res = ev.evaluate_missing_modalities(model, batches, names)
    assert len(res["all_combinations"]) == 7 and list(res["single_modalities"]) == names
    for m in res["all_combinations"].values():
        assert 0.0 <= m["accuracy"] <= 1.0 and 0.0 <= m["f1_macro"] <= 1.0
    assert set(res["modality_importance"]) == set(names)
    bad = [(batches[0][0], torch.full((4,), 6), batches[0][2])]
    with pytest.raises(ValueError, match="outside"):
        ev.evaluate_missing_modalities(model, bad, names)


# ------------------------------------------------------------------ reruns and the shared pass
@pytest.mark.parametrize("name", ["m5_2d", "m3_mixed_l"])
def test_reruns_are_bit_identical(mods, name):
    fusion, ev, _ = mods
    case = CASES[name]
    model = build_hybrid(fusion, case)
    feats = _cuda(case_inputs(case))
    pats = all_patterns(len(case.names))
    a, aw = ev.hybrid_mask_sweep(model, feats, pats, return_weights=True)
    for _ in range(2):
        b, bw = ev.hybrid_mask_sweep(model, feats, pats, return_weights=True)
        assert torch.equal(a, b) and torch.equal(aw, bw)


@pytest.mark.parametrize("name", ["m4_2d", "m3_mixed_l", "m3_general", "m2_l128"])
def test_the_shared_pass_runs_once(mods, name):
    """The library's stage counters: S patterns cost ONE shared pass (the forward's own launches,
    once) and ONE tail launch.  And the plan each case is there for is the one that ran."""
    fusion, ev, nat = mods
    case = CASES[name]
    model = build_hybrid(fusion, case)
    feats = _cuda(case_inputs(case))
    pats = all_patterns(len(case.names))
    with torch.no_grad():
        model(feats)                                   # (warm: allocations, the extension)
        ev.hybrid_mask_sweep(model, feats, pats)
        torch.cuda.synchronize()
        nat.profile_begin()
        model(feats)
        _, single = nat.profile_end()
        nat.profile_begin()
        ev.hybrid_mask_sweep(model, feats, pats)
        stages, launches = nat.profile_end()
    names = [s for s, _ in stages]
    assert names.count("sweep.shared") == 1 and names.count("sweep.tail") == 1
    fwd_single = [k for st, k, *_ in single if st.startswith("fwd.")]
    fwd_sweep = [k for st, k, *_ in launches if st.startswith("fwd.")]
    assert fwd_single and fwd_sweep == fwd_single
    assert [k for _, k, *_ in launches].count("sweep_tail_kernel") == 1
    assert len(launches) <= len(fwd_single) + 3       # + prep, (pool,) tail: nothing grows with S
    kernels = [k for _, k, *_ in launches]
    if name == "m4_2d":          # the launch-lean L = 1 plan: nothing left to pool
        assert "fwd.l1" in names and "sweep_pool_kernel" not in kernels
    if name == "m3_general":     # the general plan: out_proj on every row, no pooled-plan stage
        assert "fwd.out_gemm" in names and not {"fwd.tail", "fwd.vbar_gemm", "fwd.pool_u"} & set(names)
        assert kernels.count("sweep_pool_kernel") == 1
    if name == "m2_l128":        # the pooled plan (a 256-key pair: without the fused tail)
        assert "fwd.vbar_gemm" in names and kernels.count("sweep_pool_kernel") == 1


def test_beyond_the_sweep_limits_runs_the_generic_path(mods):
    """HybridFusion.forward takes hidden_dim up to 1024, the sweep's tail up to 256: the evaluation
    serves such a model through the per-subset loop (no sweep launch) and agrees with the metrics
    of the model's own per-subset forwards."""
    fusion, ev, nat = mods
    torch.manual_seed(13)
    model = fusion.HybridFusion({"a": 12, "b": 20}, hidden_dim=512, num_classes=5, num_heads=4, dropout=0.1).cuda().eval()
    assert not ev.sweep_supported(model)
    g = torch.Generator().manual_seed(23)
    feats = {"a": torch.randn(6, 12, generator=g), "b": torch.randn(6, 20, generator=g)}
    labels = torch.arange(6) % 5
    batches = [({m: v[lo:lo + 3] for m, v in feats.items()}, labels[lo:lo + 3], torch.ones(3, 2)) for lo in (0, 3)]
    nat.profile_begin()
    res = ev.evaluate_missing_modalities(model, batches, ["a", "b"])
    stages, launches = nat.profile_end()
    assert "sweep.shared" not in [s for s, _ in stages] and "confusion_kernel" in [k for _, k, *_ in launches]
    assert list(res["all_combinations"]) == ["a", "b", "a+b"]
    with torch.no_grad():
        for key, sub in zip(res["all_combinations"], ev.modality_subsets(2)):
            mask = torch.zeros(3, 2, device="cuda")
            mask[:, list(sub)] = 1
            preds = []
            for bf, _, _ in batches:   # (the same calls the loop makes: the same bits)
                x = {m: (v.cuda() if i in sub else torch.zeros_like(v).cuda()) for i, (m, v) in enumerate(bf.items())}
                preds.append(model(x, mask).argmax(dim=1).cpu())
            acc = float((torch.cat(preds) == labels).double().mean())
            assert res["all_combinations"][key]["accuracy"] == pytest.approx(acc, abs=1e-12)
    with pytest.raises(RuntimeError, match="hidden_dim 512"):
        ev.hybrid_mask_sweep(model, {m: v.cuda() for m, v in feats.items()}, [[1, 1]])
