"""The standard evaluation without a GPU: the metrics from hand-built device states (known-answer
bins, the empty-bin skip, MCE = 0 when every bin is empty, bad labels), the result and JSON keys,
the latency batch parsing, host-side validation of the C-ABI entry points (error codes before any
launch), the operator's fake kernel, and the float64 oracle of tests/_evalmetrics.py against the
reference's own numbers in the fixture."""
import inspect
import json

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

from _evalmetrics import (HEAD_WORDS, bins_of, build_state, case, check_preconditions, edges64, fixture,
                          fixture_margins, oracle_metrics, oracle_rows, oracle_state, state_fields)

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


# ------------------------------------------------------------------ metrics from a hand-built state
def test_known_answer_bins(ev):
    # 10 samples, 2 classes, 4 bins; bin 1 is empty and must be skipped
    st = build_state(2, 4, samples=10, correct=7, calls=2, loss_sum=1.5, nll_sum=8.0,
                     confusion=[[4, 1], [2, 3]], bin_count=[2, 0, 3, 5], bin_correct=[1, 0, 2, 4],
                     bin_conf_sum=[0.4, 0.0, 1.8, 4.5])
    m = ev.metrics_from_state(st, 2, 4)
    assert list(m) == ["accuracy", "f1_macro", "loss", "nll", "ece", "mce", "num_samples", "confusion",
                       "per_class_accuracy", "bins"]
    assert m["accuracy"] == 0.7 and m["num_samples"] == 10
    assert m["loss"] == 0.75 and m["nll"] == 0.8
    # gaps: |0.5 - 0.2|, skipped, |2/3 - 0.6|, |0.8 - 0.9|
    gaps = [0.3, abs(2 / 3 - 0.6), 0.1]
    assert m["ece"] == pytest.approx(0.2 * gaps[0] + 0.3 * gaps[1] + 0.5 * gaps[2], abs=1e-15)
    assert m["mce"] == pytest.approx(0.3, abs=1e-15)
    f1 = np.mean([2 * 4 / (5 + 6), 2 * 3 / (5 + 4)])
    assert m["f1_macro"] == pytest.approx(f1, abs=1e-15)
    assert np.array_equal(m["confusion"], [[4, 1], [2, 3]]) and m["confusion"].dtype == np.int64
    assert np.allclose(m["per_class_accuracy"], [0.8, 0.6], atol=1e-15)
    assert list(m["bins"]) == ["count", "accuracy", "confidence"]
    assert np.array_equal(m["bins"]["count"], [2, 0, 3, 5])
    assert np.allclose(m["bins"]["accuracy"], [0.5, 0.0, 2 / 3, 0.8], atol=1e-15)
    assert np.allclose(m["bins"]["confidence"], [0.2, 0.0, 0.6, 0.9], atol=1e-15)
    # a torch tensor is taken as well
    assert ev.metrics_from_state(torch.from_numpy(st), 2, 4)["ece"] == m["ece"]


def test_all_bins_empty_gives_zero_mce_and_nan_loss(ev):
    # three rows, each with a NaN softmax: in no bin, loss and NLL NaN
    st = build_state(3, 5, samples=3, correct=1, calls=1, nan_rows=3, loss_sum=float("nan"), nll_sum=float("nan"),
                     confusion=[[1, 0, 0], [1, 0, 0], [0, 1, 0]])
    m = ev.metrics_from_state(st, 3, 5)
    assert m["mce"] == 0.0 and m["ece"] == 0.0
    assert np.isnan(m["loss"]) and np.isnan(m["nll"])
    assert m["accuracy"] == pytest.approx(1 / 3)


def test_state_errors(ev):
    with pytest.raises(ValueError, match="outside"):
        ev.metrics_from_state(build_state(2, 3, samples=4, calls=1, bad=2), 2, 3)
    with pytest.raises(ValueError, match="no samples"):
        ev.metrics_from_state(build_state(2, 3), 2, 3)
    with pytest.raises(ValueError, match="words"):
        ev.metrics_from_state(np.zeros(5, np.int64), 2, 3)
    with pytest.raises(ValueError):
        ev.EvalAccumulator(0, device="cpu")
    with pytest.raises(ValueError):
        ev.EvalAccumulator(5, 257, device="cpu")


def test_accumulator_layout_and_device_requirement(ev, pkg_on_path):
    import mmf_ops
    acc = ev.EvalAccumulator(7, 15, device="cpu")
    assert acc.state.dtype == torch.int64 and acc.state.shape == (HEAD_WORDS + 49 + 45,)
    assert mmf_ops.eval_state_words(7, 15) == HEAD_WORDS + 49 + 45 == mmf_ops.EVAL_HEAD_WORDS + 94
    assert torch.equal(acc.edges, torch.linspace(0.0, 1.0, steps=16))
    with pytest.raises(RuntimeError, match="cuda"):   # no CPU fall-back
        acc.update(torch.zeros(4, 7), torch.zeros(4, dtype=torch.int64))


# ------------------------------------------------------------------ interface
def test_signatures(ev):
    sig = inspect.signature(ev.evaluate_model)
    assert list(sig.parameters) == ["model", "dataloader", "device", "return_predictions", "include_logits", "num_bins",
                                    "temperature"]
    assert sig.parameters["num_bins"].default == 15 and sig.parameters["device"].default == "cuda"
    assert list(inspect.signature(ev.measure_inference_latency).parameters) == ["model", "dataloader", "device", "warmup"]
    assert list(inspect.signature(ev.standard_evaluation).parameters)[:7] == [
        "model", "dataloader", "modality_names", "num_bins", "output_dir", "dataset_name", "fusion_type"]
    assert list(inspect.signature(ev.EvalAccumulator.update).parameters) == ["self", "logits", "labels", "temperature",
                                                                             "keep_predictions"]


def test_latency_batch_parsing(ev):
    feats = {"a": torch.zeros(3, 2)}
    assert ev._parse_latency_batch(feats) == (feats, None, None)
    y, m = torch.zeros(3), torch.ones(3, 1)
    assert ev._parse_latency_batch((feats, y, m)) == (feats, y, m)
    assert ev._parse_latency_batch([feats]) == (feats, None, None)
    assert ev._parse_latency_batch((feats, y)) == (feats, y, None)
    assert ev._parse_latency_batch(torch.zeros(3)) is None
    assert ev._parse_latency_batch(()) is None and ev._parse_latency_batch((y, feats)) is None
    assert ev._infer_batch_size(y, feats) == 3 and ev._infer_batch_size(None, feats) == 3
    assert ev._infer_batch_size(None, {"a": "text"}) is None


def test_latency_skips_unusable_batches_on_the_host(ev, capsys):
    model = torch.nn.Identity()
    out = ev.measure_inference_latency(model, [torch.zeros(3), (), {}, ({"a": "text"}, None)], device="cpu")
    assert out == (0.0, 0.0)
    text = capsys.readouterr().out
    assert text.count("Unable to parse batch") == 2 and text.count("Unable to infer batch size") == 2


def test_plots_and_json(ev, tmp_path):
    bins = {"count": np.array([2, 0, 3, 5]), "accuracy": np.array([0.5, 0.0, 2 / 3, 0.8]),
            "confidence": np.array([0.2, 0.0, 0.6, 0.9])}
    path = ev.reliability_diagram(bins, tmp_path / "plots" / "calibration.png")
    assert path == tmp_path / "plots" / "calibration.png" and path.stat().st_size > 1000
    with pytest.raises(ValueError):
        ev.reliability_diagram({"count": [1, 2], "accuracy": [0.5], "confidence": [0.5, 0.5]}, tmp_path / "x.png")
    out = ev.save_results_json({"ece": 0.25, "dataset": None}, tmp_path / "deep" / "r.json")
    assert json.loads(out.read_text()) == {"ece": 0.25, "dataset": None}
    # the reference's cases for "nothing to draw"
    assert ev.generate_attention_visualization(torch.nn.Identity(), [], [], tmp_path / "a.png", "cpu") is None
    assert ev.generate_attention_visualization(torch.nn.Identity(), [], ["a"], tmp_path / "a.png", "cpu") is None
    assert ev.attention_matrix(torch.nn.Identity(), {}, torch.ones(1, 1), []) is None
    assert ev.attention_matrix(torch.nn.Identity(), {}, torch.ones(1, 1), ["a"]) is None   # (TypeError: no return_attention)

    class Maps(torch.nn.Module):
        def forward(self, features, mask, return_attention=False):
            maps = {"a_to_b": torch.full((2, 1, 3), 0.25), "b_to_a": torch.full((2, 3, 1), 0.5), "a_to_zz": torch.ones(1),
                    "other": torch.ones(1)}
            return torch.zeros(2, 3), {"attention_maps": maps}

    got = ev.attention_matrix(Maps(), {}, torch.ones(2, 2), ["a", "b"])
    assert got.dtype == np.float32 and np.array_equal(got, np.array([[0, 0.25], [0.5, 0]], np.float32))


def test_standard_evaluation_json_keys(ev, tmp_path, monkeypatch):
    """The dicts and files of src/eval.py:598-611, 642-656, with the device walk and the latency
    replaced by a hand-built state (the GPU test runs the real ones)."""
    st = build_state(2, 4, samples=10, correct=7, calls=2, loss_sum=1.5, nll_sum=8.0, confusion=[[4, 1], [2, 3]],
                     bin_count=[2, 0, 3, 5], bin_correct=[1, 0, 2, 4], bin_conf_sum=[0.4, 0.0, 1.8, 4.5])
    monkeypatch.setattr(ev, "_evaluate", lambda *a, **k: (ev.metrics_from_state(st, 2, 4), None))
    monkeypatch.setattr(ev, "measure_inference_latency", lambda *a, **k: (1.25, 0.5))
    std, unc = ev.standard_evaluation(torch.nn.Identity(), [], ["a", "b"], num_bins=4, output_dir=tmp_path / "out",
                                      dataset_name="toy", fusion_type="late")
    assert list(std) == ["dataset", "fusion_type", "test_accuracy", "test_f1_macro", "test_loss", "ece", "mce", "nll",
                         "inference_ms_mean", "inference_ms_std"]
    assert list(unc) == ["dataset", "fusion_type", "ece", "mce", "nll", "num_bins", "calibration_plot"]
    assert std["test_accuracy"] == 0.7 and std["test_loss"] == 0.75 and std["nll"] == 0.8 and std["inference_ms_mean"] == 1.25
    assert unc["num_bins"] == 4 and unc["calibration_plot"] == str(tmp_path / "out" / "calibration.png")
    assert json.loads((tmp_path / "out" / "evaluation_results.json").read_text()) == std
    assert json.loads((tmp_path / "out" / "uncertainty.json").read_text()) == unc
    assert (tmp_path / "out" / "calibration.png").exists() and not (tmp_path / "out" / "attention_viz.png").exists()
    std2, unc2 = ev.standard_evaluation(torch.nn.Identity(), [], ["a"], num_bins=4)
    assert unc2["calibration_plot"] is None and std2["fusion_type"] == "Identity" and std2["dataset"] is None


# ------------------------------------------------------------------ C-ABI validation
def test_limits_and_null_arguments_before_any_launch(nat):
    L = nat.lib()
    assert L.mmf_eval_state_bytes(7, 15) == 8 * (HEAD_WORDS + 49 + 45)
    assert L.mmf_eval_state_bytes(1024, 256) == 8 * (HEAD_WORDS + 1024 * 1024 + 768)
    for C, nb in ((0, 15), (1025, 15), (7, 0), (7, 257)):
        assert L.mmf_eval_state_bytes(C, nb) == 0
        assert L.mmf_eval_workspace_bytes(4, C, nb) == 0
        assert L.mmf_eval_accumulate(4, C, nb, None, None, None, None, None, None, None, None, None) == ELIMIT
        assert b"limits" in L.mmf_last_error()
    assert L.mmf_eval_workspace_bytes(-1, 7, 15) == 0 and L.mmf_eval_workspace_bytes((1 << 24) + 1, 7, 15) == 0
    assert 12 * 1000 <= L.mmf_eval_workspace_bytes(1000, 7, 15) <= 12 * 1000 + 1024
    assert L.mmf_eval_workspace_bytes(1 << 24, 1024, 256) >= 12 << 24
    assert L.mmf_eval_accumulate(-1, 7, 15, None, None, None, None, None, None, None, None, None) == ELIMIT
    assert L.mmf_eval_accumulate((1 << 24) + 1, 7, 15, None, None, None, None, None, None, None, None, None) == ELIMIT
    assert L.mmf_eval_accumulate(4, 7, 15, None, None, None, None, None, None, None, None, None) == EINVAL
    assert b"null argument" in L.mmf_last_error()


# ------------------------------------------------------------------ the fake kernel
def test_fake_kernel(pkg_on_path):
    import mmf_ops
    with FakeTensorMode(), torch.device("cuda"):
        lg = torch.randn(4, 7)
        y = torch.zeros(4, dtype=torch.int64)
        state = torch.zeros(mmf_ops.eval_state_words(7, 15), dtype=torch.int64)
        preds, conf = torch.empty(4, dtype=torch.int64), torch.empty(4)
        out = torch.ops.mmfusion.eval_accumulate(lg, y, torch.linspace(0, 1, 16), torch.ones(1), state, preds, conf)
        assert out is None and state.dtype == torch.int64 and state.device.type == "cuda"
        assert torch.ops.mmfusion.eval_accumulate(lg, y, torch.linspace(0, 1, 16), None, state, None, None) is None
    schema = str(torch.ops.mmfusion.eval_accumulate.default._schema)
    assert "Tensor? temperature" in schema and schema.count("!") == 3 and schema.endswith("-> ()")


# ------------------------------------------------------------------ the oracle
def test_oracle_binning_at_the_edges():
    e = edges64(4)
    conf = np.array([0.0, 0.25, 0.4999, 0.5, 0.75, 1.0, np.nan, 0.9999999])
    assert list(bins_of(conf, 4)) == [0, 1, 1, 2, 3, 3, -1, 3]
    assert e[0] == 0.0 and e[-1] == 1.0
    # equal logits over 2^k classes: exactly 2^-k, in the bin it is the lower edge of
    r = oracle_rows(np.zeros((1, 4), np.float32), np.array([0]), 4)
    assert r["conf"][0] == 0.25 and r["bin"][0] == 1 and r["preds"][0] == 0


def test_oracle_state_round_trip():
    a, b = case(5, 3, 4), case(9, 3, 4, seed=1)
    bad = np.array(b[1])
    bad[2] = 3
    st = oracle_state([a, (b[0], bad)], 4)
    assert st["samples"] == 13 and st["bad"] == 1 and st["calls"] == 2 and st["confusion"].sum() == 13
    assert st["bin_count"].sum() == 13 and st["correct"] == np.trace(st["confusion"])
    w = build_state(3, 4, **st)
    back = state_fields(w, 3, 4)
    for k, v in st.items():
        assert np.array_equal(np.asarray(back[k]), np.asarray(v)), k


def test_case_builder_meets_its_preconditions():
    for B, C, nb in ((1, 1, 1), (63, 2, 15), (65, 65, 64), (257, 1024, 64)):
        logits, labels = case(B, C, nb)
        assert logits.shape == (B, C) and labels.shape == (B,)
        r = check_preconditions(logits, labels, nb)
        assert not r["nan"].any()
    with pytest.raises(AssertionError, match="from an edge"):
        check_preconditions(np.array([[np.log(3.0), 0.0]], np.float32), np.array([0]), 4)   # sigmoid(ln 3) = 0.75


def test_oracle_reproduces_the_reference_numbers(ev):
    fx = fixture()
    nb = int(fx["num_bins"][0])
    m = fixture_margins(fx["logits"], fx["labels"], nb)
    assert m["gap"] >= 1e-2 and m["edge"] >= 1e-3 and m["populated"] >= 5 and m["mixed"] >= 3, m
    r = oracle_rows(fx["logits"], fx["labels"], nb)
    assert np.array_equal(r["preds"], fx["preds"])
    assert np.abs(r["conf"] - fx["confidences"]).max() <= 4 * 2.0 ** -24   # the reference's float32 softmax
    got = oracle_metrics(fx["logits"], fx["labels"], nb, fx["batches"])
    assert got["accuracy"] == float(fx["accuracy"][0])
    # the reference sums in float32: a few roundings of numbers of size <= max(1, nll)
    for k in ("loss", "nll", "ece", "mce"):
        assert got[k] == pytest.approx(float(fx[k][0]), abs=1e-6), k
    # and the package's host metrics from the oracle's state agree with both
    st = oracle_state([(fx["logits"][lo:lo + n], fx["labels"][lo:lo + n])
                       for lo, n in zip(np.cumsum([0] + list(fx["batches"][:-1])), fx["batches"])], nb)
    res = ev.metrics_from_state(build_state(7, nb, **st), 7, nb)
    assert res["accuracy"] == float(fx["accuracy"][0])
    assert res["f1_macro"] == pytest.approx(float(fx["f1_macro"][0]), abs=1e-12)
    for k in ("loss", "nll", "ece", "mce"):
        assert res[k] == pytest.approx(got[k], abs=1e-12), k
