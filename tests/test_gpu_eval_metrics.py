"""GPU tests of the standard evaluation (mmf_eval_accumulate, torch.ops.mmfusion.eval_accumulate,
mmf_eval.EvalAccumulator / evaluate_model / measure_inference_latency / attention_matrix /
standard_evaluation).

Kernel against the float64 oracle of tests/_evalmetrics.py on the same float32 logits: predictions,
every counter, the confusion matrix and the bins exact; confidences within (C + 8) 2^-23; the
cross-entropy sums within that times max(1, max|logit|) per row; ECE / MCE by the rule of
tests/test_gpu_pamap2.py -- within mean / max |d conf| + 1e-6 while no sample changes bin, which is
asserted.  The cases meet the edge precondition (check_preconditions; tests/_evalmetrics.py says why
only interior edges count).  The reference fixture's margins and bounds are those its generator
documents (tests/golden/gen_eval_metrics.py)."""
import json

import numpy as np
import pytest
import torch

from _evalmetrics import (bins_of, case, ce_bound, check_preconditions, conf_bound, fixture, fixture_batches,
                          fixture_margins, fixture_model, fixture_names, oracle_metrics, oracle_rows, oracle_state,
                          state_fields)
from _util import close, diff_report

pytestmark = pytest.mark.gpu
INT_FIELDS = ("samples", "correct", "bad", "calls", "nan_rows", "reserved", "confusion", "bin_count", "bin_correct")


@pytest.fixture(scope="module")
def mods(pkg_on_path):
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible")
    import fusion
    import mmf_eval
    import mmf_native
    import mmf_ops  # noqa: F401
    mmf_native.lib()
    prev = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision("highest")
    yield fusion, mmf_eval
    torch.set_float32_matmul_precision(prev)


def _accumulate(ev, calls, C, nb, temperature=None):
    """-> (the state's fields, per-call predictions, per-call confidences, the accumulator)."""
    acc = ev.EvalAccumulator(C, nb)
    preds, confs = [], []
    for logits, labels in calls:
        p, c = acc.update(torch.from_numpy(np.array(logits)).cuda(), torch.from_numpy(np.array(labels)).cuda(),
                          temperature, keep_predictions=True)
        preds.append(p)
        confs.append(c)
    words = acc.state.cpu().numpy()
    return (state_fields(words, C, nb), [p.cpu().numpy() for p in preds], [c.cpu().numpy() for c in confs], acc)


def _check_against_oracle(ev, calls, C, nb):
    rows = [check_preconditions(lg, y, nb) for lg, y in calls]
    got, preds, confs, acc = _accumulate(ev, calls, C, nb)
    want = oracle_state(calls, nb)
    want["reserved"] = 0
    for r, p, c in zip(rows, preds, confs):
        assert p.dtype == np.int64 and c.dtype == np.float32
        assert np.array_equal(p, r["preds"])
        dconf = np.abs(c.astype(np.float64) - r["conf"])
        print(f"C {C} bins {nb} B {p.size}: max|dconf| {dconf.max():.3e} (bound {conf_bound(C):.3e})")
        assert dconf.max() <= conf_bound(C)
        assert np.array_equal(bins_of(c.astype(np.float64), nb), r["bin"])   # no sample changes bin
    for k in INT_FIELDS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k
    bound = max(ce_bound(C, lg) for lg, _ in calls)
    n = want["samples"]
    print(f"  nll_sum {got['nll_sum']:.9e} vs {want['nll_sum']:.9e}, loss_sum {got['loss_sum']:.9e} vs "
          f"{want['loss_sum']:.9e}, per-row bound {bound:.3e}")
    assert abs(got["nll_sum"] - want["nll_sum"]) <= n * bound
    assert abs(got["loss_sum"] - want["loss_sum"]) <= len(calls) * bound   # (a sum of per-call means)
    for b in range(nb):
        assert abs(got["bin_conf_sum"][b] - want["bin_conf_sum"][b]) <= max(1, int(want["bin_count"][b])) * conf_bound(C)
    # the metrics, against the reference's chain over all rows
    res = acc.result()
    lg = np.concatenate([c[0] for c in calls])
    y = np.concatenate([c[1] for c in calls])
    ref = oracle_metrics(lg, y, nb, [c[0].shape[0] for c in calls])
    dconf = np.abs(np.concatenate(confs).astype(np.float64) - np.concatenate([r["conf"] for r in rows]))
    assert res["accuracy"] == ref["accuracy"] and res["num_samples"] == y.size
    assert abs(res["nll"] - ref["nll"]) <= bound and abs(res["loss"] - ref["loss"]) <= bound
    assert abs(res["ece"] - ref["ece"]) <= dconf.mean() + 1e-6
    assert abs(res["mce"] - ref["mce"]) <= dconf.max() + 1e-6
    return res


# ------------------------------------------------------------------ kernel vs oracle
@pytest.mark.parametrize("nb", [1, 2, 15, 64])
@pytest.mark.parametrize("C", [1, 2, 7, 65, 1024])
@pytest.mark.parametrize("B", [1, 63, 65, 257])
def test_kernel_against_oracle(mods, B, C, nb):
    _, ev = mods
    _check_against_oracle(ev, [case(B, C, nb)], C, nb)


def test_three_calls_into_one_state(mods):
    _, ev = mods
    calls = [case(63, 7, 15), case(1, 7, 15, seed=1), case(257, 7, 15, seed=2)]
    res = _check_against_oracle(ev, calls, 7, 15)
    assert res["num_samples"] == 321 and res["confusion"].sum() == 321


# ------------------------------------------------------------------ exact edges
@pytest.mark.parametrize("k", [1, 2, 3])
def test_equal_logits_land_on_their_lower_edge(mods, k):
    _, ev = mods
    C = 2 ** k
    logits = np.full((5, C), 0.75, np.float32)
    labels = np.array([0, 1, 0, C - 1, 0], np.int64)
    got, preds, confs, _ = _accumulate(ev, [(logits, labels)], C, C)
    assert np.array_equal(confs[0], np.full(5, 2.0 ** -k, np.float32))     # exactly 2^-k
    assert np.array_equal(preds[0], np.zeros(5, np.int64))                # the lowest index of the tie
    want = np.zeros(C, np.int64)
    want[1] = 5                                                           # edges[1] == 2^-k <= c < edges[2]
    assert np.array_equal(got["bin_count"], want)
    assert got["bin_correct"][1] == 3 and got["correct"] == 3
    assert got["bin_conf_sum"][1] == 5 * 2.0 ** -k
    assert got["nll_sum"] == pytest.approx(5 * k * np.log(2.0), abs=5 * ce_bound(C, logits))


def test_confidence_one_falls_in_the_closed_last_bin(mods):
    _, ev = mods
    logits = np.zeros((3, 6), np.float32)
    logits[0, 2] = logits[1, 5] = logits[2, 0] = 200.0
    labels = np.array([2, 5, 1], np.int64)
    got, preds, confs, _ = _accumulate(ev, [(logits, labels)], 6, 15)
    assert np.array_equal(confs[0], np.ones(3, np.float32)) and list(preds[0]) == [2, 5, 0]
    assert got["bin_count"][14] == 3 and got["bin_count"].sum() == 3 and got["bin_correct"][14] == 2
    assert got["nll_sum"] == pytest.approx(200.0, abs=3 * ce_bound(6, logits))


# ------------------------------------------------------------------ other kernel cases
def test_ties_take_the_lowest_index(mods):
    _, ev = mods
    logits = np.array([[1, 3, 3, 0, 3], [2, 2, 2, 2, 2], [0, 1, 0, 1, -1], [-5, -7, -5, -9, -5]], np.float32)
    logits = np.tile(logits, (1, 14))   # 70 classes: the ties repeat across the lanes' strides
    labels = np.array([1, 0, 3, 2], np.int64)
    got, preds, _, _ = _accumulate(ev, [(logits, labels)], 70, 15)
    want = torch.argmax(torch.from_numpy(logits), dim=1).numpy()
    assert list(want) == [1, 0, 1, 0] and np.array_equal(preds[0], want)
    assert got["correct"] == 2 and got["confusion"][3, 1] == 1 and got["confusion"][2, 0] == 1


def test_nan_rows(mods):
    _, ev = mods
    logits, labels = (np.array(a) for a in case(9, 7, 15))
    logits[2, 3] = np.nan            # a NaN: the argmax, and a NaN softmax
    logits[4, 5] = np.inf            # inf - inf
    logits[6, :] = -np.inf           # -inf + inf
    r = oracle_rows(logits, labels, 15)
    assert list(np.flatnonzero(r["nan"])) == [2, 4, 6] and list(r["preds"][[2, 4, 6]]) == [3, 5, 0]
    got, preds, confs, acc = _accumulate(ev, [(logits, labels)], 7, 15)
    want = oracle_state([(logits, labels)], 15)
    want["reserved"] = 0
    assert np.array_equal(preds[0], r["preds"])
    assert np.array_equal(np.isnan(confs[0]), r["nan"])
    for k in INT_FIELDS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k
    assert got["nan_rows"] == 3 and got["bin_count"].sum() == 6 and got["samples"] == 9
    assert np.isnan(got["nll_sum"]) and np.isnan(got["loss_sum"])
    res = acc.result()
    assert np.isnan(res["loss"]) and np.isnan(res["nll"]) and np.isfinite(res["ece"]) and res["num_samples"] == 9


def test_out_of_range_labels_touch_nothing_else(mods):
    _, ev = mods
    logits, labels = (np.array(a) for a in case(12, 7, 15))
    bad = labels.copy()
    bad[[1, 5, 8]] = [-1, 7, 1 << 40]
    keep = np.ones(12, bool)
    keep[[1, 5, 8]] = False
    got, preds, confs, acc = _accumulate(ev, [(logits, bad)], 7, 15)
    want = oracle_state([(logits, bad)], 15)
    want["reserved"] = 0
    for k in INT_FIELDS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k
    assert got["bad"] == 3 and got["samples"] == 9 and got["confusion"].sum() == 9 and got["bin_count"].sum() == 9
    # the counts are those of the good rows alone
    alone, _, _, _ = _accumulate(ev, [(logits[keep], labels[keep])], 7, 15)
    for k in ("correct", "confusion", "bin_count", "bin_correct"):
        assert np.array_equal(np.asarray(got[k]), np.asarray(alone[k])), k
    assert got["nll_sum"] == pytest.approx(alone["nll_sum"], abs=9 * ce_bound(7, logits))
    # predictions and confidences are still written for every row
    assert np.array_equal(preds[0], oracle_rows(logits, labels, 15)["preds"]) and np.isfinite(confs[0]).all()
    with pytest.raises(ValueError, match="3 label entries outside"):
        acc.result()


def test_device_temperature_equals_predivided_logits(mods):
    _, ev = mods
    logits, labels = case(65, 7, 15)
    T = np.float32(1.7)
    divided = (np.array(logits) / T).astype(np.float32)      # IEEE float32 division on the host
    want, wp, wc, _ = _accumulate(ev, [(divided, labels)], 7, 15)
    for temperature in (torch.tensor([1.7], device="cuda"), 1.7, torch.tensor(1.7)):
        got, gp, gc, _ = _accumulate(ev, [(logits, labels)], 7, 15, temperature)
        assert np.array_equal(gp[0], wp[0]) and np.array_equal(gc[0], wc[0])
        for k in want:
            assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), k
    plain, _, pc, _ = _accumulate(ev, [(logits, labels)], 7, 15)
    assert not np.array_equal(pc[0], wc[0])   # (the temperature did something)


def test_rerun_is_bit_identical(mods):
    _, ev = mods
    calls = [case(257, 65, 64), case(63, 65, 64, seed=1)]
    states = []
    for _ in range(2):
        acc = ev.EvalAccumulator(65, 64)
        for lg, y in calls:
            acc.update(torch.from_numpy(np.array(lg)).cuda(), torch.from_numpy(np.array(y)).cuda())
        states.append(acc.state.clone())
    assert torch.equal(states[0], states[1])


def test_limits_are_refused_before_a_launch(mods):
    _, ev = mods
    import mmf_ops
    y = torch.zeros(2, dtype=torch.int64, device="cuda")
    edges = torch.linspace(0, 1, 16).cuda()
    state = torch.zeros(mmf_ops.eval_state_words(7, 15), dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="outside"):
        torch.ops.mmfusion.eval_accumulate(torch.zeros(2, 1025, device="cuda"), y, edges, None, state, None, None)
    with pytest.raises(RuntimeError, match="outside"):
        torch.ops.mmfusion.eval_accumulate(torch.zeros(2, 7, device="cuda"), y, torch.linspace(0, 1, 258).cuda(), None,
                                           state, None, None)
    with pytest.raises(RuntimeError, match="words"):
        torch.ops.mmfusion.eval_accumulate(torch.zeros(2, 7, device="cuda"), y, edges, None, state[:-1].clone(), None, None)
    with pytest.raises(RuntimeError, match="float32"):
        torch.ops.mmfusion.eval_accumulate(torch.zeros(2, 7, device="cuda").double(), y, edges, None, state, None, None)
    assert int(state.abs().sum()) == 0
    # an empty batch is no call
    torch.ops.mmfusion.eval_accumulate(torch.zeros(0, 7, device="cuda"), y[:0], edges, None, state, None, None)
    assert int(state.abs().sum()) == 0
    with pytest.raises(ValueError):
        ev.EvalAccumulator(7, 15).update(torch.zeros(2, 8, device="cuda"), y)


# ------------------------------------------------------------------ the reference fixture
def test_reference_fixture_on_the_device(mods):
    fusion, ev = mods
    fx = fixture()
    nb = int(fx["num_bins"][0])
    m = fixture_margins(fx["logits"], fx["labels"], nb)
    assert m["gap"] >= 1e-2 and m["edge"] >= 1e-3 and m["populated"] >= 5 and m["mixed"] >= 3, m
    model = fixture_model(fusion, fx)
    metrics, (preds, labels, conf, logits) = ev.evaluate_model(model, fixture_batches(fx), return_predictions=True,
                                                               include_logits=True, num_bins=nb)
    assert close(logits, fx["logits"], 1e-3), diff_report(logits, fx["logits"], 1e-3)
    assert np.array_equal(preds.numpy(), fx["preds"]) and np.array_equal(labels.numpy(), fx["labels"])
    assert list(metrics) == ["accuracy", "f1_macro", "loss", "num_samples", "ece", "mce", "nll"]
    assert metrics["accuracy"] == float(fx["accuracy"][0]) and metrics["num_samples"] == 40
    assert metrics["f1_macro"] == pytest.approx(float(fx["f1_macro"][0]), abs=1e-12)
    for k in ("loss", "nll"):
        print(k, metrics[k], float(fx[k][0]))
        assert abs(metrics[k] - float(fx[k][0])) <= 1e-3 * abs(float(fx[k][0])), k
    ref_conf = fx["confidences"].astype(np.float64)
    dconf = np.abs(conf.numpy().astype(np.float64) - ref_conf)
    assert np.array_equal(bins_of(conf.numpy().astype(np.float64), nb), bins_of(ref_conf, nb))   # no sample changes bin
    print("ece", metrics["ece"], float(fx["ece"][0]), "mce", metrics["mce"], float(fx["mce"][0]), "dconf", dconf.max())
    assert abs(metrics["ece"] - float(fx["ece"][0])) <= dconf.mean() + 1e-6
    assert abs(metrics["mce"] - float(fx["mce"][0])) <= dconf.max() + 1e-6


# ------------------------------------------------------------------ evaluate_model and friends
def _config(fusion_type):
    enc = {"imu_hand": {"type": "sequence", "input_dim": 9, "encoder_type": "lstm", "num_layers": 1, "hidden_dim": 64},
           "imu_chest": {"type": "sequence", "input_dim": 6, "encoder_type": "lstm", "num_layers": 1, "hidden_dim": 64},
           "video": {"type": "frame", "input_dim": 24, "hidden_dim": 32}}
    return {"dataset": {"modalities": list(enc), "num_classes": 6},
            "model": {"fusion_type": fusion_type, "hidden_dim": 32, "output_dim": 32, "num_heads": 4, "dropout": 0.1,
                      "layer_norm": True, "encoders": enc}}


def _batches(n, seed, sizes):
    g = torch.Generator().manual_seed(seed)
    feats = {"imu_hand": torch.randn(n, 10, 9, generator=g), "imu_chest": torch.randn(n, 10, 6, generator=g),
             "video": torch.randn(n, 5, 24, generator=g)}
    labels = torch.randint(0, 6, (n,), generator=g)
    out, lo = [], 0
    for s in sizes:
        out.append(({m: v[lo:lo + s] for m, v in feats.items()}, labels[lo:lo + s], torch.ones(s, 3)))
        lo += s
    return out


@pytest.mark.parametrize("fusion_type", ["hybrid", "late"])
def test_evaluate_model_on_a_full_model(mods, fusion_type):
    """The metrics are those of the oracle over the model's own logits (LateFusion returns a tuple:
    its first element counts)."""
    _, ev = mods
    from harness import MultimodalFusionModel
    torch.manual_seed(21)
    model = MultimodalFusionModel.from_config(_config(fusion_type)).cuda().eval()
    sizes = [8, 8, 5]
    batches = _batches(21, 33, sizes)
    metrics, (preds, labels, conf, logits) = ev.evaluate_model(model, batches, return_predictions=True,
                                                               include_logits=True)
    assert preds.shape == labels.shape == conf.shape == (21,) and logits.shape == (21, 6)
    assert (preds.dtype, labels.dtype, conf.dtype, logits.dtype) == (torch.int64, torch.int64, torch.float32, torch.float32)
    assert all(t.device.type == "cpu" for t in (preds, labels, conf, logits))
    assert torch.equal(labels, torch.cat([b[1] for b in batches]))
    r = check_preconditions(logits.numpy(), labels.numpy(), 15)
    ref = oracle_metrics(logits.numpy(), labels.numpy(), 15, sizes)
    dconf = np.abs(conf.numpy().astype(np.float64) - r["conf"])
    bound = ce_bound(6, logits.numpy())
    assert np.array_equal(preds.numpy(), r["preds"]) and dconf.max() <= conf_bound(6)
    assert np.array_equal(bins_of(conf.numpy().astype(np.float64), 15), r["bin"])
    assert metrics["accuracy"] == ref["accuracy"] and metrics["num_samples"] == 21
    assert abs(metrics["loss"] - ref["loss"]) <= bound and abs(metrics["nll"] - ref["nll"]) <= bound
    assert abs(metrics["ece"] - ref["ece"]) <= dconf.mean() + 1e-6
    assert abs(metrics["mce"] - ref["mce"]) <= dconf.max() + 1e-6
    # without predictions: the dict alone, the same numbers; three predictions without the logits
    again = ev.evaluate_model(model, batches)
    assert again == metrics
    _, three = ev.evaluate_model(model, batches, return_predictions=True)
    assert len(three) == 3 and torch.equal(three[0], preds) and torch.equal(three[2], conf)
    with pytest.raises(ValueError, match="empty"):
        ev.evaluate_model(model, [])


def test_attention_matrix_against_the_attention_maps(mods):
    fusion, ev = mods
    from _sweep import CASES, build_hybrid, case_inputs
    c = CASES["m3_mixed_l"]
    model = build_hybrid(fusion, c)
    feats = {m: v.cuda() for m, v in case_inputs(c).items()}
    mask = torch.ones(c.batch, 3, device="cuda")
    got = ev.attention_matrix(model, feats, mask, c.names)
    with torch.no_grad():
        _, info = model(feats, mask, return_attention=True)
    want = np.zeros((3, 3), np.float32)
    for key, w in info["attention_maps"].items():
        q, k = key.split("_to_")
        want[c.names.index(q), c.names.index(k)] = float(w.double().mean())
    assert len(info["attention_maps"]) == 6 and got.shape == (3, 3) and got.dtype == np.float32
    assert np.abs(got - want).max() <= 1e-6 and (np.diag(got) == 0).all()
    assert len(set(np.round(got[want > 0], 4))) > 1            # (the key lengths differ: not one constant)
    # names the maps do not know contribute nothing; a reordering transposes accordingly
    sub = ev.attention_matrix(model, feats, mask, [c.names[1], "other", c.names[0]])
    assert sub[0, 2] == got[1, 0] and sub[2, 0] == got[0, 1] and sub[1].sum() == 0 and sub[:, 1].sum() == 0
    late = fusion.LateFusion({m: c.dims[m] for m in c.names}, hidden_dim=16, num_classes=4).cuda().eval()
    assert ev.attention_matrix(late, feats, mask, c.names) is None   # (TypeError: no return_attention)


def test_latency_is_measured_with_device_events(mods, capsys):
    _, ev = mods
    from harness import MultimodalFusionModel
    torch.manual_seed(22)
    model = MultimodalFusionModel.from_config(_config("hybrid")).cuda().eval()
    batches = _batches(16, 34, [8, 8])
    mean, std = ev.measure_inference_latency(model, batches)
    assert np.isfinite(mean) and np.isfinite(std) and mean > 0 and std >= 0
    # a features-only batch gets an all-ones mask; unparsable ones are skipped with the reference's warnings
    mean2, _ = ev.measure_inference_latency(model, [batches[0][0], torch.zeros(3), ()])
    assert mean2 > 0 and capsys.readouterr().out.count("Unable to parse batch") == 2
    assert ev.measure_inference_latency(model, [torch.zeros(3), (), ({}, None, None)]) == (0.0, 0.0)


def test_standard_evaluation_writes_both_json_files(mods, tmp_path):
    _, ev = mods
    from harness import MultimodalFusionModel
    torch.manual_seed(23)
    model = MultimodalFusionModel.from_config(_config("hybrid")).cuda().eval()
    batches = _batches(21, 35, [8, 8, 5])
    names = list(model.encoders)
    std, unc = ev.standard_evaluation(model, batches, names, num_bins=10, output_dir=tmp_path, dataset_name="toy")
    assert list(std) == ["dataset", "fusion_type", "test_accuracy", "test_f1_macro", "test_loss", "ece", "mce", "nll",
                         "inference_ms_mean", "inference_ms_std", "attention_plot"]
    assert list(unc) == ["dataset", "fusion_type", "ece", "mce", "nll", "num_bins", "calibration_plot"]
    assert std["dataset"] == "toy" and std["fusion_type"] == "hybrid" and unc["num_bins"] == 10
    assert json.loads((tmp_path / "evaluation_results.json").read_text()) == std
    assert json.loads((tmp_path / "uncertainty.json").read_text()) == unc
    assert (tmp_path / "calibration.png").stat().st_size > 1000 and unc["calibration_plot"] == str(tmp_path / "calibration.png")
    assert (tmp_path / "attention_viz.png").stat().st_size > 1000
    metrics = ev.evaluate_model(model, batches, num_bins=10)
    assert (std["test_accuracy"], std["test_f1_macro"], std["test_loss"], std["ece"], std["mce"], std["nll"]) == tuple(
        metrics[k] for k in ("accuracy", "f1_macro", "loss", "ece", "mce", "nll"))
    assert std["inference_ms_mean"] > 0
    # nothing is written without an output directory, and a late-fusion model draws no attention map
    torch.manual_seed(24)
    late = MultimodalFusionModel.from_config(_config("late")).cuda().eval()
    std2, unc2 = ev.standard_evaluation(late, batches, names)
    assert std2["fusion_type"] == "late" and "attention_plot" not in std2 and unc2["calibration_plot"] is None
    assert std2["dataset"] is None and unc2["num_bins"] == 15
