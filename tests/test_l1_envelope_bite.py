"""The float64 comparison of tests/test_gpu_l1_envelope.py rejects the defects it exists for.

No device: "got" is the fp32 CPU oracle's own train step on l1_m4_ragged and l1_m2_b260 with one
defect planted -- the last sample's input gradient never written, one 32 x 32 tile of a value
projection's weight gradient never written, the weight gradient's second 256-row chunk left out of
classifier.0.weight, one sample's logits off by 2e-4 -- and tests/_l1.compare_step (the rule
the GPU module applies: close_sliced with C and CAP of tests/test_gpu_attn_headdims.py) must reject
it, while the unplanted fp32 oracle passes.  The fp32 oracle stands in for the device all the way:
the float64 reference takes its ReLU decisions within rounding of zero as it takes the device's
(tests/_util.device_relu_gates).
"""
import functools

import pytest
import torch

from _l1 import BY_NAME, compare_step, oracle_step
from _util import device_relu_gates
from cases import hybrid_inputs, hybrid_state

NAMES = ["l1_m4_ragged", "l1_m2_b260"]


@functools.lru_cache(maxsize=None)
def references(name):
    """(float64 oracle, fp32 oracle, the ReLU gates), computed once and left unchanged."""
    case = BY_NAME[name]
    sd = hybrid_state(case.names, case.dims, case.hidden, case.classes, case.seed)
    taps64, taps32 = {}, {}
    oracle_step(case, torch.float64, taps=taps64)
    oracle_step(case, torch.float32, taps=taps32)
    wts = {m: torch.from_numpy(sd[f"projections.{m}.0.weight"]) for m in case.names}
    wts["cls"] = torch.from_numpy(sd["classifier.0.weight"])
    acts = {layer: taps32[f"a/{layer}"].detach() for layer in wts}   # (ReLU' as value > 0, as on the device)
    gates, counts = device_relu_gates(taps64, wts, acts)
    print(f"BITE {name} pre-activations in the band: {counts}")
    return (oracle_step(case, torch.float64, relu_gate=gates), oracle_step(case, torch.float32, relu_gate=gates),
            gates)


def clone(out):
    return {k: v.clone() for k, v in out.items()}


def plant_dx_row(name):   # the last sample's dX row of every modality never written
    case = BY_NAME[name]
    got = clone(references(name)[1])
    _, mask_np, _ = hybrid_inputs(case)
    assert mask_np[-1].any()   # (a live sample: its rows are nonzero)
    for m in case.names:
        got[f"dx/{m}"][-1] = 0.0
    return got


def plant_wv_tile(name):   # the last row tile (rows 32.., or all of them at H <= 32) of one dW_v never written
    case = BY_NAME[name]
    got = clone(references(name)[1])
    n0 = 32 * ((case.hidden - 1) // 32)
    key = f"attention_modules.{case.names[1]}_to_{case.names[0]}.value_proj.weight"
    assert bool(got[key][n0:n0 + 32, 0:32].any())
    got[key][n0:n0 + 32, 0:32] = 0.0
    return got


def plant_cls_rows(name):   # samples 256.. left out of classifier.0.weight's gradient (the second chunk)
    case = BY_NAME[name]
    assert case.batch > 256
    got = clone(references(name)[1])
    part = oracle_step(case, torch.float32, relu_gate=references(name)[2], rows=256)
    got["classifier.0.weight"] = part["classifier.0.weight"].clone()
    return got


def plant_logits(name):   # one live sample's logits off by 2e-4 of the sample's maximum
    got = clone(references(name)[1])
    got["logits"][1] *= 1.0 + 2e-4
    return got


PLANTS = [("l1_m4_ragged", plant_dx_row), ("l1_m4_ragged", plant_wv_tile), ("l1_m4_ragged", plant_logits),
          ("l1_m2_b260", plant_dx_row), ("l1_m2_b260", plant_wv_tile), ("l1_m2_b260", plant_cls_rows),
          ("l1_m2_b260", plant_logits)]


@pytest.mark.parametrize("name", NAMES)
def test_unplanted_fp32_oracle_passes(name):
    ref64, ref32, _ = references(name)
    bad = compare_step(BY_NAME[name], ref32, ref64, ref32, f"{name} unplanted")
    assert not bad, "\n".join(bad)


def test_partial_loss_is_the_rows_left_out():
    """The rows= form of the oracle step at rows = batch is the step itself (the planted
    classifier.0.weight is the gradient without samples 256.., nothing else)."""
    name = "l1_m2_b260"
    case = BY_NAME[name]
    _, ref32, gates = references(name)
    whole = oracle_step(case, torch.float32, relu_gate=gates, rows=case.batch)
    g, r = whole["classifier.0.weight"], ref32["classifier.0.weight"]
    assert float((g - r).abs().max()) <= 1e-6 * float(r.abs().max())
    part = oracle_step(case, torch.float32, relu_gate=gates, rows=256)["classifier.0.weight"]
    assert float((part - r).abs().max()) > 1e-4 * float(r.abs().max())


@pytest.mark.parametrize("name,plant", PLANTS, ids=[f"{n}-{p.__name__}" for n, p in PLANTS])
def test_planted_defect_is_rejected(name, plant):
    ref64, ref32, _ = references(name)
    got = plant(name)
    bad = compare_step(BY_NAME[name], got, ref64, ref32, f"{name} {plant.__name__}")
    print(f"BITE {name} {plant.__name__}: compare_step rejects\n  " + "\n  ".join(bad))
    assert bad, f"{plant.__name__}: the planted defect passed the float64 comparison"
