"""The per-step float64 comparison of tests/test_gpu_recurrence_envelope.py rejects the defects it
exists for, and the whole-tensor 1e-3 rule of tests/test_gpu_lstm.py / test_gpu_gru.py does not.

No device: "got" is the fp32 CPU oracle's own run of carry_h256 and tail3_h128 (network 0, both cells)
with one defect planted, and tests/_rec.compare with the committed C and CAP must reject it, while
the unplanted fp32 oracle passes:

  carry_scaled     the carry handed back in time scaled by 1.01 at every step more than 40 steps
                   before the last (carry_h256 only: tail3_h128 has 9 steps)
  dropped_partial  workgroup j = 1's partial (its 64 hidden units' gate rows of W_hh^T dgates)
                   missing from one row's gather at one backward step; every older step inherits it
  stale_parity     h_{t-2} in place of h_{t-1} for one 64-unit block of one row at one forward step
  tail_nan / tail_zero   the last instance's last row never written
  gate_swap        two gate slices of one unit swapped at one step
  gates_scaled     a 2e-4 relative scale on one (row, step) slice of gates

Each test prints the old whole-tensor rel_err of every tensor next to the verdict; for carry_scaled
and gates_scaled it asserts that the old rule (<= 1e-3) passes them: the reason for the new rule.
"""
import numpy as np
import pytest

from _rec import BY_NAME, C, CAP, CELLS, NGATES, TENSORS, assert_live, case_inputs, compare, old_rule, oracle, references

NAMES = ["carry_h256", "tail3_h128"]
OLD_TOL = 1e-3   # TOL of tests/test_gpu_lstm.py and tests/test_gpu_gru.py
BLOCK = slice(64, 128)   # hidden block j = 1


def clone(out):
    return {k: v.copy() for k, v in out.items()}


def plant_carry_scaled(name, cell):
    T = BY_NAME[name].T
    assert T > 41

    def hook(what, t, carry, dg, whh):
        if (T - 1) - t < 40:
            return carry
        return tuple(v * 1.01 for v in carry) if isinstance(carry, tuple) else carry * 1.01

    return oracle(cell, case_inputs(name, cell)[0], np.float32, bwd_hook=hook)


def plant_dropped_partial(name, cell):
    case = BY_NAME[name]
    step, row, H = case.T - 3, case.B - 1, case.H
    rows = np.concatenate([np.arange(g * H + BLOCK.start, g * H + BLOCK.stop) for g in range(NGATES[cell])])

    def hook(what, t, carry, dg, whh):
        if t != step:
            return carry
        rec = (carry[0] if isinstance(carry, tuple) else carry).copy()
        rec[row] -= dg[row, rows] @ whh[rows]
        return (rec, carry[1]) if isinstance(carry, tuple) else rec

    return oracle(cell, case_inputs(name, cell)[0], np.float32, bwd_hook=hook)


def plant_stale_parity(name, cell):
    case = BY_NAME[name]
    step, row = case.T - 4, case.B - 1

    def hook(what, t, prev, h):
        if t != step:
            return prev
        prev = prev.copy()
        prev[row, BLOCK] = h[row, t - 2, BLOCK]
        return prev

    return oracle(cell, case_inputs(name, cell)[0], np.float32, fwd_hook=hook)


def _tail(name, cell, value):
    got = clone(references(name, cell, 0)[1])
    for key in TENSORS[cell]:
        got[key][-1] = value
    return got


def plant_tail_nan(name, cell):
    return _tail(name, cell, np.nan)


def plant_tail_zero(name, cell):
    return _tail(name, cell, 0.0)


def plant_gate_swap(name, cell):
    case = BY_NAME[name]
    got = clone(references(name, cell, 0)[1])
    g = got["gates"][case.B - 1, case.T // 2]
    u, H = 70, case.H
    g[u], g[H + u] = g[H + u], g[u]
    return got


def plant_gates_scaled(name, cell):
    case = BY_NAME[name]
    got = clone(references(name, cell, 0)[1])
    got["gates"][0, case.T // 2] *= np.float32(1.0 + 2e-4)
    return got


OLD_RULE_PASSES = (plant_carry_scaled, plant_gates_scaled)
PLANTS = [(n, p) for n in NAMES for p in (plant_carry_scaled, plant_dropped_partial, plant_stale_parity, plant_tail_nan,
                                          plant_tail_zero, plant_gate_swap, plant_gates_scaled)
          if not (n == "tail3_h128" and p is plant_carry_scaled)]


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("name", NAMES)
def test_unplanted_fp32_oracle_passes(name, cell):
    ref64, ref32 = references(name, cell, 0)
    assert_live(ref64, f"{cell} {name}")
    bad, _ = compare(cell, ref32, ref64, ref32, f"BITE {cell} {name} unplanted", c=C, cap=CAP)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("name,plant", PLANTS, ids=[f"{n}-{p.__name__[6:]}" for n, p in PLANTS])
def test_planted_defect_is_rejected(name, plant, cell):
    ref64, ref32 = references(name, cell, 0)
    got = plant(name, cell)
    assert all(got[k].dtype == np.float32 for k in TENSORS[cell])
    tag = f"BITE {cell} {name} {plant.__name__[6:]}"
    bad, _ = compare(cell, got, ref64, ref32, tag, c=C, cap=CAP)
    old = old_rule(cell, got, ref64)
    print(f"{tag}: old whole-tensor rel_err " + ", ".join(f"{k} {v:.2e}" for k, v in old.items())
          + f" -> the old {OLD_TOL:g} rule {'passes' if all(v <= OLD_TOL for v in old.values()) else 'rejects'} it")
    print(f"{tag}: compare rejects\n  " + "\n  ".join(bad))
    assert bad, f"{plant.__name__}: the planted defect passed the float64 comparison"
    if plant in OLD_RULE_PASSES:
        assert all(v <= OLD_TOL for v in old.values()), (tag, old)
