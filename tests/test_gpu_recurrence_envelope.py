"""The persistent LSTM / GRU recurrence (csrc/recurrence.h, lstm.hip, gru.hip) per time step and
across the launch envelope recurrence_plan admits, against float64.

tests/test_gpu_lstm.py and tests/test_gpu_gru.py bound max|diff| by 1e-3 of the whole tensor's
maximum: a BPTT step whose gradient is a thousandth of the largest is unchecked there, and so is
anything below 1e-3 in the forward.  They stop at 4 networks and 12 instances, reach the <128>
forward only at T = 1 (h_{t-1} = 0: the recurrent matvec multiplies zeros), never put a 2- or 3-row
tail instance on H = 128 or 192, never run T = 2 or 3 and never use a first row beyond 8.  The cases
of tests/_rec.py are the smallest shapes that reach each of those, both cells through the raw C ABI:

  inst32_h64 (8, 16, 6, 64)      LMAX_N and LMAX_I: 32 instances, 32 workgroups
  n8_h256 (8, 8, 6, 256)         8 networks x G = 4: 64 workgroups, 16 instances
  b128_h64 (1, 128, 5, 64)       one network, first rows up to 124, 32 instances
  tail3_h128 (2, 7, 9, 128)      4 + 3 rows; the <128> matvec against a nonzero h
  tail2_h192 (1, 6, 9, 192)      4 + 2 rows, KP = 12
  single3_h256 (3, 3, 9, 256)    one partial instance per network
  parity_t2, parity_t3 (1, 4, 2 | 3, 256)    the first reuse of each parity buffer
  carry_h64, carry_h256 (1, 2, 64, 64 | 256) dh on the last step only: every older step is pure carry
  long_h256 (1, 2, 1024, 256)    the C3 length with two rows, dh on every step
  saturated_h64 (1, 2, 16, 64)   xproj x 20: exp overflow / rcp(inf); all outputs finite

Per case: every (row, step) slice of the float64 reference is alive (tests/_rec.assert_live, before
the device is touched); the timeout word is 0 after each launch; h, c, gates and dgates of networks 0,
n / 2 and n - 1 go by tests/_rec.compare (close_sliced, one slice per (row, step), C and CAP of
tests/_rec.py); no network's output equals another's.  Without a reference, bit for bit: a row's
result does not depend on the instance it lands in (B = 9 as 4 + 4 + 1 rows against nine B = 1
launches), and a rerun of n8_h256 gives the same bits.  At module level SequenceEncoder('lstm') and
GRUSequenceEncoder (B = 7, T = 19, D = 11, H = 128, 2 layers, ragged lengths) against float64 and
fp32 torch.nn.LSTM / GRU + Linear on the CPU under the same rule, one slice per sample and per
parameter.  tests/test_recurrence_bite.py shows that the rule rejects the defects these cases exist
to find.

Measured worst e_dev / max(e_32, 2^-24) per case, LSTM / GRU (profiles/recurrence_envelope/pytest.log):
    inst32_h64 4.92 / 3.86     n8_h256 3.05 / 4.71       b128_h64 7.46 / 3.69     tail3_h128 5.63 / 3.58
    tail2_h192 2.81 / 2.51     single3_h256 3.29 / 3.58  parity_t2 3.10 / 2.40    parity_t3 2.79 / 2.46
    carry_h64 4.81 / 7.47      carry_h256 5.48 / 3.06    long_h256 3.73 / 3.91    saturated_h64 3.74 / 3.58
    the encoders 5.69 / 4.10 (the encoding of one sample; every parameter gradient <= 4.59)
The worst, 7.47 (GRU carry_h64 dgates) and 7.46 (LSTM b128_h64 dgates), are in tensors whose largest
device error is 1.3e-6 and 6.0e-7 of a slice's maximum: the fp32 oracle happens to sit nearer to
float64 in one slice.  C = 16, the next power of two at or above twice the worst, for the C ABI and
the modules alike.  The largest device error of any slice is 6.1e-5 (GRU saturated_h64 dgates: with
z within a few ulp of 1 the factor 1 - z cancels; the fp32 oracle's own worst slice of that tensor is
6.1e-5 off as well and no slice's ratio is above 3.58, so CAP is the nearer bound in such a slice and
holds), the next largest 2.1e-6.  The v_exp_f32 / v_rcp_f32 activations put the device no more than
7.5 times as far from float64 as numpy's fp32 anywhere.  No kernel defect was found.
"""
import numpy as np
import pytest
import torch

from _rec import (BY_NAME, C, CAP, CASES, CELLS, TENSORS, assert_live, case_inputs, checked_nets, compare,
                  make_inputs, references, run_cell)
from _util import close_sliced, sliced_ratio, sliced_report

pytestmark = pytest.mark.gpu
NAMES = [c.name for c in CASES]


@pytest.fixture(scope="module")
def nat(pkg_on_path):
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible")
    import mmf_native
    mmf_native.lib()
    return mmf_native


@pytest.fixture(scope="module")
def enc_mod(pkg_on_path):
    import encoders
    return encoders


def profiled(nat, cell, nets):
    """run_cell under the library's launch records -> (outputs, the recurrence kernels that ran)."""
    nat.profile_begin()
    try:
        outs = run_cell(nat, cell, nets)
    finally:
        _, launches = nat.profile_end()
    return outs, [k for _, k, *_ in launches if k.startswith(cell)]


@pytest.mark.parametrize("cell", CELLS)
@pytest.mark.parametrize("name", NAMES)
def test_case_vs_fp64(nat, name, cell):
    case = BY_NAME[name]
    nets = case_inputs(name, cell)
    picked = checked_nets(case.n)
    live = min(assert_live(references(name, cell, i)[0], f"{cell} {name} net {i}") for i in picked)
    outs, ran = profiled(nat, cell, nets)
    G = case.H // 64
    inst = case.n * ((case.B + 3) // 4)
    print(f"REC {cell} {name}: {cell}_fwd_kernel<{case.H}> over T = {case.T} steps "
          f"({'h_{t-1} nonzero from t = 1' if case.T > 1 else 'h_{t-1} = 0 only'}), {inst} instances x G = {G} = "
          f"{inst * G} workgroups, launches {ran}, smallest slice of the reference {live:.1e} of its tensor")
    assert ran == [f"{cell}_fwd_kernel", f"{cell}_bwd_kernel"], ran
    for i, out in enumerate(outs):
        for key in TENSORS[cell]:
            assert np.isfinite(out[key]).all(), (i, key)
    bad, worst = [], 0.0
    for i in picked:
        r64, r32 = references(name, cell, i)
        b, w = compare(cell, outs[i], r64, r32, f"{cell} {name} net {i}")
        bad += b
        worst = max(worst, w)
    print(f"REC {cell} {name}: worst ratio {worst:.2f} (C = {C})")
    for i in range(case.n):
        for k in range(i + 1, case.n):
            for key in TENSORS[cell]:
                assert not np.array_equal(outs[i][key], outs[k][key]), (i, k, key)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("cell", CELLS)
def test_row_independent_of_instance(nat, cell):
    """n = 1, B = 9, T = 10, H = 192 as one launch (instances of 4 + 4 + 1 rows) and as nine B = 1
    launches on the same rows: a row's arithmetic does not involve B and the gather sums in a fixed
    order, so every output of every row is the same bit for bit."""
    B, T, H = 9, 10, 192
    inp = make_inputs(np.random.default_rng([77, CELLS.index(cell)]), cell, B, T, H)
    whole = run_cell(nat, cell, [inp])[0]
    for b in range(B):
        row = {k: (v[b:b + 1] if v.ndim == 3 else v) for k, v in inp.items()}
        alone = run_cell(nat, cell, [row])[0]
        for key in TENSORS[cell]:
            assert np.isfinite(alone[key]).all() and alone[key].any(), (b, key)
            assert np.array_equal(whole[key][b:b + 1], alone[key]), (
                b, key, float(np.abs(whole[key][b:b + 1] - alone[key]).max()))


@pytest.mark.parametrize("cell", CELLS)
def test_rerun_is_bit_identical(nat, cell):
    """n8_h256 (64 mutually waiting workgroups) twice, forward and backward: the same bits."""
    nets = case_inputs("n8_h256", cell)
    first, second = run_cell(nat, cell, nets), run_cell(nat, cell, nets)
    for i, (a, b) in enumerate(zip(first, second)):
        for key in TENSORS[cell]:
            assert np.isfinite(a[key]).all(), (i, key)
            assert np.array_equal(a[key], b[key]), (i, key, float(np.abs(a[key] - b[key]).max()))


# ---------------------------------------------------------------------------
# Module level: SequenceEncoder('lstm') and GRUSequenceEncoder under the same rule
# ---------------------------------------------------------------------------
ENC_B, ENC_T, ENC_D, ENC_H, ENC_LAYERS, ENC_OUT = 7, 19, 11, 128, 2, 8
ENC_LENGTHS = [19, 1, 7, 19, 2, 12, 5]


class _TorchEncoder(torch.nn.Module):
    """torch.nn.LSTM / GRU + Linear with the encoders' state dict (rnn.*, projection.*): run over the
    full T and read at lengths - 1, as oracle/lstm_cpu.sequence_encoder does."""

    def __init__(self, cell):
        super().__init__()
        rnn = torch.nn.LSTM if cell == "lstm" else torch.nn.GRU
        self.rnn = rnn(ENC_D, ENC_H, num_layers=ENC_LAYERS, batch_first=True)
        self.projection = torch.nn.Linear(ENC_H, ENC_OUT)

    def forward(self, x, lengths):
        out, _ = self.rnn(x)
        return self.projection(out[torch.arange(x.shape[0]), lengths - 1])


def _encoder_run(model, x, lengths, g_out):
    x = x.clone().requires_grad_(True)
    enc = model(x, lengths)
    (enc * g_out).sum().backward()
    res = {"encoding": enc.detach().cpu(), "dx": x.grad.detach().cpu()}
    res.update({f"grad/{k}": p.grad.detach().cpu() for k, p in model.named_parameters()})
    return res


@pytest.mark.parametrize("cell", CELLS)
def test_sequence_encoder_vs_fp64(enc_mod, cell):
    torch.manual_seed(31 + CELLS.index(cell))
    if cell == "lstm":
        mine = enc_mod.SequenceEncoder(ENC_D, ENC_H, ENC_OUT, num_layers=ENC_LAYERS, encoder_type="lstm")
    else:
        mine = enc_mod.GRUSequenceEncoder(ENC_D, ENC_H, ENC_OUT, num_layers=ENC_LAYERS)
    sd = {k: v.detach().clone() for k, v in mine.state_dict().items()}
    x = torch.randn(ENC_B, ENC_T, ENC_D)
    g_out = torch.randn(ENC_B, ENC_OUT)
    lengths = torch.tensor(ENC_LENGTHS)
    refs = []
    for dtype in (torch.float64, torch.float32):
        ref = _TorchEncoder(cell)
        ref.load_state_dict(sd, strict=True)
        refs.append(_encoder_run(ref.to(dtype).eval(), x.to(dtype), lengths, g_out.to(dtype)))
    ref64, ref32 = refs
    assert all(v.dtype == torch.float64 for v in ref64.values()) and all(v.dtype == torch.float32 for v in ref32.values())
    mine = mine.to("cuda:0").eval()
    got = _encoder_run(mine, x.to("cuda:0"), lengths, g_out.to("cuda:0"))
    assert not enc_mod.lstm_timed_out("cuda:0")
    assert set(got) == set(ref64)
    for b, n in enumerate(ENC_LENGTHS):
        assert not bool(got["dx"][b, n:].any()), b        # padded steps: exactly zero
        assert bool(got["dx"][b, :n].any()), b
    bad, worst = [], 0.0
    for key in ref64:
        sdim = 0 if key in ("encoding", "dx") else None   # per sample; a parameter gradient is one slice
        ratio, e_dev = sliced_ratio(got[key], ref64[key], ref32[key], slice_dim=sdim)
        worst = max(worst, ratio)
        print(f"REC {cell} encoder {key}: ratio {ratio:.2f}, e_dev {e_dev:.3e}")
        if not close_sliced(got[key], ref64[key], ref32[key], slice_dim=sdim, c=C, cap=CAP):
            bad.append(f"{key}: " + sliced_report(got[key], ref64[key], ref32[key], slice_dim=sdim, c=C, cap=CAP))
    print(f"REC {cell} encoder: worst ratio {worst:.2f} (C = {C})")
    assert not bad, "\n".join(bad)
