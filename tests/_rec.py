"""The LSTM / GRU recurrence (csrc/recurrence.h, lstm.hip, gru.hip) against float64, step by step
(test helper, not collected): the case table of tests/test_gpu_recurrence_envelope.py, the seeded
input recipes, the raw C-ABI runners and the rule.

The rule (compare): tests/_util.close_sliced with one slice per (row, time step) -- (B, T, X) seen as
(B T, X) -- on h, c (LSTM), gates and dgates: max|got - ref64| <= min(C max(e_32, 2^-24), CAP) of the
slice's max|ref64|, e_32 being the fp32 oracle's own distance from the float64 one in that slice.  A
whole-tensor bound cannot see a step whose BPTT gradient is a thousandth of the largest; this one
normalises every step by itself, so no step is left out -- which needs a reference that is alive in
every slice (assert_live: each slice's max|ref64| at least 1e-6 of its tensor's, asserted from the
float64 oracle before the device is touched; the +2 on the LSTM's forget slice and the GRU's z slice
keeps the carry alive).

C is measured, not chosen: the worst e_dev / max(e_32, 2^-24) over every case, tensor
and slice on the MI355X, doubled, rounded up to a power of two.  CAP is the project's 1e-4.
"""
from __future__ import annotations

import functools
from typing import NamedTuple

import numpy as np
import torch

from _gru import gru_backward, gru_forward
from _util import close_sliced, rel_err, sliced_errors, sliced_ratio, sliced_report

C = 16.0      # measured worst 7.47 (the docstring of tests/test_gpu_recurrence_envelope.py)
CAP = 1e-4
LIVE = 1e-6   # every (row, step) slice of the float64 reference is at least this much of its tensor's maximum
CELLS = ("lstm", "gru")
TENSORS = {"lstm": ("h", "c", "gates", "dgates"), "gru": ("h", "gates", "dgates")}
NGATES = {"lstm": 4, "gru": 3}
KEEP = 1     # the gate slice that carries the state, in both cells: f of (i, f, g, o), z of (r, z, n)


class RecCase(NamedTuple):
    name: str
    n: int
    B: int
    T: int
    H: int
    dh: str = "all"      # "all": dh ~ N(0, 1) on every step; "last": on the last step only
    scale: float = 1.0   # xproj multiplied by this


CASES = [
    RecCase("inst32_h64", 8, 16, 6, 64),          # LMAX_N and LMAX_I: 32 instances, 32 workgroups
    RecCase("n8_h256", 8, 8, 6, 256),             # 8 networks x G = 4: 64 workgroups, 16 instances
    RecCase("b128_h64", 1, 128, 5, 64),           # one network, b0 up to 124, 32 instances
    RecCase("tail3_h128", 2, 7, 9, 128),          # 4 + 3 rows; the <128> matvec against a nonzero h
    RecCase("tail2_h192", 1, 6, 9, 192),          # 4 + 2 rows, KP = 12
    RecCase("single3_h256", 3, 3, 9, 256),        # one partial instance per network
    RecCase("parity_t2", 1, 4, 2, 256),           # first reuse of a parity buffer
    RecCase("parity_t3", 1, 4, 3, 256),
    RecCase("carry_h64", 1, 2, 64, 64, "last"),   # every older step is pure carry
    RecCase("carry_h256", 1, 2, 64, 256, "last"),
    RecCase("long_h256", 1, 2, 1024, 256),        # the C3 length with two rows, dh on every step
    RecCase("saturated_h64", 1, 2, 16, 64, "all", 20.0),   # exp overflow / rcp(inf)
]
BY_NAME = {c.name: c for c in CASES}


def make_inputs(rng, cell, B, T, H, dh="all", scale=1.0):
    """One network's inputs, float32: xproj ~ N(0, 1) with +2 on the slice that carries the state
    (times `scale`), w_hh and b_hn (GRU) ~ U(+-1/sqrt(H)), dh ~ N(0, 1) on every step or the last."""
    ng = NGATES[cell]
    bound = 1.0 / np.sqrt(H)
    xproj = rng.standard_normal((B, T, ng * H))
    xproj[..., KEEP * H:(KEEP + 1) * H] += 2.0
    out = {"xproj": (xproj * scale).astype(np.float32),
           "w_hh": rng.uniform(-bound, bound, size=(ng * H, H)).astype(np.float32)}
    if cell == "gru":
        out["b_hn"] = rng.uniform(-bound, bound, size=H).astype(np.float32)
    d = rng.standard_normal((B, T, H)).astype(np.float32)
    if dh == "last":
        d[:, :-1] = 0.0
    out["dh"] = d
    return out


@functools.lru_cache(maxsize=None)
def case_inputs(name, cell):
    """The case's networks, each with its own data (computed once; treat as read-only)."""
    case = BY_NAME[name]
    rng = np.random.default_rng([CASES.index(case), CELLS.index(cell), 20240])
    return tuple(make_inputs(rng, cell, case.B, case.T, case.H, case.dh, case.scale) for _ in range(case.n))


def oracle(cell, inp, dtype=np.float64, fwd_hook=None, bwd_hook=None):
    """{h, (c,) gates, dgates} of one network from the CPU oracle, all of `dtype`."""
    if cell == "lstm":
        from oracle.lstm_cpu import lstm_backward, lstm_forward
        H = inp["w_hh"].shape[1]
        eye, z = np.eye(4 * H, dtype=np.float32), np.zeros(4 * H, np.float32)   # x I + 0 is xproj exactly
        h, c, g = lstm_forward(inp["xproj"], eye, inp["w_hh"], z, z, dtype=dtype, hook=fwd_hook)
        return {"h": h, "c": c, "gates": g, "dgates": lstm_backward(inp["w_hh"], c, g, inp["dh"], dtype=dtype, hook=bwd_hook)}
    h, g = gru_forward(inp["xproj"], inp["w_hh"], inp["b_hn"], dtype=dtype, hook=fwd_hook)
    return {"h": h, "gates": g, "dgates": gru_backward(inp["w_hh"], h, g, inp["dh"], dtype=dtype, hook=bwd_hook)}


@functools.lru_cache(maxsize=None)
def references(name, cell, net):
    """(float64 oracle, fp32 oracle) of network `net` of the case: computed once, left unchanged."""
    inp = case_inputs(name, cell)[net]
    r64, r32 = oracle(cell, inp, np.float64), oracle(cell, inp, np.float32)
    assert all(v.dtype == np.float64 for v in r64.values()) and all(v.dtype == np.float32 for v in r32.values())
    return r64, r32


def checked_nets(n):
    """Networks compared with the oracles: all of them up to two, else the first, a middle one and the last."""
    return list(range(n)) if n <= 2 else [0, n // 2, n - 1]


def _steps(a):
    return torch.from_numpy(np.ascontiguousarray(a)).reshape(-1, a.shape[-1])


def assert_live(ref64, tag):
    """Every (row, step) slice of every float64 reference tensor is finite and at least LIVE of the
    tensor's maximum: the per-slice rule then leaves no step out.  Returns the smallest fraction."""
    worst = 1.0
    for key, v in ref64.items():
        assert np.isfinite(v).all(), (tag, key)
        m = np.abs(v).max(axis=-1)
        frac = float(m.min() / m.max())
        assert frac >= LIVE, f"{tag} {key}: a slice of the float64 reference is {frac:.1e} of the tensor's maximum"
        worst = min(worst, frac)
    return worst


def compare(cell, got, ref64, ref32, tag, c=C, cap=CAP):
    """The rule: every tensor of the cell, one slice per (row, step).  Prints each tensor's worst
    e_dev / max(e_32, 2^-24) and largest e_dev with the old whole-tensor rel_err next to it;
    returns (the failures, the worst ratio)."""
    bad, worst = [], 0.0
    for key in TENSORS[cell]:
        g, r64, r32 = _steps(got[key]), _steps(ref64[key]), _steps(ref32[key])
        ratio, e_dev = sliced_ratio(g, r64, r32, slice_dim=0)
        e32 = sliced_errors(g, r64, r32, 0)[1]
        print(f"REC {tag} {key}: ratio {ratio:.2f}, e_dev {e_dev:.3e}, e_32 {float(e32.min()):.1e}..{float(e32.max()):.1e}, "
              f"whole-tensor rel_err {rel_err(g, r64):.2e}")
        worst = max(worst, ratio)
        if not close_sliced(g, r64, r32, slice_dim=0, c=c, cap=cap):
            bad.append(f"{tag} {key}: " + sliced_report(g, r64, r32, slice_dim=0, c=c, cap=cap))
    return bad, worst


def old_rule(cell, got, ref64):
    """The whole-tensor rel_err of every tensor: what tests/test_gpu_lstm.py and test_gpu_gru.py bound by 1e-3."""
    return {key: rel_err(got[key], ref64[key]) for key in TENSORS[cell]}


# ---------------------------------------------------------------------------
# The raw C-ABI runners
# ---------------------------------------------------------------------------
def _dev_list(arrs, dev):
    return [torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev) if a is not None else None for a in arrs]


def run_lstm(nat, xproj_l, w_hh_l, dh_l):
    """Raw C-ABI forward + backward for n LSTMs on cuda:0; a None entry of dh_l is passed as NULL.
    The timeout word is read after each launch.  -> h, c, gates, dgates: lists of float64 arrays."""
    L = nat.lib()
    dev = torch.device("cuda", 0)
    n = len(xproj_l)
    B, T, H4 = xproj_l[0].shape
    H = H4 // 4
    xp, wh = _dev_list(xproj_l, dev), _dev_list(w_hh_l, dev)
    h = [torch.empty(B, T, H, device=dev) for _ in range(n)]
    c = [torch.empty(B, T, H, device=dev) for _ in range(n)]
    g = [torch.empty(B, T, 4 * H, device=dev) for _ in range(n)]
    sync = [torch.empty(L.mmf_lstm_sync_bytes(B, H), dtype=torch.uint8, device=dev) for _ in range(n)]
    tmo = torch.zeros(1, dtype=torch.int32, device=dev)
    arr = lambda ts: nat.ptr_array([t.data_ptr() if t is not None else 0 for t in ts])  # noqa: E731
    st = nat.stream_ptr(dev)
    rc = L.mmf_lstm_forward(n, B, T, H, arr(xp), arr(wh), arr(h), arr(c), arr(g), arr(sync), tmo.data_ptr(), st)
    assert rc == 0, L.mmf_last_error()
    torch.cuda.synchronize(dev)
    assert int(tmo.item()) == 0, "forward: inter-workgroup wait timed out"
    dh = _dev_list(dh_l, dev)
    dg = [torch.empty(B, T, 4 * H, device=dev) for _ in range(n)]
    rc = L.mmf_lstm_backward(n, B, T, H, arr(wh), arr(c), arr(g), arr(dh), arr(dg), arr(sync), tmo.data_ptr(), st)
    assert rc == 0, L.mmf_last_error()
    torch.cuda.synchronize(dev)
    assert int(tmo.item()) == 0, "backward: inter-workgroup wait timed out"
    cpu = lambda ts: [t.cpu().double().numpy() for t in ts]  # noqa: E731
    return cpu(h), cpu(c), cpu(g), cpu(dg)


def run_gru(nat, xproj_l, w_hh_l, b_hn_l, dh_l):
    """Raw C-ABI forward + backward for n GRUs on cuda:0; a None entry of dh_l is passed as NULL.
    The timeout word is read after each launch.  -> h, gates, dgates: lists of float64 arrays."""
    L = nat.lib()
    dev = torch.device("cuda", 0)
    n = len(xproj_l)
    B, T, H3 = xproj_l[0].shape
    H = H3 // 3
    xp, wh, bn = _dev_list(xproj_l, dev), _dev_list(w_hh_l, dev), _dev_list(b_hn_l, dev)
    h = [torch.empty(B, T, H, device=dev) for _ in range(n)]
    g = [torch.empty(B, T, 4 * H, device=dev) for _ in range(n)]
    sync = [torch.empty(L.mmf_gru_sync_bytes(B, H), dtype=torch.uint8, device=dev) for _ in range(n)]
    tmo = torch.zeros(1, dtype=torch.int32, device=dev)
    arr = lambda ts: nat.ptr_array([t.data_ptr() if t is not None else 0 for t in ts])  # noqa: E731
    st = nat.stream_ptr(dev)
    rc = L.mmf_gru_forward(n, B, T, H, arr(xp), arr(wh), arr(bn), arr(h), arr(g), arr(sync), tmo.data_ptr(), st)
    assert rc == 0, L.mmf_last_error()
    torch.cuda.synchronize(dev)
    assert int(tmo.item()) == 0, "forward: inter-workgroup wait timed out"
    dh = _dev_list(dh_l, dev)
    dg = [torch.empty(B, T, 4 * H, device=dev) for _ in range(n)]
    rc = L.mmf_gru_backward(n, B, T, H, arr(wh), arr(h), arr(g), arr(dh), arr(dg), arr(sync), tmo.data_ptr(), st)
    assert rc == 0, L.mmf_last_error()
    torch.cuda.synchronize(dev)
    assert int(tmo.item()) == 0, "backward: inter-workgroup wait timed out"
    cpu = lambda ts: [t.cpu().double().numpy() for t in ts]  # noqa: E731
    return cpu(h), cpu(g), cpu(dg)


def run_cell(nat, cell, nets):
    """The runner of `cell` on a sequence of make_inputs() dicts -> one {tensor: float64 array} per network."""
    col = lambda k: [d[k] for d in nets]  # noqa: E731
    if cell == "lstm":
        outs = run_lstm(nat, col("xproj"), col("w_hh"), col("dh"))
    else:
        outs = run_gru(nat, col("xproj"), col("w_hh"), col("b_hn"), col("dh"))
    return [dict(zip(TENSORS[cell], per_net)) for per_net in zip(*outs)]
