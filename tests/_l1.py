"""Shared by tests/test_gpu_l1_envelope.py, tests/test_l1_envelope_bite.py and
tests/test_gpu_train_step.py: the launch-lean L = 1 plan's envelope cases (csrc/l1.hip,
lean_l1_desc of csrc/hybrid.hip), their oracle step and the float64 comparison rule (test infra).
"""
import numpy as np
import torch

from _philox import mask_provider
from _util import close_sliced, sliced_ratio, sliced_report
from cases import _MASK_ROWS, HybridCase, hybrid_inputs, hybrid_state
from test_gpu_attn_headdims import C, CAP

SEED, OFFSET = 0x2468_ACE0_1357, 3

MASK_M4 = [[1, 1, 1, 1], [1, 0, 1, 1], [0, 0, 0, 0], [0.5, 1, 0, 1], [0, 0, 1, 0], [1, 1, 1, 0.25], [0, 1, 1, 1]]
MASK_M2 = [[1, 1], [1, 0], [0, 1], [0, 0], [0.5, 1], [1, 0.25], [1, 1]]
MASKS = {4: MASK_M4, 3: _MASK_ROWS, 2: MASK_M2}


def _case(name, dims, batch, hidden, heads, classes, seed):
    names = [f"m{i}" for i in range(len(dims))]
    return HybridCase(name, names, dict(zip(names, dims)), {m: 0 for m in names}, batch=batch, hidden=hidden,
                      heads=heads, classes=classes, seed=seed, mask=MASKS[len(dims)])


L1_CASES = [
    # l1_key_bwd_kernel<0, 3> and the three-pairs-per-key branch of pair_key_bwd, 12 pairs, 34 weight-gradient
    # jobs, 48 zero regions (L1_MAXZ), C = 16 (L1_MAXC), H % 16 != 0, head dim 12, 2 tiles (the second: 5 rows)
    _case("l1_m4_ragged", [12, 20, 4, 16], 21, 36, 3, 16, 401),
    # the <128> forms with three pairs per key, head dim 16, 484 weight-gradient tiles, a 1-row last tile
    _case("l1_m4_full128", [128] * 4, 17, 128, 8, 5, 402),
    # the <128> forms with one pair per key, one head of 128, exactly one tile, one waiting workgroup per tile
    _case("l1_m2_full128", [128] * 2, 16, 128, 1, 3, 403),
    # 17 tiles, the weight gradient's second 256-row chunk (4 rows), the loss sum's second stride, head dim 4
    _case("l1_m2_b260", [8, 24], 260, 20, 5, 2, 404),
    # no dropout, H = 100, D from 4 to 128 in one model, 3 tiles with a 1-row last tile
    _case("l1_m3_h100", [100, 4, 128], 33, 100, 5, 11, 405),
    # 22 tiles x 12 pairs = 264 workgroups: over l1_train_capacity on a 256-CU part (the split plan's step)
    _case("l1_m4_b352", [4] * 4, 352, 8, 2, 3, 406),
]
BY_NAME = {c.name: c for c in L1_CASES}
DROPOUT = {c.name: 0.0 if c.name == "l1_m3_h100" else 0.1 for c in L1_CASES}


def case_labels(case):
    return torch.from_numpy(np.random.default_rng(case.seed + 31337).integers(0, case.classes, case.batch))


def masked_samples(case):
    """Indices of the samples whose every modality is masked."""
    _, mask_np, _ = hybrid_inputs(case)
    return [b for b in range(case.batch) if not mask_np[b].any()]


def oracle_step(case, dtype, seed=SEED, offset=OFFSET, taps=None, relu_gate=None, rows=None):
    """forward -> CE(label_smoothing 0.05) -> backward of the oracle under the replayed masks:
    {logits, loss, dx/<m>, <parameter name>}.  rows: the loss keeps samples [0, rows) only, still
    divided by the batch (what a weight gradient that left the later rows out would be of)."""
    from oracle.hybrid_cpu import cross_entropy_ls, hybrid_forward
    p = DROPOUT[case.name]
    sd = hybrid_state(case.names, case.dims, case.hidden, case.classes, case.seed)
    feats_np, mask_np, _ = hybrid_inputs(case)
    params = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in sd.items()}
    xs = {m: torch.from_numpy(v).to(dtype).requires_grad_(True) for m, v in feats_np.items()}
    logits, _ = hybrid_forward(params, case.names, xs, torch.from_numpy(mask_np).to(dtype), case.heads, p=p,
                               train=True, gen=mask_provider(seed, offset, p), taps=taps, relu_gate=relu_gate)
    if rows is None:
        loss = cross_entropy_ls(logits, case_labels(case))
    else:
        per = torch.nn.functional.cross_entropy(logits, case_labels(case), label_smoothing=0.05, reduction="none")
        loss = per[:rows].sum() / case.batch
    loss.backward()
    out = {"logits": logits.detach(), "loss": loss.detach()}
    out.update({f"dx/{m}": xs[m].grad for m in case.names})
    out.update({n: p_.grad for n, p_ in params.items()})
    return out


def is_qk(key):
    return ".query_proj." in key or ".key_proj." in key


def compare_step(case, got, ref64, ref32, tag):
    """One train step against float64: logits and every dx/<m> per sample, the loss and every
    parameter gradient as one slice under close_sliced(C, CAP), e_32 from the two CPU oracles alone;
    the query / key projection gradients (softmax over one key: no gradient reaches them) and the
    input gradients of fully masked samples exact zeros.  Prints each figure, returns the failures."""
    bad = []
    assert set(got) == set(ref64) == set(ref32), (sorted(got), sorted(ref64))
    dead = masked_samples(case)
    for key in ref64:
        if is_qk(key):
            assert not bool(ref64[key].any()), key   # (the float64 reference: identically zero)
            if not bool(torch.all(got[key] == 0)):
                bad.append(f"{key}: not exactly zero, max {float(got[key].abs().max()):.3e}")
            continue
        sdim = 0 if key == "logits" or key.startswith("dx/") else None
        ratio, e_dev = sliced_ratio(got[key], ref64[key], ref32[key], slice_dim=sdim)
        print(f"L1ENV {tag} {key}: ratio {ratio:.2f}, e_dev {e_dev:.3e}")
        if not close_sliced(got[key], ref64[key], ref32[key], slice_dim=sdim, c=C, cap=CAP):
            bad.append(f"{key}: " + sliced_report(got[key], ref64[key], ref32[key], slice_dim=sdim, c=C, cap=CAP))
        if key.startswith("dx/"):
            for b in dead:
                if not bool(torch.all(got[key][b] == 0)):
                    bad.append(f"{key}[{b}] of a fully masked sample is not exactly zero: "
                               f"max {float(got[key][b].abs().max()):.3e}")
    return bad


def _three_calls(st, nat):
    """The split path the one-call step replaces: mmf_hybrid_forward -> mmf_cross_entropy_ls ->
    mmf_hybrid_backward on the step's own buffers (accumulate = 1)."""
    import ctypes
    L = nat.lib()
    d = st.plan.desc
    s = nat.stream_ptr(st.dev)
    rc = L.mmf_hybrid_forward(ctypes.byref(d), ctypes.byref(st.pstruct), ctypes.cast(st.xarr[0], ctypes.c_void_p),
                              st.mask.data_ptr(), st.rng.data_ptr(), st.saved.data_ptr(), st.logits.data_ptr(),
                              st.fw.data_ptr(), None, s)
    nat.check(rc, "forward")
    rc = L.mmf_cross_entropy_ls(st.mask.size(0), d.num_classes, st.logits.data_ptr(), st.labels.data_ptr(),
                                st.smoothing, 1.0, st.losses.data_ptr(), st.dlogits.data_ptr(), s)
    nat.check(rc, "cross-entropy")
    rc = L.mmf_hybrid_backward(ctypes.byref(d), ctypes.byref(st.pstruct), ctypes.cast(st.xarr[0], ctypes.c_void_p),
                               st.mask.data_ptr(), st.saved.data_ptr(), st.dlogits.data_ptr(), st.ws.data_ptr(),
                               ctypes.byref(st.gstruct), ctypes.cast(st.dxarr[0], ctypes.c_void_p), s)
    nat.check(rc, "backward")
