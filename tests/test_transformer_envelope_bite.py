"""The per-token float64 rule of tests/test_gpu_transformer_envelope.py rejects the defects it exists for.

No device: "got" is the fp32 CPU oracle's own result (tests/_transenc.stack_forward, dropout 0.1 replayed
from Philox, its own ReLU decisions handed back as the gates the GPU module would read from the device) with
one defect planted, through stack_forward's hooks or on its outputs, on tr_chunk_edges (5 x 130, H = 64,
lengths 130 / 129 / 128 / 64 / 1), tr_ragged_h252 (3 x 47, H = 252, lengths 47 / 46 / 3) and, for the defects
in a ragged tail, tr_ragged_h252_tail (lengths 3 / 46 / 47: with the shortest sample last, the last slab,
chunk and reduce group of tr_ragged_h252 hold padded rows, whose partials are exactly zero) -- the shapes the
GPU module runs.  _transenc.compare_envelope with that module's C and CAP must reject each, and passes
the unplanted oracle.

  1  keys_lost         one valid token of the 130-step sample loses the keys >= 128 in one head (its O row
                       and LSE), carried through the rest of the forward
  2a ln_chunk          norm2.weight's gradient without one 32-row chunk's partial
  2b ln_group          ... without the last (short) reduce group: chunks 3 and 4 (rows 96..140, all valid) of
                       tr_ragged_h252_tail's 3 + 2
  3  slab_w, slab_b    out_proj.weight's / .bias's gradient without the last, 13-row slab (rows 128..140, all
                       valid) of tr_ragged_h252_tail
  4  keep_transposed   the out_proj branch's backward keep mask (dr of LayerNorm 1) drawn for one row at
                       the transposed index c n + row instead of row H + c
  5a dx_neighbour      one valid dx row taken from its neighbour
  5b dx_padded         one padded dx row left at 1e-7
  6  y1_scaled         a 2e-4 scale on one token's y1, carried on
  7  gate_scale        the 1 / (1 - p) gate scale dropped in one 128-row tile of dH (ffn = 32: one column tile)
  8  ln_variance       rstd from E[z^2] - E[z]^2 at a mean of 100 (Case(2, 9, 6, 32, ffn=24, bias_offset=100))

For each the older verdict, close(., float64, 1e-3) on out, dx and the gradients -- all that
tests/test_gpu_transformer_encoder.py looks at -- is printed.  It is asserted for defect 1 only, which it
must pass: that is why the GPU module exists.  The dilution: the token's O row moves in 16 of 64 columns, the
change reaches out only through the mean over 130 steps, and every gradient sums over 650 rows.  Observed
here (reported, not asserted): the old rule also passes 5b and 6 and rejects 2a, 2b, 3, 4, 5a, 7 and 8 -- at
these small shapes a missing chunk or slab is percents of its one tensor; what it cannot see is a single
token of the forward (1, 6) and an inexact zero (5b).
"""
import pytest
import torch

import _philox
from _transenc import (C, CAP, ENVELOPE_CASES as CASES, P_DROP, RNG, SITE_TR, Case, compare_envelope, gated_references,
                       ln_plan, make_case, old_rule, run_oracle, tail_rows, wgrad_plan)

EDGE, RAG, RAGT = CASES["tr_chunk_edges"], CASES["tr_ragged_h252"], CASES["tr_ragged_h252_tail"]
OFFSET = Case(2, 9, 6, 32, ffn=24, bias_offset=100.0)
_BASE = {}


def base(case):
    """(inputs, masks, p, gates, float64 reference, fp32 reference) of a case, computed once."""
    if case not in _BASE:
        p = P_DROP if case is not OFFSET else 0.0
        sd, x, lengths, gout = make_case(case)
        masks = _philox.mask_provider(RNG[0], RNG[1], p) if p > 0 else None
        own = run_oracle(case, sd, x, lengths, gout, torch.float32, p=p, mask_fn=masks)
        h_dev = {k: own[f"h/{k}"] for k in range(case.layers)}
        r64, r32, _ = gated_references(case, sd, x, lengths, gout, h_dev, p, masks, case.id)
        gates = {k: (r64[f"pre/{k}"].abs() <= 1e-5 * r64[f"scale/{k}"], h_dev[k] > 0) for k in range(case.layers)}
        _BASE[case] = ((sd, x, lengths, gout), masks, p, gates, r64, r32)
    return _BASE[case]


def planted(case, hooks=None, live=None):
    """The fp32 oracle of the case with the hooks planted, under the base run's masks and gates."""
    (sd, x, lengths, gout), masks, p, gates, _, _ = base(case)
    return run_oracle(case, sd, x, lengths, gout, torch.float32, p=p, mask_fn=masks, relu_gate=gates, hooks=hooks,
                      live=live)


def verdicts(case, got, tag):
    """(the envelope rule's violations, the old rule's verdict) of a planted result."""
    _, _, _, _, r64, r32 = base(case)
    bad, _, _ = compare_envelope(got, r64, r32, case.layers, f"BITE {tag}", C, CAP)
    old = old_rule(got, r64)
    print(f"BITE {tag}: the envelope rule {'REJECTS' if bad else 'passes'} ({len(bad)} tensors: "
          f"{[b.split(':')[0] for b in bad][:6]}), the old rule close(., 1e-3) {'passes' if old else 'REJECTS'}")
    return bad, old


def copy_of(res):
    return {k: v.clone() for k, v in res.items()}


@pytest.mark.parametrize("case", [EDGE, RAG, RAGT, OFFSET],
                         ids=["tr_chunk_edges", "tr_ragged_h252", "tr_ragged_h252_tail", "offset100"])
def test_unplanted_oracle_passes(case):
    got = planted(case)
    assert torch.equal(got["out"], base(case)[5]["out"])
    bad, old = verdicts(case, got, f"unplanted {case.id}")
    assert not bad and old, bad


def test_1_keys_lost():
    def scores(k, s):
        s = s.clone()
        s[0, 2, 100, 128:] = float("-inf")
        return s
    bad, old = verdicts(EDGE, planted(EDGE, {"scores": scores}), "1 keys_lost")
    assert any(b.startswith("o/0") for b in bad) and any(b.startswith("lse/0") for b in bad), bad
    assert old, "the whole-tensor 1e-3 rule on out, dx and the gradients was expected to pass this defect"


def _ln2_partial(case, rows):
    """sum over `rows` of dy xhat of the last LayerNorm: a reduce partial of norm2.weight's gradient."""
    live = {}
    res = planted(case, live=live)
    H = case.hidden
    dy = live["y2/0"].grad.reshape(-1, H)
    st = res["st2/0"].reshape(-1, 2)
    xhat = (res["z2/0"].reshape(-1, H) - st[:, :1]) * st[:, 1:]
    return res, (dy[rows] * xhat[rows]).sum(0)


def test_2a_ln_chunk():
    assert ln_plan(EDGE)[0] == 21
    res, part = _ln2_partial(EDGE, slice(7 * 32, 8 * 32))       # chunk 7: valid tokens of sample 1
    got = copy_of(res)
    got["grad/transformer.layers.0.norm2.weight"] -= part
    bad, _ = verdicts(EDGE, got, "2a ln_chunk")
    assert [b.split(":")[0] for b in bad] == ["grad/transformer.layers.0.norm2.weight"], bad


def test_2b_ln_group():
    chunks, _, group, ngroup, last, _ = ln_plan(RAGT)
    assert (chunks, group, ngroup, last) == (5, 3, 2, 2) and tail_rows(RAGT)["ln_group"] == (45, 45)
    res, part = _ln2_partial(RAGT, slice(group * (ngroup - 1) * 32, None))   # chunks 3 and 4: rows 96..140
    got = copy_of(res)
    got["grad/transformer.layers.0.norm2.weight"] -= part
    bad, _ = verdicts(RAGT, got, "2b ln_group")
    assert [b.split(":")[0] for b in bad] == ["grad/transformer.layers.0.norm2.weight"], bad


@pytest.mark.parametrize("which", ["weight", "bias"])
def test_3_slab(which):
    plan = {j[0]: j for j in wgrad_plan(RAGT)}
    _, M, N, _, nsplit, kchunk, last, _ = plan["out_proj"]
    assert (nsplit, kchunk, last) == (5, 32, 13) and tail_rows(RAGT)["slab/out_proj"] == (13, 13)
    live = {}
    res = planted(RAGT, live=live)
    da = live["a/0"].grad.reshape(-1, M)
    o = res["o/0"].reshape(-1, N)
    key = f"grad/transformer.layers.0.self_attn.out_proj.{which}"
    rows = slice((nsplit - 1) * kchunk, None)                  # the ragged last slab: rows 128..140
    got = copy_of(res)
    got[key] -= da[rows].t() @ o[rows] if which == "weight" else da[rows].sum(0)
    bad, _ = verdicts(RAGT, got, f"3 slab_{which}")
    assert [b.split(":")[0] for b in bad] == [key], bad


def test_4_keep_transposed():
    n, H, row = RAG.B * RAG.T, RAG.hidden, 5

    def drop_bwd(site, t, keep):
        if site != SITE_TR + 1:
            return None
        flat = keep.reshape(-1)
        alt = keep.clone().reshape(n, H)
        alt[row] = flat[torch.arange(H) * n + row]
        assert not torch.equal(alt[row], keep.reshape(n, H)[row])
        return alt.reshape(keep.shape) / (1.0 - P_DROP)
    got = planted(RAG, {"drop_bwd": drop_bwd})
    assert torch.equal(got["out"], base(RAG)[5]["out"])           # the forward is untouched
    bad, _ = verdicts(RAG, got, "4 keep_transposed")
    assert any(b.startswith("dx") for b in bad), bad


def test_5a_dx_neighbour():
    got = copy_of(planted(EDGE))
    got["dx"][1, 77] = got["dx"][1, 78]
    bad, _ = verdicts(EDGE, got, "5a dx_neighbour")
    assert [b.split(":")[0] for b in bad] == ["dx"], bad


def test_5b_dx_padded():
    got = copy_of(planted(EDGE))
    assert float(got["dx"][3, 64:].abs().max()) == 0.0
    got["dx"][3, 64, 0] = 1e-7
    bad, _ = verdicts(EDGE, got, "5b dx_padded")
    assert bad == ["dx: a padded row is not exactly 0.0 (max 1.000e-07)"], bad


def test_6_y1_scaled():
    def y1(k, t):
        f = torch.ones(t.shape[:2], dtype=t.dtype)
        f[1, 5] = 1.0 + 2e-4
        return t * f.unsqueeze(-1)
    bad, _ = verdicts(RAG, planted(RAG, {"y1": y1}), "6 y1_scaled")
    assert any(b.startswith("y1/0") for b in bad), bad


def test_7_gate_scale():
    n = EDGE.B * EDGE.T

    def drop_bwd(site, t, keep):
        if site != SITE_TR + 2:
            return None
        alt = (keep / (1.0 - P_DROP)).reshape(n, -1).clone()
        alt[128:256] = keep.reshape(n, -1)[128:256]               # rows 128..255, every column (ffn = 32 < 128)
        return alt.reshape(keep.shape)
    got = planted(EDGE, {"drop_bwd": drop_bwd})
    assert torch.equal(got["y2/0"], base(EDGE)[5]["y2/0"])
    bad, _ = verdicts(EDGE, got, "7 gate_scale")
    assert any(b.startswith("dx") for b in bad) and any("linear1.weight" in b for b in bad), bad


def test_8_ln_variance():
    def layer_norm(z, gamma, beta, eps):
        mean = z.mean(dim=-1, keepdim=True)
        var = (z * z).mean(dim=-1, keepdim=True) - mean * mean
        return (z - mean) / torch.sqrt(var.clamp_min(0.0) + eps) * gamma + beta
    bad, _ = verdicts(OFFSET, planted(OFFSET, {"layer_norm": layer_norm}), "8 ln_variance")
    assert any(b.startswith("y1/0") for b in bad), bad
