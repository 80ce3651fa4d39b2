"""The float64 comparison of tests/test_gpu_gemm_envelope.py rejects the defects it exists for.

No device: "got" is the fp32 CPU oracle's own step on env_ragged (B = 41, L = 100 / 72 / 130, the
shape the GPU module runs) with one defect planted, and tests/_seqstep.compare -- the function the
GPU module calls, with its C and CAP -- must reject it, while the unplanted fp32 oracle passes.
The slabs are those of the GPU module's restated split on 256 CUs (wgrad_plan).  Planted from the
oracle's taps (dZ_m = dL/da_m * ReLU'(z_m), X'_m = in/<m>):

  a_ragged_tail    projections.m0.0.weight (4,100 rows, 65 slabs of 64) without the 4 rows of its
                   ragged last slab
  b_middle_slab    the same gradient without one whole middle slab
  c_bias_slab      projections.m2.0.bias (5,330 rows, 56 slabs of 96) without one slab's row sums
  d_dx_neighbour   dx/m2 (L = 130): sample 1's rows of the 128-row tile 1 (flat rows 130..255)
                   taken from sample 0; sample 1's mask weight there is 0.25
and through planted_forward, a restatement of oracle.hybrid_cpu.hybrid_forward with two hooks
(without a hook it equals the oracle bit for bit, which is tested):
  e_value_head     one head's value-path term (pbar_h^T dU_h, the E_m term) of pair m0_to_m2 left
                   out of dZ_m2 for sample 1: every gradient downstream of dZ_m2 inherits it
  f_pcol_tile      mean_L P_m2 of sample 3 without its last 128-row tile (rows 128 and 129)

Whether the suite's older rule, close(got, fp32 oracle, 1e-3) of the whole tensor, notices each
defect is printed, and what was observed is asserted (OLD_RULE_PASSES): at this shape it rejects all
six too, each in fewer tensors -- a to d move their one tensor by 2.7e-2, 0.20, 0.25 and 0.68 of its
maximum; e moves projections.m2.0.bias by 4.8e-2, dx/m2 by 1.2e-2 and projections.m2.0.weight by
5.4e-3 (5 times the old bound); f moves sample 3's logits by 1.8e-4 and flips a classifier ReLU.
The old rule's blind spot at these shapes is the device's own rounding, not these defects: it
allows 1e-3 where the float64 rule allows at most 1e-4 and typically 1e-5.
"""
import functools

import pytest
import torch

from _seqstep import OFFSET, SEED, compare, oracle_step
from _util import close, device_relu_gates
from cases import hybrid_state, pair_names
from oracle import hybrid_cpu
from test_gpu_gemm_envelope import BY_NAME, C, CAP, P_DROP, wgrad_plan

CASE = BY_NAME["env_ragged"]
CUS = 256
OLD_TOL = 1e-3
SPLITS = {label: (nsplit, kchunk, last) for label, _, _, nsplit, kchunk, last in wgrad_plan(CASE, CUS)[0]}


def planted_forward(params, names, feats, mask, num_heads, p=0.0, train=False, gen=None, taps=None, relu_gate=None,
                    drop_value_head=None, drop_pcol_tile=None):
    """oracle.hybrid_cpu.hybrid_forward, restated with two hooks.
    drop_value_head = (pair index, sample, head): that head's value rows of that sample take P_k
    detached, so no gradient reaches P_k through them (value_proj's own gradients are intact);
    drop_pcol_tile = (modality, sample, first row): mean_L P_m of that sample without the rows from
    `first row` on (the forward value only: the backward of the mean is intact)."""
    F = hybrid_cpu
    mask = mask.to(feats[names[0]].dtype)
    P = {}
    for i, m in enumerate(names):
        x = feats[m]
        mk = mask[:, i].reshape(-1, *([1] * (x.dim() - 1)))
        xd = F._dropout(x * mk, p, train, gen, F.SITE_IN + i)
        z = F.linear(xd, params[f"projections.{m}.0.weight"], params[f"projections.{m}.0.bias"])
        a = F._relu(z, m, relu_gate)
        if taps is not None:
            taps[f"in/{m}"], taps[f"z/{m}"], taps[f"a/{m}"] = xd.detach(), z.detach(), a
            a.retain_grad()
        P[m] = F._dropout(a, p, train, gen, F.SITE_PROJ + i)
    lists = {m: [P[m]] for m in names}
    for g, (q, k) in enumerate(F.pairs_present(names, params)):
        ki = names.index(k)
        pre = f"attention_modules.{q}_to_{k}."
        if drop_value_head is not None and drop_value_head[0] == g:
            att, _ = _cma_cut_value_head(params, pre, P[q], P[k], drop_value_head[1], drop_value_head[2], num_heads,
                                         mask[:, ki], p, train, gen, F.SITE_ATTN + g)
        else:
            att, _ = F.cma_forward(params, pre, P[q], P[k], P[k], num_heads, mask=mask[:, ki], p=p, train=train,
                                   gen=gen, site=F.SITE_ATTN + g)
        lists[q].append(att)
    pooled = []
    for i, m in enumerate(names):
        agg = torch.stack(lists[m], 0).mean(0)
        agg = agg * mask[:, i].reshape(-1, *([1] * (agg.dim() - 1)))
        pm = agg.mean(1) if agg.dim() == 3 else agg
        if drop_pcol_tile is not None and drop_pcol_tile[0] == m:
            _, b, row0 = drop_pcol_tile
            gone = torch.zeros_like(pm)
            gone[b] = (P[m][b, row0:].sum(0) * mask[b, i] / (len(lists[m]) * P[m].shape[1])).detach()
            pm = pm - gone
        pooled.append(pm)
    pooled_t = torch.stack(pooled, 1)
    w = F.adaptive_weights(params, names, {m: pooled[i] for i, m in enumerate(names)}, mask)
    fused = (pooled_t * w.unsqueeze(-1)).sum(1)
    zc = F.linear(fused, params["classifier.0.weight"], params["classifier.0.bias"])
    ac = F._relu(zc, "cls", relu_gate)
    if taps is not None:
        taps["in/cls"], taps["z/cls"], taps["a/cls"] = fused.detach(), zc.detach(), ac
        ac.retain_grad()
    h = F._dropout(ac, p, train, gen, F.SITE_CLS)
    return F.linear(h, params["classifier.3.weight"], params["classifier.3.bias"]), {}


def _cma_cut_value_head(params, prefix, query, key, b, h, num_heads, mask, p, train, gen, site):
    """cma_forward(query, key, value = key) where head h's columns of sample b's V take `key`
    detached: V = key W_v^T + b_v + [(key.detach() - key) sel_b] W_v,h^T.  The added term is exactly
    zero in value and carries minus the gradient that reaches `key` through those columns."""
    w = params[prefix + "value_proj.weight"]
    hd = w.shape[0] // num_heads
    w_cut = torch.zeros_like(w)
    w_cut[h * hd:(h + 1) * hd] = w[h * hd:(h + 1) * hd].detach()
    sel = torch.zeros(key.shape[0], 1, 1, dtype=key.dtype)
    sel[b] = 1.0
    extra = ((key.detach() - key) * sel).matmul(w_cut.t())
    real = hybrid_cpu.linear

    def linear(x, weight, bias):
        out = real(x, weight, bias)
        return out + extra if weight is w else out

    hybrid_cpu.linear = linear
    try:
        return hybrid_cpu.cma_forward(params, prefix, query, key, key, num_heads, mask=mask, p=p, train=train,
                                      gen=gen, site=site)
    finally:
        hybrid_cpu.linear = real


def state():
    return hybrid_state(CASE.names, CASE.dims, CASE.hidden, CASE.classes, CASE.seed)


@functools.lru_cache(maxsize=None)
def references():
    """(float64 oracle, fp32 oracle, the fp32 pass's taps), computed once and left unchanged.  The
    float64 pass takes the fp32 pass's ReLU decisions within rounding of zero, as the GPU module's
    takes the device's; it is run a second time only if one of them differs from its own."""
    sd = state()
    taps32, taps64 = {}, {}
    ref32 = oracle_step(CASE, sd, torch.float32, SEED, OFFSET, P_DROP, taps=taps32)
    ref64 = oracle_step(CASE, sd, torch.float64, SEED, OFFSET, P_DROP, taps=taps64)
    wts = {m: torch.from_numpy(sd[f"projections.{m}.0.weight"]) for m in CASE.names}
    wts["cls"] = torch.from_numpy(sd["classifier.0.weight"])
    acts = {layer: taps32[f"a/{layer}"].detach() for layer in wts}
    gates, counts = device_relu_gates(taps64, wts, acts)
    flips = sum(int((sel & (pos != (taps64[f"z/{layer}"] > 0))).sum()) for layer, (sel, pos) in gates.items())
    print(f"BITE pre-activations in the band: {counts}, decided otherwise in fp32: {flips}")
    if flips:
        ref64 = oracle_step(CASE, sd, torch.float64, SEED, OFFSET, P_DROP, relu_gate=gates)
    return ref64, ref32, taps32


def dz_and_input(m):
    """(dZ_m, X'_m) of the fp32 pass as (B L, H) and (B L, D) matrices."""
    _, _, taps = references()
    a, z = taps[f"a/{m}"], taps[f"z/{m}"]
    dz = a.grad * (z > 0).to(z.dtype)
    return dz.reshape(-1, dz.shape[-1]), taps[f"in/{m}"].reshape(-1, taps[f"in/{m}"].shape[-1])


def clone(out):
    return {k: v.clone() for k, v in out.items()}


def plant_a():
    got = clone(references()[1])
    dz, xd = dz_and_input("m0")
    nsplit, kchunk, last = SPLITS["projections.m0"]
    assert (nsplit, kchunk, last) == (65, 64, 4)
    rows = slice((nsplit - 1) * kchunk + last // 32 * 32, dz.shape[0])
    got["projections.m0.0.weight"] -= dz[rows].t() @ xd[rows]
    return got


def plant_b():
    got = clone(references()[1])
    dz, xd = dz_and_input("m0")
    nsplit, kchunk, _ = SPLITS["projections.m0"]
    rows = slice((nsplit // 2) * kchunk, (nsplit // 2 + 1) * kchunk)
    got["projections.m0.0.weight"] -= dz[rows].t() @ xd[rows]
    return got


def plant_c():
    got = clone(references()[1])
    dz, _ = dz_and_input("m2")
    nsplit, kchunk, last = SPLITS["projections.m2"]
    assert (nsplit, kchunk, last) == (56, 96, 50)
    got["projections.m2.0.bias"] -= dz[(nsplit // 2) * kchunk:(nsplit // 2 + 1) * kchunk].sum(0)
    return got


def plant_d():
    got = clone(references()[1])
    L = CASE.seq["m2"]
    assert L == 130 and CASE.mask[1][2] == 0.25 and CASE.mask[0][2] == 1.0
    n = 2 * 128 - L   # sample 1's rows inside tile 1 (flat rows 128..255): l = 0..125
    got["dx/m2"][1, :n] = got["dx/m2"][0, :n]
    return got


def plant_e():
    fwd = functools.partial(planted_forward, drop_value_head=(pair_names(CASE.names).index("m0_to_m2"), 1, 1))
    return oracle_step(CASE, state(), torch.float32, SEED, OFFSET, P_DROP, forward=fwd)


def plant_f():
    fwd = functools.partial(planted_forward, drop_pcol_tile=("m2", 3, 128))
    return oracle_step(CASE, state(), torch.float32, SEED, OFFSET, P_DROP, forward=fwd)


PLANTS = {"a_ragged_tail": plant_a, "b_middle_slab": plant_b, "c_bias_slab": plant_c, "d_dx_neighbour": plant_d,
          "e_value_head": plant_e, "f_pcol_tile": plant_f}
OLD_RULE_PASSES = ()   # observed (printed by the test below): the old rule rejects every one


def test_planted_forward_is_the_oracle():
    """Without a hook the restatement equals oracle.hybrid_cpu.hybrid_forward bit for bit."""
    _, ref32, _ = references()
    mine = oracle_step(CASE, state(), torch.float32, SEED, OFFSET, P_DROP, forward=planted_forward)
    for key in ref32:
        assert torch.equal(mine[key], ref32[key]), key


def test_taps_rebuild_the_weight_gradient():
    """dZ^T X' and the column sums of dZ from the taps are the oracle's own projection gradients."""
    _, ref32, _ = references()
    for m in CASE.names:
        dz, xd = dz_and_input(m)
        assert close(dz.t() @ xd, ref32[f"projections.{m}.0.weight"], 1e-5)
        assert close(dz.sum(0), ref32[f"projections.{m}.0.bias"], 1e-5)


def test_unplanted_fp32_oracle_passes():
    ref64, ref32, _ = references()
    bad, _, _ = compare(ref32, ref64, ref32, "BITE unplanted", C, CAP)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("which", list(PLANTS))
def test_planted_defect_is_rejected(which):
    ref64, ref32, _ = references()
    got = PLANTS[which]()
    old = [k for k in ref32 if not close(got[k], ref32[k], OLD_TOL)]
    print(f"BITE {which}: close(got, fp32 oracle, {OLD_TOL:g}) rejects {old if old else 'nothing'}")
    bad, _, _ = compare(got, ref64, ref32, f"BITE {which}", C, CAP)
    print(f"BITE {which}: compare rejects\n  " + "\n  ".join(bad))
    assert bad, f"{which}: the planted defect passed the float64 comparison"
    assert (not old) == (which in OLD_RULE_PASSES), (which, old)
