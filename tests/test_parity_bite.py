"""The float64 comparison of tests/test_gpu_attn_headdims.py rejects the defects it exists for.

No device: "got" is the fp32 CPU oracle's own output with one defect planted -- a dropped tail
key, a padded feature column left out of QK^T, a query row whose gradient was never written, a
sample whose gradient is off by 2e-4 -- and compare_fp64 (close_sliced with the module's C and
CAP) must reject it, while the unplanted fp32 oracle passes.  Whether the suite's older rule,
close(got, ref, 1e-3, 1e-5), notices each defect is printed, not asserted.
"""
import pytest
import torch

from _util import close
from cases import cma_inputs, cma_state
from test_gpu_attn_headdims import BY_NAME, compare_fp64, references


def planted_oracle(case, drop_key=None, skip_col=None):
    """The fp32 oracle of oracle_cma (oracle/hybrid_cpu.cma_forward, eval mode) with a defect
    planted in the forward: drop_key = (sample, head, key): that key left out of the softmax;
    skip_col = (head, column): that feature column left out of QK^T."""
    sd = cma_state(case.query_dim, case.key_dim, case.hidden, case.seed)
    params = {k: torch.from_numpy(v).requires_grad_(True) for k, v in sd.items()}
    q_np, k_np, v_np, mask, grad = cma_inputs(case)
    qt, kt, vt = (torch.from_numpy(a).requires_grad_(True) for a in (q_np, k_np, v_np))
    B, Lq, Lk, H, h = case.batch, case.lq, case.lk, case.hidden, case.heads
    hd = H // h
    lin = lambda x, n: x.matmul(params[f"{n}.weight"].t()) + params[f"{n}.bias"]  # noqa: E731
    q = lin(qt, "query_proj").reshape(B, Lq, h, hd).permute(0, 2, 1, 3)
    k = lin(kt, "key_proj").reshape(B, Lk, h, hd).permute(0, 2, 1, 3)
    v = lin(vt, "value_proj").reshape(B, Lk, h, hd).permute(0, 2, 1, 3)
    if skip_col is not None:
        keep = torch.ones(h, hd)
        keep[skip_col[0], skip_col[1]] = 0.0
        q = q * keep.reshape(1, h, 1, hd)
    s = q.matmul(k.transpose(-1, -2)) * (hd ** -0.5)
    if mask is not None:
        mt = torch.from_numpy(mask)
        mk = mt.reshape(B, 1) if mt.dim() == 1 else mt
        s = s.masked_fill((mk == 0).reshape(B, 1, 1, -1), float("-inf"))
    if drop_key is not None:
        gone = torch.zeros(B, h, 1, Lk, dtype=torch.bool)
        gone[drop_key[0], drop_key[1], 0, drop_key[2]] = True
        s = s.masked_fill(gone, float("-inf"))
    a = torch.nan_to_num(torch.softmax(s, dim=-1), nan=0.0, posinf=0.0, neginf=0.0)
    att = lin(a.matmul(v).permute(0, 2, 1, 3).reshape(B, Lq, H), "out_proj")
    (att * torch.from_numpy(grad)).sum().backward()
    out = {"attended": att.detach(), "weights": a.detach(), "dquery": qt.grad, "dkey": kt.grad, "dvalue": vt.grad}
    for name, p in params.items():
        out[f"grad/{name}"] = p.grad
    return out


def plant_a():   # hd48_edge: the last key (the one-key second chunk) dropped for one (sample, head)
    return planted_oracle(BY_NAME["hd48_edge"], drop_key=(1, 0, 64))


def plant_b():   # hd48_edge: the last real feature column of one head left out of QK^T
    return planted_oracle(BY_NAME["hd48_edge"], skip_col=(1, 47))


def plant_c():   # hd64_blocks: dquery of the one-row second query block never written
    out = {k: v.clone() for k, v in references("hd64_blocks")[1].items()}
    out["dquery"][1, 128] = 0.0
    return out


def plant_d():   # hd40_1d: the live sample behind the masked one off by 2e-4
    out = {k: v.clone() for k, v in references("hd40_1d")[1].items()}
    out["dvalue"][2] *= 1.0 + 2e-4
    return out


PLANTS = {"a_drop_tail_key": ("hd48_edge", plant_a), "b_skip_padded_column": ("hd48_edge", plant_b),
          "c_unwritten_dquery_row": ("hd64_blocks", plant_c), "d_scaled_dvalue": ("hd40_1d", plant_d)}


def test_planted_oracle_is_the_oracle():
    """Without a defect the restatement above equals oracle_cma bit for bit."""
    for name in ("hd48_edge", "hd40_1d"):
        _, ref32 = references(name)
        mine = planted_oracle(BY_NAME[name])
        for key in ref32:
            assert torch.equal(mine[key], ref32[key]), (name, key)


@pytest.mark.parametrize("name", ["hd48_edge", "hd64_blocks", "hd40_1d"])
def test_unplanted_fp32_oracle_passes(name):
    ref64, ref32 = references(name)
    bad = compare_fp64(BY_NAME[name], ref32, ref64, ref32, f"{name} unplanted")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("which", list(PLANTS))
def test_planted_defect_is_rejected(which):
    name, plant = PLANTS[which]
    ref64, ref32 = references(name)
    got = plant()
    old = [k for k in ref32 if not close(got[k], ref32[k], 1e-3, 1e-5)]
    print(f"BITE {which}: close(got, ref, 1e-3, 1e-5) rejects {old if old else 'nothing'}")
    bad = compare_fp64(BY_NAME[name], got, ref64, ref32, f"{name} {which}")
    print(f"BITE {which}: close_sliced rejects\n  " + "\n  ".join(bad))
    assert bad, f"{which}: the planted defect passed the float64 comparison"
