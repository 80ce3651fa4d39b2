"""The HybridFusion attention kernels at head dims 48, 24 and 12 and the general plan at 64,
against the float64 oracle.

The pooled, lean, long-key and general-plan kernels of csrc/attention.hip are otherwise tested
at head dims 8, 16, 32 and 64 only: never with hd < HDP (the zero padding of the LDS images, the
d0 + 3 < hd store guards), the lean <64> forms never in train mode, the general plan never at
<64>.  The cases below are the smallest shapes that reach those forms.

The projections and the classifier have a ReLU, and no seed keeps every pre-activation clear of
zero (seq_general_hd64 has 1 to 8 of them within 1e-5 * (|x| @ |W|^T) on every seed tried), so
the cases run through train_step.HybridTrainStep as tests/test_gpu_headline.py does: one
forward_backward(), the device's ReLU decisions read back from its saved activations and handed
to the oracle for the pre-activations within rounding of zero (tests/_util.device_relu_gates,
which also asserts that the device passes nothing outside that band), the attention and
projection dropout replayed from Philox (tests/_philox.py).  Dropout 0.1, except seq_hd12 at 0
so that the DROP = false forms are compared too.

Comparison at "highest": tests/_util.close_sliced, per sample, against the float64 oracle with
the fp32 oracle's own error as the yardstick -- the same C and CAP as
tests/test_gpu_attn_headdims.py (its docstring has the rule and the measured ratios).

Measured worst e_dev / max(e_32, 2^-24) per case: seq_hd48 2.37, seq_lean_hd48 15.32
(gating_layers.a.weight, a cancelling sum), seq_lean_hd24 2.76, seq_hd12 3.55, seq_long_hd48
7.16, seq_general_hd64 4.20; the largest e_dev 5.2e-6 (seq_hd12 gating_layers.a.bias).
HybridTrainStep and the library accept every one of these shapes.

At "medium" each case runs through the module in train mode under the norm rule of
tests/test_gpu_bf16.py (the fp32 oracle as reference, the bf16-operand oracle as the error bf16
costs by itself).
"""
import functools

import pytest
import torch

import _seqstep
from _philox import mask_provider
from _seqstep import OFFSET, SEED
from _util import bf16_matmul_mode
from cases import HybridCase, hybrid_inputs, hybrid_state
from test_gpu_attn_headdims import C, CAP

pytestmark = pytest.mark.gpu

POOL_CASES = [
    # attn_pool_fwd_kernel<64>, attn_pool_bwd_dq_kernel<64>, attn_pool_bwd_dk_kernel<64>, padded
    HybridCase("seq_hd48", ["a", "b"], {"a": 20, "b": 12}, {"a": 40, "b": 72}, batch=2, hidden=96, heads=2,
               classes=4, seed=301, mask=[[1, 1], [1, 0.5]]),
    # attn_pool_fwd_lean<64> and attn_pool_bwd_fused_lean<64> in train mode, padded
    HybridCase("seq_lean_hd48", ["a", "b"], {"a": 32, "b": 64}, {"a": 64, "b": 96}, batch=2, hidden=96, heads=2,
               classes=4, seed=302, mask=[[1, 1], [1, 0]]),
    # the lean <32> forms padded; odd batch
    HybridCase("seq_lean_hd24", ["a", "b"], {"a": 32, "b": 16}, {"a": 32, "b": 64}, batch=3, hidden=96, heads=4,
               classes=5, seed=303, mask=[[1, 1], [0, 1], [1, 0.5]]),
    # hd % 8 != 0: off the tail fast path and the fused-plan check of csrc/hybrid.hip
    HybridCase("seq_hd12", ["a", "b", "c"], {"a": 16, "b": 24, "c": 8}, {"a": 16, "b": 40, "c": 9}, batch=2,
               hidden=48, heads=4, classes=5, seed=304, mask=[[1, 1, 1], [0, 1, 0.5]]),
    # attn_poolL_*<64> padded; 3 key chunks; Lk % 8 != 0
    HybridCase("seq_long_hd48", ["a", "b"], {"a": 32, "b": 48}, {"a": 160, "b": 300}, batch=2, hidden=96, heads=2,
               classes=4, seed=305, mask=[[1, 1], [0.5, 1]]),
    # heads x Lk = 4104 > POOL_PB_CAP: the general flash plan at <64>
    HybridCase("seq_general_hd64", ["x", "y"], {"x": 16, "y": 8}, {"x": 8, "y": 2052}, batch=1, hidden=128,
               heads=2, classes=3, seed=306, mask=[[1, 1]]),
]
BY_NAME = {c.name: c for c in POOL_CASES}
DROPOUT = {c.name: 0.0 if c.name == "seq_hd12" else 0.1 for c in POOL_CASES}
EXPECT = {   # name prefixes of the instantiations each case exists for
    "seq_hd48": ["attn_pool_fwd_kernel<64", "attn_pool_bwd_dq_kernel<64", "attn_pool_bwd_dk_kernel<64"],
    "seq_lean_hd48": ["attn_pool_fwd_lean<64", "attn_pool_bwd_fused_lean<64"],
    "seq_lean_hd24": ["attn_pool_fwd_lean<32", "attn_pool_bwd_fused_lean<32"],
    "seq_hd12": ["attn_pool_fwd_kernel<32", "attn_pool_bwd_dq_kernel<32", "attn_pool_bwd_dk_kernel<32"],
    "seq_long_hd48": ["attn_poolL_lse_kernel<64", "attn_poolL_colsum_kernel<64", "attn_poolL_dq_kernel<64",
                      "attn_pool_bwd_dk_kernel<64"],
    "seq_general_hd64": ["attn_fwd_kernel<64, 0", "attn_bwd_dkv_kernel<64", "attn_bwd_dq_kernel<64"],
}


@pytest.fixture(scope="module")
def env(pkg_on_path):
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible")
    import fusion
    import mmf_native
    import train_step
    mmf_native.lib()
    return fusion, mmf_native, train_step


def build_model(fusion, case):
    return _seqstep.build_model(fusion, case, DROPOUT[case.name])


@pytest.mark.parametrize("name", [c.name for c in POOL_CASES])
def test_hybrid_step_vs_fp64(env, name):
    fusion, nat, train_step = env
    case = BY_NAME[name]
    prev = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision("highest")
    try:
        step, sd, got, launches, seed, offset = _seqstep.device_step(nat, fusion, train_step, case, DROPOUT[name])
    finally:
        torch.set_float32_matmul_precision(prev)
    ran = [k for _, k, *_ in launches]
    print(f"HEADDIMS {name} kernels: {sorted(set(ran))}")
    for want in EXPECT[name]:
        assert any(k.startswith(want) for k in ran), (want, sorted(set(ran)))

    ref64, ref32 = _seqstep.gated_references(step, case, sd, seed, offset, DROPOUT[name], f"HEADDIMS {name}")
    bad, _, _ = _seqstep.compare(got, ref64, ref32, f"HEADDIMS {name}", C, CAP)
    assert not bad, "\n".join(bad)


@functools.lru_cache(maxsize=None)
def medium_references(name):
    """(fp32 oracle, bf16-operand oracle) of the module's train-mode call on the case: logits,
    input gradients and parameter gradients of sum(logits * G)."""
    from oracle.hybrid_cpu import hybrid_forward
    case = BY_NAME[name]
    p = DROPOUT[name]
    sd = hybrid_state(case.names, case.dims, case.hidden, case.classes, case.seed)
    feats_np, mask_np, grad_np = hybrid_inputs(case)

    def run():
        params = {k: torch.from_numpy(v).requires_grad_(True) for k, v in sd.items()}
        xs = {m: torch.from_numpy(v).requires_grad_(True) for m, v in feats_np.items()}
        ref, _ = hybrid_forward(params, case.names, xs, torch.from_numpy(mask_np), case.heads, p=p, train=True,
                                gen=mask_provider(SEED, OFFSET, p))
        (ref * torch.from_numpy(grad_np)).sum().backward()
        out = {"logits": ref.detach()}
        out.update({f"dx/{m}": xs[m].grad for m in case.names})
        out.update({n: p_.grad for n, p_ in params.items()})
        return out

    ref = run()
    with bf16_matmul_mode():
        emu = run()
    return ref, emu


@pytest.mark.parametrize("name", [c.name for c in POOL_CASES])
def test_hybrid_medium(env, name):
    from test_gpu_bf16 import _bf16_kernels_ran, group_scale, logits_ok, norm_ok
    fusion, nat, _ = env
    case = BY_NAME[name]
    feats_np, mask_np, grad_np = hybrid_inputs(case)
    prev = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision("medium")
    try:
        model, _ = build_model(fusion, case)
        model = model.train()
        model._rng_state.copy_(torch.tensor([SEED, OFFSET], dtype=torch.int64))
        feats = {m: torch.from_numpy(v).cuda().requires_grad_(True) for m, v in feats_np.items()}
        nat.profile_begin()
        logits = model(feats, torch.from_numpy(mask_np).cuda())
        (logits * torch.from_numpy(grad_np).cuda()).sum().backward()
        torch.cuda.synchronize()
        _, launches = nat.profile_end()
    finally:
        torch.set_float32_matmul_precision(prev)
    ran, mfma = _bf16_kernels_ran(nat, launches)
    assert ran, mfma
    ref, emu = medium_references(name)
    ok, e = logits_ok(logits.detach().cpu(), ref["logits"])
    assert ok, e
    grads = [k for k in ref if k != "logits"]
    S = group_scale([ref[k] for k in grads])
    for m in case.names:
        ok, e = norm_ok(feats[m].grad, ref[f"dx/{m}"], emu[f"dx/{m}"], S)
        assert ok, (m, e)
    for n, prm in model.named_parameters():
        ok, e = norm_ok(prm.grad, ref[n], emu[n], S)
        assert ok, (n, e)
