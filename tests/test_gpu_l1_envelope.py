"""The launch-lean L = 1 step (csrc/l1.hip) across the envelope lean_l1_desc admits, against float64.

The other GPU modules run the lean plan at three shapes only: M = 3 with one partial tile
(tiny_l1), M = 2 / H = 8 / B = 3 (known_answer_2mod) and the C2 shape with 16 exact tiles (c2_l1).
The cases of tests/_l1.py are the smallest shapes that reach what those leave out: M = 4 (three
pairs per key: l1_key_bwd_kernel<FH, 3>, the three-pair branch of pair_key_bwd, twelve pairs, 34
weight-gradient jobs and 48 zero regions -- L1_MAXZ exactly), the <128> forms at M = 2 and M = 4,
several tiles with a ragged last one, B > 256 (the weight gradient's second 256-row chunk, the loss
sum's second stride, 17 and 22 tiles), H = 36, 20 and 100 (zero_pad, the j < H guards, h4 = H / 4
not dividing the 512 float4 slots), head dims 4, 12, 16, 20 and 128, C = 16, D_m from 4 to 128 in
one model, p = 0 on the train step, and the capacity fallback of mmf_hybrid_train_step_part
(l1_m4_b352: 264 workgroups, over l1_train_capacity on a 256-CU part).

Per case, at "highest":
  a. the plan that ran, from the library's launch records; the sync words back at zero;
  b. one HybridTrainStep.forward_backward() against the float64 oracle (tests/_l1.compare_step:
     close_sliced per sample with the fp32 oracle's own error as the yardstick, C and CAP of
     tests/test_gpu_attn_headdims.py; the device's ReLU decisions within rounding of zero handed to
     the oracle, dropout replayed from Philox; query / key projection gradients and the input
     gradients of fully masked samples exact zeros);
  c. the one-call step == forward -> cross-entropy -> backward as three calls, bit for bit over two
     steps (which puts l1_pair_fwd_kernel, l1_head_fwd_kernel, l1_head_bwd_kernel,
     l1_key_bwd_kernel<FH, NPK> and cross_entropy_kernel under (b) at every shape);
and once: the module path at M = 4 (twelve attention maps, each the mask indicator), and the fused
clip partials at 484 weight-gradient tiles.  tests/test_l1_envelope_bite.py shows that
(b)'s rule rejects the defects these shapes exist to find.

Measured worst e_dev / max(e_32, 2^-24) per case (profiles/l1_envelope/pytest.log):
    l1_m4_ragged 24.80 (gating_layers.m3.bias)    l1_m4_full128 12.29 (gating_layers.m3.bias)
    l1_m2_full128 2.58 (classifier.0.bias)        l1_m2_b260 4.58 (dx/m1)
    l1_m3_h100 5.68 (gating_layers.m0.bias)       l1_m4_b352 7.71 (dx/m3)
    the module path of l1_m4_ragged: logits 1.38, fusion weights 1.77
The two worst are gating biases, the cancelling sum (dscore = w (g - sum w g)) that the docstring of
tests/test_gpu_attn_headdims.py describes: the device is 1.5e-6 and 8.2e-7 of the tensor's maximum
from float64 there and the fp32 oracle happens to sit at the 2^-24 floor.  The largest e_dev of any
tensor is 5.0e-6 (l1_m4_full128 gating_layers.m1.bias): CAP never binds, C = 32 holds on every
tensor, nothing is relaxed.  (c) holds bit for bit at every shape.  l1_m4_b352 took the split plan
(264 workgroups against a capacity of 256).
"""
import functools

import pytest
import torch

from _l1 import (BY_NAME, DROPOUT, L1_CASES, OFFSET, SEED, _three_calls, case_labels, compare_step, is_qk,
                 oracle_step)
from _util import close_sliced, device_relu_gates, oracle_hybrid, sliced_ratio, sliced_report
from cases import hybrid_inputs, hybrid_state
from test_gpu_attn_headdims import C, CAP

pytestmark = pytest.mark.gpu
NAMES = [c.name for c in L1_CASES]
SPLIT = ("l1_pair_fwd_kernel", "l1_head_fwd_kernel", "cross_entropy_kernel", "l1_head_bwd_kernel",
         "l1_key_bwd_kernel", "l1_wgrad_kernel")


@pytest.fixture(scope="module")
def env(pkg_on_path):
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible")
    import fusion
    import mmf_native
    import train_step
    mmf_native.lib()
    return fusion, mmf_native, train_step


@pytest.fixture
def highest():
    prev = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision("highest")
    try:
        yield
    finally:
        torch.set_float32_matmul_precision(prev)


def build_model(fusion, case):
    model = fusion.HybridFusion({m: case.dims[m] for m in case.names}, hidden_dim=case.hidden,
                                num_classes=case.classes, num_heads=case.heads, dropout=DROPOUT[case.name])
    sd = hybrid_state(case.names, case.dims, case.hidden, case.classes, case.seed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    model = model.cuda()
    model._rng_state.copy_(torch.tensor([SEED, OFFSET], dtype=torch.int64))
    return model, sd


def build_step(env, case, **kw):
    fusion, _, train_step = env
    model, sd = build_model(fusion, case)
    feats_np, mask_np, _ = hybrid_inputs(case)
    step = train_step.HybridTrainStep(model, [torch.from_numpy(feats_np[m]).cuda() for m in case.names],
                                      torch.from_numpy(mask_np).cuda(), case_labels(case).cuda(), **kw)
    return model, sd, step


def kernel_names(launches):
    return [k for _, k, *_ in launches]


def step_outputs(st):
    return [t.detach().cpu().clone() for t in (st.logits, st.losses, st.dlogits, st.fw, st.grad, *st.dx, st.rng)]


@functools.lru_cache(maxsize=None)
def _device_step(env, name):
    """One forward_backward() of the case on the device, run once and shared by (a) and (b): the
    kernels that ran, the sync words, every output, the saved activations."""
    _, nat, _ = env
    case = BY_NAME[name]
    prev = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision("highest")
    try:
        _, sd, step = build_step(env, case)
        seed, offset = (int(v) for v in step.rng.tolist())
        nat.profile_begin()
        step.forward_backward()
        torch.cuda.synchronize()
        _, launches = nat.profile_end()
    finally:
        torch.set_float32_matmul_precision(prev)
    out = {"ran": kernel_names(launches), "sync_nonzero": int(step.sync.count_nonzero()), "sd": sd,
           "rng": (seed, offset)}
    step.check_status()   # (raises if a bounded wait of the one-launch step gave up)
    got = {"logits": step.logits.cpu(), "loss": step.loss.reshape(()).cpu()}
    got.update({f"dx/{m}": step.dx[i].cpu() for i, m in enumerate(case.names)})
    got.update({n: g.cpu() for n, g in step.named_grads().items()})
    out["got"] = got
    acts = {m: step.saved_activation("proj", i).cpu() for i, m in enumerate(case.names)}
    acts["cls"] = step.saved_activation("cls_hidden").cpu()
    out["acts"] = acts
    return out


def plan_of(ran):
    """"fused" (l1_fwd_loss_kernel + l1_wgrad_kernel), "split" (the six launches of the separate
    kernels) or None."""
    kinds = {k.split("<")[0] for k in ran}
    if kinds == {"l1_fwd_loss_kernel", "l1_wgrad_kernel"}:
        return "fused"
    if kinds == set(SPLIT):
        return "split"
    return None


@pytest.mark.parametrize("name", NAMES)
def test_plan_that_ran(env, name):
    dev = _device_step(env, name)
    ran = dev["ran"]
    print(f"L1ENV {name} kernels: {sorted(set(ran))}")
    assert not any(k.startswith(("sk_", "attn_")) for k in ran), ran
    form = "<128>" if name.endswith("full128") else "<0>"
    if name == "l1_m4_b352":
        plan = plan_of(ran)
        print(f"L1ENV {name} plan: {plan}")
        assert plan in ("fused", "split"), sorted(set(ran))
    else:
        assert f"l1_fwd_loss_kernel{form}" in ran, ran
        assert "l1_wgrad_kernel" in ran, ran
        assert not any(k.startswith(("cross_entropy_kernel", "l1_head", "l1_key_bwd")) for k in ran), ran
    assert not any(k.startswith("l1_") and "<" in k and not k.endswith(form) for k in ran), (form, ran)
    assert dev["sync_nonzero"] == 0


@pytest.mark.parametrize("name", NAMES)
def test_step_vs_fp64(env, name):
    case = BY_NAME[name]
    dev = _device_step(env, name)
    sd, got = dev["sd"], dev["got"]
    seed, offset = dev["rng"]
    taps = {}
    oracle_step(case, torch.float64, seed, offset, taps=taps)
    wts = {m: torch.from_numpy(sd[f"projections.{m}.0.weight"]) for m in case.names}
    wts["cls"] = torch.from_numpy(sd["classifier.0.weight"])
    gates, counts = device_relu_gates(taps, wts, dev["acts"])
    print(f"L1ENV {name} pre-activations in the band: {counts}")
    ref64 = oracle_step(case, torch.float64, seed, offset, relu_gate=gates)
    ref32 = oracle_step(case, torch.float32, seed, offset, relu_gate=gates)
    nqk = sum(1 for k in ref64 if is_qk(k))
    assert nqk == 4 * len(case.names) * (len(case.names) - 1)   # (M = 4: the 48 zero regions)
    bad = compare_step(case, got, ref64, ref32, name)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", NAMES)
def test_one_call_equals_three_calls(env, highest, name):
    """Two consecutive steps from the same dropout state, as one call and as forward ->
    cross-entropy -> backward: logits, losses, dlogits, fusion weights, the flat gradient, every dX
    and the advanced dropout state bit for bit."""
    _, nat, _ = env
    case = BY_NAME[name]
    runs = []
    for split in (False, True):
        _, _, st = build_step(env, case)
        nat.profile_begin()
        outs = []
        for _ in range(2):
            _three_calls(st, nat) if split else st.forward_backward()
            torch.cuda.synchronize()
            outs.append(step_outputs(st))
        _, launches = nat.profile_end()
        ran = kernel_names(launches)
        if split:
            print(f"L1ENV {name} three calls: {sorted(set(ran))}")
            assert plan_of(ran) == "split", sorted(set(ran))
        else:
            assert int(st.sync.count_nonzero()) == 0
            st.check_status()
        runs.append(outs)
    labels = ["logits", "losses", "dlogits", "fusion weights", "grad"] + [f"dx/{m}" for m in case.names] + ["rng"]
    for k, (step_a, step_b) in enumerate(zip(*runs)):
        for what, a, b in zip(labels, step_a, step_b):
            assert torch.equal(a, b), (name, k, what, float((a.double() - b.double()).abs().max()))
    if DROPOUT[name] > 0:
        assert int(runs[0][1][-1][1]) == OFFSET + 2   # the stream advanced once per step


def test_module_path_m4_ragged(env, highest):
    """HybridFusion.forward in eval mode at M = 4: twelve attention maps, each the key's mask
    indicator exactly; logits and fusion weights against float64, per sample."""
    fusion, nat, _ = env
    case = BY_NAME["l1_m4_ragged"]
    model, _ = build_model(fusion, case)
    model = model.eval()
    feats_np, mask_np, _ = hybrid_inputs(case)
    nat.profile_begin()
    with torch.no_grad():
        logits, info = model({m: torch.from_numpy(v).cuda() for m, v in feats_np.items()},
                             torch.from_numpy(mask_np).cuda(), return_attention=True)
    torch.cuda.synchronize()
    _, launches = nat.profile_end()
    ran = kernel_names(launches)
    print(f"L1ENV {case.name} module path: {sorted(set(ran))}")
    assert "l1_pair_fwd_kernel<0>" in ran and "l1_head_fwd_kernel<0>" in ran, ran
    maps = info["attention_maps"]
    assert len(maps) == 12
    mask = torch.from_numpy(mask_np)
    for key, amap in maps.items():
        k = case.names.index(key.split("_to_")[1])
        want = (mask[:, k] != 0).float().reshape(-1, 1, 1, 1).expand(case.batch, case.heads, 1, 1)
        assert torch.equal(amap.cpu(), want), key
    ref64, _, _ = oracle_hybrid(case, torch.float64)
    ref32, _, _ = oracle_hybrid(case, torch.float32)
    got = {"logits": logits.cpu(), "fusion_weights": info["fusion_weights"].cpu()}
    bad = []
    for key, g in got.items():
        ratio, e_dev = sliced_ratio(g, ref64[key], ref32[key], slice_dim=0)
        print(f"L1ENV {case.name} module {key}: ratio {ratio:.2f}, e_dev {e_dev:.3e}")
        if not close_sliced(g, ref64[key], ref32[key], slice_dim=0, c=C, cap=CAP):
            bad.append(f"{key}: " + sliced_report(g, ref64[key], ref32[key], slice_dim=0, c=C, cap=CAP))
    assert not bad, "\n".join(bad)


def test_fused_clip_partials_484_tiles(env, highest):
    """l1_m4_full128: 484 weight-gradient tiles, one clip partial each.  One clipped step() with the
    partials from the weight-gradient launch (fuse_clip) and one with the optimizer's own reduction
    pass: the same gradient bits and step count, the norm within 1e-5 of the float64 2-norm of the
    device's own gradient, clipping active."""
    case = BY_NAME["l1_m4_full128"]
    runs = []
    for fuse in (True, False):
        _, _, st = build_step(env, case, gradient_clip_norm=0.05, fuse_clip=fuse)
        assert st.fuse_clip == fuse
        st.step()
        torch.cuda.synchronize()
        st.check_status()
        g = st.grad.cpu().clone()
        norm, want = float(st.grad_norm.item()), float(g.double().norm())
        print(f"L1ENV {case.name} fuse_clip={fuse}: grad_norm {norm:.9e}, float64 {want:.9e}, "
              f"clip_coef {float(st.clip_coef.item()):.6e}")
        assert abs(norm - want) <= 1e-5 * want
        assert float(st.clip_coef.item()) < 1.0
        runs.append((g, int(st.step_dev.item())))
    assert torch.equal(runs[0][0], runs[1][0])
    assert runs[0][1] == runs[1][1] == 1
