"""One HybridTrainStep.forward_backward() against the float64 oracle: the mechanics shared by
tests/test_gpu_pool_headdims.py and tests/test_gpu_gemm_envelope.py (and, for the comparison
alone, tests/test_gemm_envelope_bite.py).

The projections and the classifier have a ReLU, and no seed keeps every pre-activation clear of
zero, so the device's ReLU decisions are read back from its saved activations and handed to the
oracle for the pre-activations within rounding of zero (tests/_util.device_relu_gates, which also
asserts that the device passes nothing outside that band); the input, projection, attention and
classifier dropout are replayed from Philox (tests/_philox.py).

compare() is the rule: tests/_util.close_sliced against the float64 oracle with the fp32 oracle's
own error as the yardstick, logits and dx/<m> one slice per sample, every parameter gradient and
the loss one slice, *key_proj.bias (mathematically zero) under tests/_util.zero_grad_bound.
"""
import numpy as np
import torch

from _philox import mask_provider
from _util import EPS32, close_sliced, device_relu_gates, sliced_ratio, sliced_report, zero_grad_bound
from cases import hybrid_inputs, hybrid_state

SEED, OFFSET = 0x2468_ACE0_1357, 3


def case_labels(case):
    return torch.from_numpy(np.random.default_rng(case.seed + 31337).integers(0, case.classes, case.batch))


def build_model(fusion, case, dropout):
    model = fusion.HybridFusion({m: case.dims[m] for m in case.names}, hidden_dim=case.hidden,
                                num_classes=case.classes, num_heads=case.heads, dropout=dropout)
    sd = hybrid_state(case.names, case.dims, case.hidden, case.classes, case.seed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return model.cuda(), sd


def oracle_step(case, sd, dtype, seed, offset, dropout, taps=None, relu_gate=None, forward=None):
    """forward -> CE(label_smoothing 0.05) -> backward of the oracle under the replayed masks:
    {logits, loss, dx/<m>, <parameter name>}.  forward: a stand-in for oracle.hybrid_cpu.hybrid_forward
    with its signature (tests/test_gemm_envelope_bite.py plants defects through one)."""
    from oracle.hybrid_cpu import cross_entropy_ls, hybrid_forward
    feats_np, mask_np, _ = hybrid_inputs(case)
    params = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in sd.items()}
    xs = {m: torch.from_numpy(v).to(dtype).requires_grad_(True) for m, v in feats_np.items()}
    logits, _ = (forward or hybrid_forward)(params, case.names, xs, torch.from_numpy(mask_np).to(dtype), case.heads,
                                            p=dropout, train=True, gen=mask_provider(seed, offset, dropout),
                                            taps=taps, relu_gate=relu_gate)
    loss = cross_entropy_ls(logits, case_labels(case))
    loss.backward()
    out = {"logits": logits.detach(), "loss": loss.detach()}
    out.update({f"dx/{m}": xs[m].grad for m in case.names})
    out.update({n: p_.grad for n, p_ in params.items()})
    return out


def make_step(fusion, train_step, case, dropout, rng=(SEED, OFFSET)):
    """(HybridTrainStep on the case's weights and inputs with its rng pinned, the weights)."""
    model, sd = build_model(fusion, case, dropout)
    feats_np, mask_np, _ = hybrid_inputs(case)
    step = train_step.HybridTrainStep(model, [torch.from_numpy(feats_np[m]).cuda() for m in case.names],
                                      torch.from_numpy(mask_np).cuda(), case_labels(case).cuda())
    step.rng.copy_(torch.tensor(list(rng), dtype=torch.int64))
    return step, sd


def step_outputs(step, case):
    """{logits, loss, dx/<m>, <parameter name>} of the step's last forward_backward(), on the host."""
    got = {"logits": step.logits.cpu(), "loss": step.loss.reshape(()).cpu()}
    got.update({f"dx/{m}": step.dx[i].cpu() for i, m in enumerate(case.names)})
    got.update({n: g.cpu() for n, g in step.named_grads().items()})
    return got


def device_step(nat, fusion, train_step, case, dropout):
    """One profiled forward_backward() at the current matmul precision:
    (step, weights, outputs, launch records, seed, offset)."""
    step, sd = make_step(fusion, train_step, case, dropout)
    seed, offset = (int(v) for v in step.rng.tolist())
    nat.profile_begin()
    step.forward_backward()
    torch.cuda.synchronize()
    _, launches = nat.profile_end()
    return step, sd, step_outputs(step, case), launches, seed, offset


def gated_references(step, case, sd, seed, offset, dropout, tag):
    """(float64 oracle, fp32 oracle) of the step, both under the device's ReLU decisions for the
    pre-activations within rounding of zero."""
    dev_acts = {m: step.saved_activation("proj", i).cpu() for i, m in enumerate(case.names)}
    dev_acts["cls"] = step.saved_activation("cls_hidden").cpu()
    taps = {}
    oracle_step(case, sd, torch.float64, seed, offset, dropout, taps=taps)
    wts = {m: torch.from_numpy(sd[f"projections.{m}.0.weight"]) for m in case.names}
    wts["cls"] = torch.from_numpy(sd["classifier.0.weight"])
    gates, counts = device_relu_gates(taps, wts, dev_acts)
    print(f"{tag} pre-activations in the band: {counts}")
    ref64 = oracle_step(case, sd, torch.float64, seed, offset, dropout, relu_gate=gates)
    ref32 = oracle_step(case, sd, torch.float32, seed, offset, dropout, relu_gate=gates)
    return ref64, ref32


def compare(got, ref64, ref32, tag, c, cap):
    """(violations, largest e_dev / max(e_32, 2^-24) over the tensors, largest e_dev); prints one
    line per tensor."""
    assert set(got) == set(ref64), (sorted(got), sorted(ref64))
    scale = max(float(ref64[k].abs().max()) for k in ref64 if k not in ("logits", "loss"))
    bad, worst, worst_e = [], 0.0, 0.0
    for key in ref64:
        if key.endswith("key_proj.bias"):
            g, own = float(got[key].abs().max()), float(ref32[key].abs().max())
            bound = zero_grad_bound(ref32[key], scale, c)
            print(f"{tag} {key}: max|got| {g:.3e}, fp32 oracle {own:.3e}, 2^-24 S {EPS32 * scale:.3e}, "
                  f"ratio {g / max(own, EPS32 * scale):.2f}")
            if not g <= bound:
                bad.append(f"{key}: max|got| {g:.3e} > {bound:.3e}")
            continue
        sdim = 0 if key == "logits" or key.startswith("dx/") else None
        ratio, e_dev = sliced_ratio(got[key], ref64[key], ref32[key], slice_dim=sdim)
        print(f"{tag} {key}: ratio {ratio:.2f}, e_dev {e_dev:.3e}")
        worst, worst_e = max(worst, ratio), max(worst_e, e_dev)
        if not close_sliced(got[key], ref64[key], ref32[key], slice_dim=sdim, c=c, cap=cap):
            bad.append(f"{key}: " + sliced_report(got[key], ref64[key], ref32[key], slice_dim=sdim, c=c, cap=cap))
    print(f"{tag} worst ratio {worst:.2f}, largest e_dev {worst_e:.3e}")
    return bad, worst, worst_e
