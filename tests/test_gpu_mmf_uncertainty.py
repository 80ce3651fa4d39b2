"""mmf_uncertainty on the device: the MC reduction against float64 numpy, the fused MC-dropout
forward against sequential forwards (bit for bit) and against the CPU oracle with replayed Philox
masks, the temperature NLL against float64 torch, and TemperatureScaling.calibrate /
UncertaintyWeightedFusion against results recorded from the reference
(tests/golden/gen_uncertainty.py).  Tolerance: the project's 1e-3 fp32 parity unless stated."""
import numpy as np
import pytest
import torch
import torch.nn as nn

from _philox import mask_provider
from _util import close, diff_report, load_fixture, rel_err
from cases import HybridCase, hybrid_inputs, hybrid_state

pytestmark = pytest.mark.gpu
RTOL = 1e-3
SEED, OFFSET, P = 0x1234_5678_9ABC, 7, 0.3


@pytest.fixture(scope="module")
def mods(pkg_on_path):
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible")
    import fusion
    import mmf_native
    import mmf_uncertainty
    return fusion, mmf_uncertainty, mmf_native


# the cases of the same names in tests/test_gpu_train_mode.py: the launch-lean L = 1 plan (2-D
# inputs), the pooled plan, and the general plan (heads x Lk beyond the pooled helpers' budget)
CASES = {
    "train_l1": HybridCase("train_l1", ["a", "b", "c"], {"a": 12, "b": 20, "c": 16},
                           {"a": 0, "b": 0, "c": 0}, batch=8, hidden=32, heads=4, classes=5, seed=52,
                           mask=[[1, 1, 1], [1, 0, 1], [0, 0, 1], [0, 0, 0], [1, 1, 0.5]]),
    "train_pooled": HybridCase("train_pooled", ["m0", "m1", "m2"], {"m0": 24, "m1": 32, "m2": 16},
                               {"m0": 16, "m1": 24, "m2": 8}, batch=4, hidden=32, heads=4, classes=5, seed=51,
                               mask=[[1, 1, 1], [1, 0, 1], [0, 0, 0], [0.5, 1, 0]]),
    "train_general_long": HybridCase("train_general_long", ["x", "y"], {"x": 16, "y": 8},
                                     {"x": 20, "y": 140}, batch=2, hidden=64, heads=2, classes=3, seed=53,
                                     mask=[[1, 1], [1, 0]]),
}


def _model(fusion, case, seed=None):
    sd = hybrid_state(case.names, case.dims, case.hidden, case.classes, case.seed if seed is None else seed)
    model = fusion.HybridFusion({m: case.dims[m] for m in case.names}, hidden_dim=case.hidden,
                                num_classes=case.classes, num_heads=case.heads, dropout=P)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return model.cuda(), sd


def _set_rng(model):
    model._rng_state.copy_(torch.tensor([SEED, OFFSET], dtype=torch.int64))


def _inputs(case):
    feats_np, mask_np, _ = hybrid_inputs(case)
    return feats_np, mask_np, {m: torch.from_numpy(v).cuda() for m, v in feats_np.items()}, torch.from_numpy(mask_np).cuda()


def _reduce64(stack):
    """src/uncertainty.py:58-66 in float64 numpy over an (S, B, C) stack."""
    z = np.asarray(stack, np.float64)
    e = np.exp(z - z.max(axis=-1, keepdims=True))
    p = e / e.sum(axis=-1, keepdims=True)
    return z.mean(axis=0), p.mean(axis=0), p.var(axis=0).mean(axis=-1)


# ------------------------------------------------------------------ 1. mc_reduce
MC_SHAPES = [(1, 1, 1), (2, 3, 3), (10, 5, 11), (32, 4, 65), (3, 67, 130)]


@pytest.mark.parametrize("S,B,C", MC_SHAPES, ids=lambda v: str(v))
def test_mc_reduce_matches_float64(mods, S, B, C):
    """A single sample, a single class (all probabilities 1, variance 0), classes beyond one wave's
    64 lanes, rows beyond one workgroup, odd counts.  The variance is a cancellation case: a
    confident model (one logit 4 above the rest) whose samples differ by 1e-2 in the logits, so the
    probabilities differ in the 3rd-5th digit; every ROW must be within 1e-3 of its own float64
    value (a difference-of-squares accumulation is off by 6e-3 to 0.67 here, a Welford / two-pass
    one stays below 1.1e-4)."""
    rng = np.random.default_rng(42)
    base = 2.0 * rng.standard_normal((B, C))
    base[np.arange(B), np.arange(B) % C] += 4.0
    stack = (base + 1e-2 * rng.standard_normal((S, B, C))).astype(np.float32)
    ml, mp, var = torch.ops.mmfusion.mc_reduce(torch.from_numpy(stack).cuda())
    torch.cuda.synchronize()
    ref_ml, ref_mp, ref_var = _reduce64(stack)
    assert rel_err(ml.cpu(), ref_ml) <= RTOL, rel_err(ml.cpu(), ref_ml)
    assert rel_err(mp.cpu(), ref_mp) <= RTOL, rel_err(mp.cpu(), ref_mp)
    got = var.cpu().double().numpy()
    worst = float(np.max(np.abs(got - ref_var) / np.maximum(ref_var, 1e-300)))
    print(f"mc_reduce {(S, B, C)}: variance worst per-row relative error {worst:.3e}")
    assert np.all(np.abs(got - ref_var) <= RTOL * ref_var), (worst, got, ref_var)
    if S == 1 or C == 1:
        assert torch.all(var == 0)
    if C == 1:
        assert torch.all(mp == 1)


def test_mc_reduce_optional_outputs(mods):
    """Each output pointer of mmf_mc_reduce may be NULL."""
    _, _, nat = mods
    L = nat.lib()
    stack = torch.randn(4, 6, 9, device="cuda")
    ml, mp, var = torch.ops.mmfusion.mc_reduce(stack)
    only_var = torch.full((6,), -1.0, device="cuda")
    rc = L.mmf_mc_reduce(4, 6, 9, stack.data_ptr(), None, None, only_var.data_ptr(), nat.stream_ptr(stack.device))
    assert rc == 0, L.mmf_last_error()
    only_mp = torch.full((6, 9), -1.0, device="cuda")
    rc = L.mmf_mc_reduce(4, 6, 9, stack.data_ptr(), None, only_mp.data_ptr(), None, nat.stream_ptr(stack.device))
    assert rc == 0, L.mmf_last_error()
    torch.cuda.synchronize()
    assert torch.equal(only_var, var) and torch.equal(only_mp, mp)


# ------------------------------------------------------------------ 2. fused MC forward
@pytest.mark.parametrize("name", ["train_l1", "train_pooled", "train_general_long"])
def test_fused_mc_forward_equals_sequential_forwards(mods, name):
    fusion, unc, nat = mods
    case, S = CASES[name], 3
    model, _ = _model(fusion, case)
    _, _, feats, mask = _inputs(case)
    model.train()
    _set_rng(model)
    with torch.no_grad():
        want = [model(feats, mask).clone() for _ in range(S)]
    assert int(model._rng_state[1].item()) == OFFSET + S

    model.eval()
    _set_rng(model)
    mc = unc.MCDropoutUncertainty(model, num_samples=S)
    nat.profile_begin()
    mean_logits, variance = mc(feats, mask)
    torch.cuda.synchronize()
    stages, launches = nat.profile_end()
    assert not model.training                                    # the mode is restored
    assert int(model._rng_state[1].item()) == OFFSET + S          # advanced by exactly S
    assert int(model._rng_state[0].item()) == SEED
    # one C-ABI call: its two stages, and one reduction launch under a stable name
    names = [s for s, _ in stages]
    assert "mc.forward" in names and "mc.reduce" in names, names
    assert [k for _, k, *_ in launches].count("mc_reduce_kernel") == 1
    assert mc.logits_stack.shape == (S, case.batch, case.classes)
    for s in range(S):
        assert torch.equal(mc.logits_stack[s], want[s]), s
    assert mean_logits.shape == (case.batch, case.classes) and variance.shape == (case.batch,)
    ml, _, var = torch.ops.mmfusion.mc_reduce(torch.stack(want))
    assert torch.equal(mean_logits, ml) and torch.equal(variance, var)

    model.train()                                                # a model in train mode stays there
    mc(feats, mask)
    assert model.training and int(model._rng_state[1].item()) == OFFSET + 2 * S


# ------------------------------------------------------------------ 3. MCDropoutUncertainty vs the oracle
class _Wrap(nn.Module):
    """Any module that is not HybridFusion itself: forces MCDropoutUncertainty's generic loop."""

    def __init__(self, inner):
        super().__init__()
        self.inner = inner

    def forward(self, *args, **kwargs):
        return self.inner(*args, **kwargs)


@pytest.mark.parametrize("name", ["train_pooled", "train_l1"])
def test_mc_dropout_matches_oracle(mods, name):
    fusion, unc, _ = mods
    from oracle.hybrid_cpu import hybrid_forward
    case, S = CASES[name], 4
    model, sd = _model(fusion, case)
    feats_np, mask_np, feats, mask = _inputs(case)
    model.eval()
    _set_rng(model)
    mean_logits, variance = unc.MCDropoutUncertainty(model, num_samples=S)(feats, mask)
    torch.cuda.synchronize()

    params = {k: torch.from_numpy(v) for k, v in sd.items()}
    xs = {m: torch.from_numpy(v) for m, v in feats_np.items()}
    samples = []
    with torch.no_grad():
        for s in range(S):
            ref, _ = hybrid_forward(params, case.names, xs, torch.from_numpy(mask_np), case.heads, p=P,
                                    train=True, gen=mask_provider(SEED, OFFSET + s, P))
            samples.append(ref.numpy())
    ref_ml, _, ref_var = _reduce64(np.stack(samples))
    assert close(mean_logits.cpu(), ref_ml, RTOL), diff_report(mean_logits.cpu(), ref_ml, RTOL)
    assert close(variance.cpu(), ref_var, RTOL), diff_report(variance.cpu(), ref_var, RTOL)

    # the generic path (S module calls + mc_reduce) gives the same bits
    _set_rng(model)
    generic = unc.MCDropoutUncertainty(_Wrap(model).eval(), num_samples=S)
    ml2, var2 = generic(feats, mask)
    torch.cuda.synchronize()
    assert torch.equal(ml2, mean_logits) and torch.equal(var2, variance)
    assert not model.training and int(model._rng_state[1].item()) == OFFSET + S


# ------------------------------------------------------------------ 4. temperature_nll
@pytest.mark.parametrize("T", [0.5, 1.0, 3.0])
@pytest.mark.parametrize("N,C", [(1, 2), (7, 11), (1000, 11), (4097, 3)])
def test_temperature_nll_matches_float64(mods, N, C, T):
    g = torch.Generator().manual_seed(1000 * N + C)
    logits = 3.0 * torch.randn(N, C, generator=g)
    labels = torch.randint(0, C, (N,), generator=g)
    t64 = torch.tensor([T], dtype=torch.float64, requires_grad=True)
    ref = torch.nn.functional.cross_entropy(logits.double() / t64, labels)
    ref.backward()
    temp = torch.tensor([T], device="cuda")
    lg, lb = logits.cuda(), labels.cuda()
    loss, dtemp = torch.ops.mmfusion.temperature_nll(lg, lb, temp)
    loss2, dtemp2 = torch.ops.mmfusion.temperature_nll(lg, lb, temp)
    torch.cuda.synchronize()
    print(f"temperature_nll {(N, C)} T={T}: loss {float(loss):.7e} (ref {float(ref.detach()):.7e}), "
          f"dT {float(dtemp):.7e} (ref {float(t64.grad):.7e})")
    assert abs(float(loss) - float(ref.detach())) <= RTOL * abs(float(ref.detach()))
    assert abs(float(dtemp) - float(t64.grad)) <= RTOL * abs(float(t64.grad))
    assert torch.equal(loss, loss2) and torch.equal(dtemp, dtemp2)   # fixed-order reduction


def test_temperature_nll_autograd(mods):
    """The operator's autograd formula hands d loss / dT to the temperature."""
    logits, labels = 3.0 * torch.randn(64, 7, device="cuda"), torch.randint(0, 7, (64,), device="cuda")
    temp = torch.tensor([1.5], device="cuda", requires_grad=True)
    loss, dtemp = torch.ops.mmfusion.temperature_nll(logits, labels, temp)
    (2.0 * loss).backward()
    assert torch.allclose(temp.grad, 2.0 * dtemp)


# ------------------------------------------------------------------ 5. TemperatureScaling.calibrate
def test_temperature_scaling_calibrate_matches_reference(mods):
    _, unc, _ = mods
    fx = load_fixture("uncertainty_ref")
    logits, labels = torch.from_numpy(fx["cal/logits"]), torch.from_numpy(fx["cal/labels"])
    t_ref, nll_ref = float(fx["cal/temperature"][0]), float(fx["cal/nll"][0])
    ts = unc.TemperatureScaling()
    with torch.no_grad():
        ts.temperature.fill_(5.0)                      # calibrate() resets T to 1
    ts.calibrate(logits.cuda(), labels.cuda())         # (a CPU parameter migrates to the logits' device)
    assert ts.temperature.device.type == "cuda" and isinstance(ts.temperature, nn.Parameter)
    t = float(ts.temperature.detach().cpu()[0])
    nll = float(torch.nn.functional.cross_entropy(logits.double() / t, labels))
    print(f"calibrate: T {t:.6f} (reference {t_ref:.6f}), NLL {nll:.6f} (reference {nll_ref:.6f})")
    assert abs(t - t_ref) <= RTOL * t_ref
    assert nll <= nll_ref * (1 + RTOL)
    assert nll < float(fx["cal/nll_at_1"][0])          # and it did calibrate
    scaled = ts(logits.cuda())
    assert torch.allclose(scaled.cpu(), logits / t)


# ------------------------------------------------------------------ 6. UncertaintyWeightedFusion
def test_uncertainty_weighted_fusion_matches_reference(mods):
    _, unc, _ = mods
    fx = load_fixture("uncertainty_ref")
    names = ["imu", "video", "hr"]
    preds = {n: torch.from_numpy(fx["uwf/predictions"][:, j].copy()).cuda().requires_grad_(True)
             for j, n in enumerate(names)}
    uncs = {n: torch.from_numpy(fx["uwf/uncertainties"][:, j].copy()).cuda().requires_grad_(True)
            for j, n in enumerate(names)}
    mask = torch.from_numpy(fx["uwf/mask"]).cuda()
    assert mask.shape == (6, 3) and bool((mask[3] == 0).all()) and bool((mask[0] == 1).all())
    fused, weights = unc.UncertaintyWeightedFusion()(preds, uncs, mask)
    (fused * torch.from_numpy(fx["uwf/upstream"]).cuda()).sum().backward()
    torch.cuda.synchronize()
    dpred = torch.stack([preds[n].grad for n in names], dim=1).cpu()
    dunc = torch.stack([uncs[n].grad for n in names], dim=1).cpu()
    for what, got, ref in (("fused", fused.detach().cpu(), fx["uwf/fused"]), ("weights", weights.cpu(), fx["uwf/weights"]),
                           ("dpredictions", dpred, fx["uwf/dpredictions"]),
                           ("duncertainties", dunc, fx["uwf/duncertainties"])):
        assert close(got, ref, RTOL), (what, diff_report(got, ref, RTOL))
    assert torch.all(dunc[3] == 0)                     # the 1 / M fallback row: no gradient in u
    assert torch.allclose(weights[3].cpu(), torch.full((3,), 1.0 / 3.0))


# ------------------------------------------------------------------ 7. EnsembleUncertainty
def test_ensemble_uncertainty_matches_float64(mods):
    fusion, unc, _ = mods
    case = CASES["train_pooled"]
    models = [_model(fusion, case, seed=s)[0].eval() for s in (71, 72)]
    models[1].train()                                   # predict runs it in eval mode and puts it back
    _, _, feats, mask = _inputs(case)
    feats_only = {k: v for k, v in feats.items()}
    probs, variance = unc.EnsembleUncertainty(models).predict_with_uncertainty(feats_only)
    torch.cuda.synchronize()
    assert not models[0].training and models[1].training
    with torch.no_grad():
        logits = [m.eval()(feats_only).cpu().numpy() for m in models]
    _, ref_mp, ref_var = _reduce64(np.stack(logits))
    assert probs.shape == (case.batch, case.classes) and variance.shape == (case.batch,)
    assert close(probs.cpu(), ref_mp, RTOL), diff_report(probs.cpu(), ref_mp, RTOL)
    assert close(variance.cpu(), ref_var, RTOL), diff_report(variance.cpu(), ref_var, RTOL)
