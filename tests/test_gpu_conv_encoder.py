"""ConvSequenceEncoder on the GPU (csrc/conv_encoder.hip) against the reference's recorded
results (tests/golden/convenc_*.npz, gen_convenc.py) and against plain torch.nn on the CPU in
float64, at the project's fp32 parity bound close(got, ref, 1e-3).

Every parity case fixes a seed and asserts, before looking at the device, that it is well posed
(_convenc.check_preconditions): no BatchNorm output within 1e-5 (relative) of the ReLU kink in
float64, and fp32 torch on the CPU within 1e-4 of float64 on every compared tensor.

The conv bias gradients are mathematically zero in training mode (BatchNorm removes the mean);
they are bounded by zero_grad_bound(fp32 torch, scale, c = 4): the device sums the same values in
another order and gets 4x fp32 torch's own noise.  Measured on the MI355X over the cases below:
device max|db| between 0.4x and 2.2x fp32 torch's (0.04x and 0.07x at a conv-bias offset of 100,
where the device keeps the batch mean to twice fp32's digits).

The conv M tile is 128 rows, the weight-gradient stage 32 rows and the reduction chunk 128 rows:
(2, 70, .) puts all three edges inside the second sample, (3, 5, .) several samples in one tile.
"""
import pytest
import torch

from _convenc import (BIAS_KEYS, OUT_DIM, ZERO_GRAD_C, Case, check_buffers, check_parity, check_preconditions,
                      make_case, run_device, run_torch)
from _util import close, diff_report, load_fixture, zero_grad_bound

pytestmark = pytest.mark.gpu

PARITY = [
    Case(3, 1, 17, 64),                     # both taps' neighbours are padding
    Case(3, 2, 17, 64),
    Case(3, 5, 17, 64),                     # several samples per M tile: halos must not leak across samples
    Case(2, 70, 17, 64),                    # a tile / stage / chunk edge inside a sample
    Case(3, 5, 1, 64),                      # channel tails
    Case(2, 9, 8, 256),                     # several N tiles
    Case(2, 70, 128, 64),                   # several K steps, the cooking input width
    Case(3, 37, 17, 64, seed=2, train=False),       # eval: running statistics
    Case(3, 37, 17, 64, bias_offset=100.0),         # variance at a large mean
]
BUFFERS = [Case(3, 37, 17, 64), Case(3, 37, 17, 64, momentum=None)]
_REFS = {}


@pytest.fixture(scope="module")
def enc_mod(pkg_on_path):
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible")
    import encoders
    return encoders


def refs(case: Case):
    """(state dict, x, gout, float64 result, float32 result) of a case, computed once."""
    if case not in _REFS:
        sd, x, gout = make_case(case)
        _REFS[case] = (sd, x, gout, run_torch(case, sd, x, gout, torch.float64),
                       run_torch(case, sd, x, gout, torch.float32))
    return _REFS[case]


@pytest.mark.parametrize("name", ["convenc_eval", "convenc_train"])
def test_reference_fixture(enc_mod, name):
    """The reference's own SequenceEncoder(17, 64, 16, encoder_type='cnn') at (3, 37, 17): its state
    dict loads, and output, dX, every parameter gradient and the post-forward buffers match."""
    fx = {k: torch.from_numpy(v) for k, v in load_fixture(name).items()}
    train = name.endswith("train")
    e = enc_mod.ConvSequenceEncoder(17, 64, OUT_DIM, dropout=0.0)
    e.load_state_dict({k[3:]: v for k, v in fx.items() if k.startswith("sd/")})
    e = e.cuda().train(train)
    x = fx["x"].cuda().requires_grad_(True)
    out = e(x)
    (out * fx["gout"].cuda()).sum().backward()
    assert close(out.detach(), fx["out"], 1e-3), diff_report(out.detach(), fx["out"], 1e-3)
    assert close(x.grad, fx["dx"], 1e-3), diff_report(x.grad, fx["dx"], 1e-3)
    scale = max(float(v.abs().max()) for k, v in fx.items() if k.startswith("grad/"))
    for k, p in e.named_parameters():
        ref = fx[f"grad/{k}"]
        if train and k in BIAS_KEYS:
            assert float(p.grad.abs().max()) <= zero_grad_bound(ref, scale, ZERO_GRAD_C), (k, float(p.grad.abs().max()))
        else:
            assert close(p.grad, ref, 1e-3), (k, diff_report(p.grad, ref, 1e-3))
    for k, b in e.named_buffers():
        ref = fx[f"post/{k}"]
        if k.endswith("num_batches_tracked"):
            assert int(b) == int(ref) == (4 if train else 3)
        else:
            assert close(b, ref, 1e-3), (k, diff_report(b, ref, 1e-3))
            if not train:
                assert torch.equal(b.cpu(), fx[f"sd/{k}"])


@pytest.mark.parametrize("case", PARITY, ids=lambda c: c.id)
def test_parity_float64(enc_mod, case):
    sd, x, gout, r64, r32 = refs(case)
    check_preconditions(case, r64, r32)
    got = run_device(enc_mod, case, sd, x, gout)
    check_parity(case, got, r64, r32)
    if not case.train:      # eval leaves the buffers alone
        for k, v in sd.items():
            if "running" in k or "num_batches" in k:
                assert torch.equal(got[f"buf/{k}"], v), k


@pytest.mark.parametrize("case", BUFFERS, ids=lambda c: c.id)
def test_train_mode_buffers(enc_mod, case):
    """running_mean / running_var (momentum, unbiased variance; momentum=None: cumulative average)
    and num_batches_tracked of both BatchNorms after one forward, against torch."""
    sd, x, gout, r64, r32 = refs(case)
    check_preconditions(case, r64, r32)
    got = run_device(enc_mod, case, sd, x, gout)
    check_buffers(case, got, r64)
    assert int(got["buf/conv_net.1.num_batches_tracked"]) == 4
    assert not torch.equal(got["buf/conv_net.4.running_var"], sd["conv_net.4.running_var"])


def test_training_needs_more_than_one_value(enc_mod):
    e = enc_mod.ConvSequenceEncoder(8, 32, OUT_DIM).cuda().train()
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        e(torch.randn(1, 1, 8, device="cuda"))
    assert e.eval()(torch.randn(1, 1, 8, device="cuda")).shape == (1, OUT_DIM)


def test_no_input_gradient(enc_mod):
    """An input that does not require grad: the parameter gradients are the same bits, and the
    backward operator writes nothing for dX (an empty tensor)."""
    case = Case(3, 37, 17, 64)
    sd, x, gout, _, _ = refs(case)
    a = run_device(enc_mod, case, sd, x, gout, need_dx=True)
    b = run_device(enc_mod, case, sd, x, gout, need_dx=False)
    assert b["dx"] is None
    for k in a:
        if k.startswith("grad/"):
            assert torch.equal(a[k], b[k]), k
    H = case.hidden
    xd = x.cuda()
    w1, w2 = torch.randn(H, 3, case.cin, device="cuda"), torch.randn(H, 3, H, device="cuda")
    v = [torch.rand(H, device="cuda") + 0.5 for _ in range(10)]
    pooled, y1, y2, s1, s2 = torch.ops.mmfusion.conv_encoder_fwd(xd, w1, v[0], v[1], v[2], v[3], v[4], w2, v[5], v[6],
                                                                 v[7], v[8], v[9], True, 1e-5, 1e-5)
    g = torch.ops.mmfusion.conv_encoder_bwd(xd, w1, w2, y1, y2, s1, s2, torch.ones_like(pooled), True, False)
    assert g[0].numel() == 0 and g[1].shape == w1.shape


def test_bit_identical_reruns(enc_mod):
    case = Case(2, 70, 128, 64)
    sd, x, gout, _, _ = refs(case)
    a = run_device(enc_mod, case, sd, x, gout)
    b = run_device(enc_mod, case, sd, x, gout)
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_module_path_cooking_model(enc_mod):
    """from_config with video FrameEncoder + audio ConvSequenceEncoder at B = 4: forward -> CE ->
    backward runs, and the logits match the same model with the audio conv stack evaluated by
    float64 torch on the CPU."""
    from harness import MultimodalFusionModel
    cfg = {"dataset": {"modalities": ["video", "audio"], "num_classes": 7},
           "model": {"output_dim": 32, "hidden_dim": 32, "num_heads": 4, "dropout": 0.0, "fusion_type": "hybrid",
                     "layer_norm": True,
                     "encoders": {"video": {"type": "frame", "input_dim": 48, "hidden_dim": 32, "dropout": 0.0},
                                  "audio": {"type": "sequence", "encoder_type": "cnn", "input_dim": 128,
                                            "hidden_dim": 64, "dropout": 0.0}}}}
    torch.manual_seed(3)
    m = MultimodalFusionModel.from_config(cfg).cuda().eval()
    audio = m.encoders["audio"]
    assert type(audio) is enc_mod.ConvSequenceEncoder
    with torch.no_grad():
        for i in (1, 4):
            audio.conv_net[i].running_mean.normal_(0.0, 0.5)
            audio.conv_net[i].running_var.uniform_(0.5, 1.5)
    B = 4
    feats = {"video": torch.randn(B, 6, 48, device="cuda"), "audio": torch.randn(B, 21, 128, device="cuda")}
    labels = torch.tensor([0, 3, 6, 2], device="cuda")
    logits = m(feats)
    torch.nn.functional.cross_entropy(logits, labels).backward()
    torch.cuda.synchronize()
    assert logits.shape == (B, 7) and bool(torch.isfinite(logits).all())
    for k, p in m.named_parameters():
        if k.startswith("encoders.audio."):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, k
    # the audio encoding from float64 torch on the CPU, the rest of the model as it is
    conv64 = torch.nn.Sequential(
        torch.nn.Conv1d(128, 64, 3, padding=1), torch.nn.BatchNorm1d(64), torch.nn.ReLU(),
        torch.nn.Conv1d(64, 64, 3, padding=1), torch.nn.BatchNorm1d(64), torch.nn.ReLU()).double().eval()
    conv64.load_state_dict({k: v.detach().cpu().double() for k, v in audio.conv_net.state_dict().items()})
    with torch.no_grad():
        pooled = conv64(feats["audio"].cpu().double().transpose(1, 2)).mean(dim=2).float().cuda()
        enc = {"video": m.encoders["video"](feats["video"]), "audio": audio.projection(pooled)}
        ref = m.fusion_model({k: m.layer_norms[k](v) for k, v in enc.items()}, None)
    assert close(logits.detach(), ref, 1e-3), diff_report(logits.detach(), ref, 1e-3)


def test_compile_fullgraph_matches_eager(enc_mod):
    """torch.compile(encoder, fullgraph=True): no graph break from the new operators; forward,
    gradients and the running statistics equal eager's."""
    case = Case(3, 37, 17, 64)
    sd, x, gout, _, _ = refs(case)
    res = []
    for compiled in (False, True):
        e = enc_mod.ConvSequenceEncoder(case.cin, case.hidden, OUT_DIM, dropout=0.0)
        e.load_state_dict(sd)
        e = e.cuda().train()
        f = torch.compile(e, backend="inductor", fullgraph=True) if compiled else e
        xin = x.cuda().requires_grad_(True)
        out = f(xin)
        (out * gout.cuda()).sum().backward()
        torch.cuda.synchronize()
        res.append((out.detach(), xin.grad, {k: p.grad for k, p in e.named_parameters()},
                    {k: b.detach().clone() for k, b in e.named_buffers()}))
    (o0, dx0, g0, b0), (o1, dx1, g1, b1) = res
    assert close(o1, o0, 1e-6) and close(dx1, dx0, 1e-6)
    scale = max(float(v.abs().max()) for v in g0.values())
    for k in g0:
        # (the conv bias gradients are rounding noise around zero: a last-bit change upstream redraws it)
        atol = 2 * zero_grad_bound(g0[k], scale, ZERO_GRAD_C) if k in BIAS_KEYS else 0.0
        assert close(g1[k], g0[k], 1e-6, atol=atol), (k, diff_report(g1[k], g0[k], 1e-6, atol))
    for k in b0:
        assert close(b1[k], b0[k], 1e-6), k
    assert int(b1["conv_net.1.num_batches_tracked"]) == 4
