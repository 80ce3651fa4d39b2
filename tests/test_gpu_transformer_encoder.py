"""TransformerSequenceEncoder on the GPU (csrc/transformer.hip) against the reference's recorded results
(tests/golden/transenc_*.npz, gen_transenc.py) and against the formula oracle of tests/_transenc.py in
float64 on the CPU (which test_transformer_encoder.py ties to float64 nn.TransformerEncoder at 1e-12),
at the project's fp32 parity bound close(got, ref, 1e-3).

Every parity case fixes a seed and asserts, before looking at the device, that it is well posed
(_transenc.check_preconditions): no linear1 pre-activation of a valid token within 1e-6 (|y1| |W1|^T +
|b1|) of the ReLU kink in float64, and fp32 nn.TransformerEncoder on the CPU within 1e-4 of float64 on
every compared tensor.

The LayerNorm kernels take 4 rows per workgroup forward and 32 backward (one dgamma / dbeta partial per
32 rows, reduced in groups of ~sqrt(chunks)); the attention takes 128 queries per workgroup and 64- or
128-key chunks; the weight-gradient splits are >= 32 rows: (2, 70, .) puts a row-chunk and a reduce-group
edge inside the second sample, (2, 130, .) needs two query blocks and several key chunks.
"""
import pytest
import torch

import _philox
from _transenc import (Case, build_device, check_parity, check_preconditions, compared_keys, make_case,
                       run_device, run_oracle, run_torch)
from _util import close, diff_report, load_fixture

pytestmark = pytest.mark.gpu

PARITY = [
    Case(3, 1, 17, 16, ffn=24),                                     # T = 1: softmax over one key
    Case(2, 70, 5, 64, ffn=40),                                     # n = 140: chunk edges inside a sample
    Case(2, 130, 8, 64, ffn=32, lengths=(130, 65)),                 # two attention query blocks, key chunks
    Case(2, 9, 8, 256, ffn=96),                                     # the widest row, head_dim 64
    Case(3, 5, 8, 20, ffn=30),                                      # head_dim 5, ffn % 4 != 0: the generic GEMM path
    Case(2, 12, 6, 16, ffn=24, layers=2),                           # two layers, lengths None
    Case(3, 10, 6, 16, ffn=24, layers=2, lengths=(10, 25, 4)),      # a length above T counts as T
    Case(3, 37, 17, 16, ffn=24, lengths=(37, 20, 1), train=False),  # eval mode
    # LayerNorm's variance at a large mean (make_case keeps the offset out of the attention scores, where
    # fp32 torch itself would sit 1e-4 .. 1e-3 from float64; as it is, 1.4e-5)
    Case(2, 9, 6, 32, ffn=24, bias_offset=100.0),
]
DROPOUT_CASE = Case(2, 37, 6, 32, ffn=40, layers=2, lengths=(37, 20), seed=5)
DROP_P, DROP_RNG = 0.3, (1234, 7)
_REFS = {}


@pytest.fixture(scope="module")
def enc_mod(pkg_on_path):
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible")
    import encoders
    return encoders


def refs(case: Case):
    """(state dict, x, lengths, gout, float64 oracle result, float32 torch result) of a case, computed once."""
    if case not in _REFS:
        sd, x, lengths, gout = make_case(case)
        _REFS[case] = (sd, x, lengths, gout, run_oracle(case, sd, x, lengths, gout, torch.float64),
                       run_torch(case, sd, x, lengths, gout, torch.float32))
    return _REFS[case]


@pytest.mark.parametrize("name", ["transenc_train", "transenc_eval"])
def test_reference_fixture(enc_mod, name):
    """The reference's own SequenceEncoder(17, 16, 16, num_layers=1, encoder_type='transformer') at
    (3, 37, 17) with lengths [37, 20, 1]: its state dict loads; output, dX and every parameter gradient
    match what it recorded, and the float64 oracle on the same inputs."""
    fx = {k: torch.from_numpy(v) for k, v in load_fixture(name).items()}
    sd = {k[3:]: v for k, v in fx.items() if k.startswith("sd/")}
    case = Case(3, 37, 17, 16, lengths=(37, 20, 1), train=name.endswith("train"))
    r64 = run_oracle(case, sd, fx["x"], fx["lengths"], fx["gout"], torch.float64)
    r32 = {k: fx[k] for k in compared_keys(r64)}      # fp32 torch: the reference's record itself
    check_preconditions(case, r64, r32)
    got = run_device(enc_mod, case, sd, fx["x"], fx["lengths"], fx["gout"])
    check_parity(case, got, r64)
    for k in compared_keys(r64):
        assert close(got[k], fx[k], 1e-3), (name, k, diff_report(got[k], fx[k], 1e-3))


@pytest.mark.parametrize("case", PARITY, ids=lambda c: c.id)
def test_parity_float64(enc_mod, case):
    sd, x, lengths, gout, r64, r32 = refs(case)
    check_preconditions(case, r64, r32)
    got = run_device(enc_mod, case, sd, x, lengths, gout)
    check_parity(case, got, r64)


def test_dropout_replayed_by_the_oracle(enc_mod):
    """Train mode with dropout 0.3: the oracle is fed the keep masks of the four sites per layer
    (attention probabilities, out_proj, linear1's activation, linear2) rebuilt from the module's Philox
    (seed, offset); the forward advances the offset by one."""
    case = DROPOUT_CASE
    sd, x, lengths, gout = make_case(case)
    r64 = run_oracle(case, sd, x, lengths, gout, torch.float64, p=DROP_P,
                     mask_fn=_philox.mask_provider(DROP_RNG[0], DROP_RNG[1], DROP_P))
    plain = run_oracle(case, sd, x, lengths, gout, torch.float64)
    assert not close(plain["out"], r64["out"], 1e-2)          # the masks do something
    check_preconditions(case, r64)
    got = run_device(enc_mod, case, sd, x, lengths, gout, dropout=DROP_P, rng=DROP_RNG)
    check_parity(case, got, r64)
    e = build_device(enc_mod, case, sd, DROP_P)
    e._rng_state.copy_(torch.tensor(DROP_RNG, dtype=torch.int64))
    e(x.cuda(), lengths.cuda())
    assert e._rng_state.tolist() == [DROP_RNG[0], DROP_RNG[1] + 1]
    e.eval()(x.cuda(), lengths.cuda())                        # eval draws nothing but still snapshots
    assert e._rng_state.tolist()[0] == DROP_RNG[0]


def test_exact_zeros(enc_mod):
    """dx at padded positions is exactly 0.0; a sample of length 0 gets the projection's bias as its
    output and exactly zero gradients (torch gives NaN there)."""
    case = Case(3, 9, 6, 16, ffn=24, layers=2, lengths=(9, 4, 0), seed=7)
    sd, x, lengths, gout = make_case(case)
    r64 = run_oracle(case, sd, x, lengths, gout, torch.float64)
    check_preconditions(case, r64)
    got = run_device(enc_mod, case, sd, x, lengths, gout)
    check_parity(case, got, r64)
    dx = got["dx"]
    assert float(dx[0].abs().min()) > 0.0
    assert float(dx[1, 4:].abs().max()) == 0.0 and float(dx[1, :4].abs().max()) > 0.0
    assert float(dx[2].abs().max()) == 0.0
    assert torch.equal(got["out"][2], sd["projection.bias"])
    # only samples of length 0: every gradient of the stack (and of both projections' weights) is 0.0
    case0 = Case(2, 5, 6, 16, ffn=24, lengths=(0, 0), seed=8)
    sd, x, lengths, gout = make_case(case0)
    got = run_device(enc_mod, case0, sd, x, lengths, gout)
    assert torch.equal(got["out"], sd["projection.bias"].expand(2, -1))
    for k in compared_keys(got):
        if k not in ("out", "grad/projection.bias"):
            assert float(got[k].abs().max()) == 0.0, k


def test_padding_invariance(enc_mod):
    """Padded inputs replaced by values of magnitude 1e3: output, valid dx and all parameter gradients
    are the same bits."""
    case = Case(3, 37, 17, 16, ffn=24, layers=2, lengths=(37, 20, 1), seed=9)
    sd, x, lengths, gout = make_case(case)
    pad = torch.arange(case.T).unsqueeze(0) >= lengths.unsqueeze(1)
    x2 = torch.where(pad.unsqueeze(-1), 1e3 * torch.randn(x.shape, generator=torch.Generator().manual_seed(1)), x)
    a = run_device(enc_mod, case, sd, x, lengths, gout)
    b = run_device(enc_mod, case, sd, x2, lengths, gout)
    assert float(b["dx"][pad].abs().max()) == 0.0
    for k in compared_keys(a):
        assert torch.equal(a[k], b[k]), (k, diff_report(b[k], a[k], 0.0))


def test_bit_identical_reruns(enc_mod):
    """Two runs of the same call (dropout on, the same Philox state) give the same bits."""
    case = DROPOUT_CASE
    sd, x, lengths, gout = make_case(case)
    a = run_device(enc_mod, case, sd, x, lengths, gout, dropout=DROP_P, rng=DROP_RNG)
    b = run_device(enc_mod, case, sd, x, lengths, gout, dropout=DROP_P, rng=DROP_RNG)
    c = run_device(enc_mod, case, sd, x, lengths, gout, dropout=DROP_P, rng=(DROP_RNG[0], DROP_RNG[1] + 1))
    for k in compared_keys(a):
        assert torch.equal(a[k], b[k]), k
    assert not torch.equal(a["out"], c["out"])                 # another offset, other masks
    case = PARITY[1]
    sd, x, lengths, gout, _, _ = refs(case)
    a = run_device(enc_mod, case, sd, x, lengths, gout)
    b = run_device(enc_mod, case, sd, x, lengths, gout)
    for k in compared_keys(a):
        assert torch.equal(a[k], b[k]), k


def test_eval_equals_train_at_dropout_zero(enc_mod):
    case = Case(3, 37, 17, 16, ffn=24, lengths=(37, 20, 1))
    sd, x, lengths, gout, _, _ = refs(case)
    a = run_device(enc_mod, case, sd, x, lengths, gout)
    b = run_device(enc_mod, Case(3, 37, 17, 16, ffn=24, lengths=(37, 20, 1), train=False), sd, x, lengths, gout)
    for k in compared_keys(a):
        assert torch.equal(a[k], b[k]), k


def test_no_input_gradient(enc_mod):
    """An input that does not require grad: the parameter gradients are the same bits."""
    case = PARITY[5]
    sd, x, lengths, gout, _, _ = refs(case)
    a = run_device(enc_mod, case, sd, x, lengths, gout, need_dx=True)
    b = run_device(enc_mod, case, sd, x, lengths, gout, need_dx=False)
    assert b["dx"] is None
    for k in a:
        if k.startswith("grad/") and not k.startswith("grad/input_projection"):
            assert torch.equal(a[k], b[k]), k


def test_module_path_from_config(enc_mod):
    """MultimodalFusionModel.from_config with a transformer IMU encoder: one forward -> CE -> backward
    runs, every encoder parameter gets a finite, nonzero gradient."""
    from harness import MultimodalFusionModel
    cfg = {"dataset": {"modalities": ["video", "imu"], "num_classes": 7},
           "model": {"output_dim": 32, "hidden_dim": 32, "num_heads": 4, "dropout": 0.1, "fusion_type": "hybrid",
                     "layer_norm": True,
                     "encoders": {"video": {"type": "frame", "input_dim": 48, "hidden_dim": 32},
                                  "imu": {"type": "sequence", "encoder_type": "transformer", "input_dim": 9,
                                          "hidden_dim": 32, "num_layers": 2}}}}
    torch.manual_seed(3)
    m = MultimodalFusionModel.from_config(cfg).cuda().train()
    assert type(m.encoders["imu"]) is enc_mod.TransformerSequenceEncoder
    B = 4
    feats = {"video": torch.randn(B, 6, 48, device="cuda"), "imu": torch.randn(B, 21, 9, device="cuda")}
    labels = torch.tensor([0, 3, 6, 2], device="cuda")
    logits = m(feats)
    torch.nn.functional.cross_entropy(logits, labels).backward()
    torch.cuda.synchronize()
    assert logits.shape == (B, 7) and bool(torch.isfinite(logits).all())
    for k, p in m.named_parameters():
        if k.startswith("encoders.imu."):
            assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, k
