"""TransformerSequenceEncoder / build_encoder without a GPU: the public surface against the reference's
'transformer' SequenceEncoder (src/encoders.py:99-111, 177-206, 400-451) and its recorded fixtures, the
C-ABI's host-side validation, the operators' fake kernels, and the formula oracle (tests/_transenc.py)
against float64 nn.TransformerEncoder.  The numbers are covered by test_gpu_transformer_encoder.py."""
import ctypes

import pytest
import torch
import torch.nn as nn
from torch._subclasses.fake_tensor import FakeTensorMode

import _transenc as tr
from _util import close, diff_report, load_fixture


@pytest.fixture(scope="module")
def enc_mod(pkg_on_path):
    import encoders
    return encoders


@pytest.fixture(scope="module")
def nat(pkg_on_path):
    import mmf_native
    try:
        mmf_native.lib()
    except RuntimeError as e:
        pytest.fail(f"libmmfusion.so not built: {e}")
    return mmf_native


def _fixture_sd(name):
    fx = load_fixture(name)
    return {k[3:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("sd/")}


def test_state_dict_keys_and_order_match_the_reference(enc_mod):
    sd = _fixture_sd("transenc_train")
    e = enc_mod.TransformerSequenceEncoder(17, 16, 16, num_layers=1, dropout=0.0)
    assert list(e.state_dict()) == list(sd)
    e.load_state_dict(sd, strict=True)
    assert list(e.state_dict())[:2] == ["projection.weight", "projection.bias"]   # Identity registered first
    assert "transformer.layers.0.self_attn.in_proj_weight" in sd and "_rng_state" not in e.state_dict()


def test_same_seed_same_weights_as_torch_modules_in_reference_order(enc_mod):
    torch.manual_seed(5)
    e = enc_mod.TransformerSequenceEncoder(17, 32, 16, num_layers=2, dropout=0.2)
    torch.manual_seed(5)
    nn.Dropout(0.2)
    ref = {"input_projection": nn.Linear(17, 32)}
    layer = nn.TransformerEncoderLayer(d_model=32, nhead=4, dropout=0.2, batch_first=True)
    ref["transformer"] = nn.TransformerEncoder(layer, num_layers=2)
    ref["projection"] = nn.Linear(32, 16)
    sd = e.state_dict()
    n = 0
    for prefix, mod in ref.items():
        for k, v in mod.state_dict().items():
            assert torch.equal(sd[f"{prefix}.{k}"], v), f"{prefix}.{k}"
            n += 1
    assert n == len(sd)


def test_surface(enc_mod):
    e = enc_mod.TransformerSequenceEncoder(17, 32, 16, num_layers=3, dropout=0.25)
    assert (e.encoder_type, e.hidden_dim, e.output_dim) == ("transformer", 32, 16)
    assert e.rnn is None and e.conv_net is None and e.pool is None
    assert isinstance(e.dropout_layer, nn.Dropout) and e.dropout_layer.p == 0.25
    assert isinstance(e.input_projection, nn.Linear) and e.input_projection.weight.shape == (32, 17)
    assert isinstance(e.transformer, nn.TransformerEncoder) and len(e.transformer.layers) == 3
    lyr = e.transformer.layers[0]
    assert lyr.self_attn.num_heads == 4 and lyr.linear1.out_features == 2048 and lyr.dropout.p == 0.25
    assert isinstance(e.projection, nn.Linear) and e.projection.weight.shape == (16, 32)
    layers, p, eps = e._stack()
    assert len(layers) == 3 and p == 0.25 and eps == 1e-5
    d = enc_mod.TransformerSequenceEncoder(8)
    assert (d.hidden_dim, d.output_dim, d.dropout_layer.p, len(d.transformer.layers)) == (256, 128, 0.1, 2)
    assert enc_mod.recurrence_kind(d) is None


def test_errors(enc_mod):
    e = enc_mod.TransformerSequenceEncoder(8, 16, 16, num_layers=1)
    with pytest.raises(ValueError, match="Expected 3D input sequence, got shape"):
        e(torch.randn(4, 8))
    with pytest.raises(RuntimeError, match="ROCm device"):
        e(torch.randn(2, 5, 8))                      # a CPU tensor: the package's device error
    e.transformer = None
    with pytest.raises(RuntimeError, match="Transformer modules not initialized."):
        e(torch.randn(2, 5, 8))
    e = enc_mod.TransformerSequenceEncoder(8, 16, 16, num_layers=1)
    e.input_projection = None
    with pytest.raises(RuntimeError, match="Transformer modules not initialized."):
        e(torch.randn(2, 5, 8))


def _swapped(enc_mod, final_norm=None, **layer_kw):
    e = enc_mod.TransformerSequenceEncoder(8, 16, 16, num_layers=2)
    layer = nn.TransformerEncoderLayer(d_model=16, nhead=layer_kw.pop("nhead", 4), batch_first=True, **layer_kw)
    e.transformer = nn.TransformerEncoder(layer, num_layers=2, norm=final_norm)
    return e


def test_stack_refuses_what_the_kernels_do_not_implement(enc_mod):
    assert len(_swapped(enc_mod, dim_feedforward=24)._stack()[0]) == 2        # any dim_feedforward is fine
    for bad in (_swapped(enc_mod, norm_first=True), _swapped(enc_mod, activation="gelu"),
                _swapped(enc_mod, final_norm=nn.LayerNorm(16)), _swapped(enc_mod, nhead=2),
                _swapped(enc_mod, bias=False)):
        with pytest.raises(NotImplementedError, match="no torch fallback"):
            bad._stack()
        with pytest.raises(NotImplementedError):      # ... and forward refuses before touching the device
            bad(torch.randn(2, 5, 8))
    e = _swapped(enc_mod)
    e.transformer.layers[1].dropout1.p = 0.5          # dropout p differs inside the stack
    with pytest.raises(NotImplementedError):
        e._stack()
    e = _swapped(enc_mod)
    e.transformer.layers[1].norm2.eps = 1e-3
    with pytest.raises(NotImplementedError):
        e._stack()


def test_sequence_encoder_transformer_still_not_implemented(enc_mod):
    with pytest.raises(NotImplementedError) as ei:
        enc_mod.SequenceEncoder(8, encoder_type="transformer")
    msg = str(ei.value)
    assert "not on the MI355X path" in msg and "gru" not in msg.lower() and "TransformerSequenceEncoder" in msg


def test_build_encoder_dispatch(enc_mod):
    a = enc_mod.build_encoder("imu", 9, 64, {"type": "sequence", "encoder_type": "transformer", "hidden_dim": 32,
                                             "num_layers": 1})
    assert type(a) is enc_mod.TransformerSequenceEncoder and (a.hidden_dim, a.output_dim) == (32, 64)
    assert a.input_projection.in_features == 9 and len(a.transformer.layers) == 1
    cfg = {"encoder_type": "transformer", "hidden_dim": 16}
    assert type(enc_mod.build_encoder("audio", 8, 16, cfg)) is enc_mod.TransformerSequenceEncoder
    assert cfg == {"encoder_type": "transformer", "hidden_dim": 16}      # the caller's dict is not consumed
    assert type(enc_mod.build_encoder("audio", 8, 16, {"encoder_type": "gru", "hidden_dim": 16})) \
        is enc_mod.GRUSequenceEncoder


def test_from_config_builds_a_transformer_encoder(enc_mod):
    from harness import MultimodalFusionModel
    cfg = {"dataset": {"modalities": ["video", "imu"], "num_classes": 7},
           "model": {"output_dim": 32, "hidden_dim": 32, "num_heads": 4, "dropout": 0.1, "fusion_type": "hybrid",
                     "encoders": {"video": {"type": "frame", "input_dim": 48, "hidden_dim": 32},
                                  "imu": {"type": "sequence", "encoder_type": "transformer", "input_dim": 9,
                                          "hidden_dim": 32, "num_layers": 1}}}}
    m = MultimodalFusionModel.from_config(cfg)
    assert type(m.encoders["imu"]) is enc_mod.TransformerSequenceEncoder
    assert "encoders.imu.transformer.layers.0.norm2.bias" in set(m.state_dict())


def _desc(nat, B=3, T=37, H=16, F=2048, NL=1, training=1, dropout=0.0, eps=1e-5):
    return nat.TransformerDesc(B, T, H, F, NL, training, dropout, eps)


def test_limits_cpu(nat):
    """Host-side validation (include/mmfusion.h): shapes outside the limits are refused before anything
    touches the device (null device pointers here)."""
    L = nat.lib()

    def fwd(**kw):
        d = _desc(nat, **kw)
        return L.mmf_transformer_encoder_forward(ctypes.byref(d), *([None] * 8))

    def bwd(**kw):
        d = _desc(nat, **kw)
        return L.mmf_transformer_encoder_backward(ctypes.byref(d), *([None] * 9))

    ELIMIT, EINVAL = 2, 1
    for call in (fwd, bwd):
        for H in (6, 260, 320):
            assert call(H=H) == ELIMIT and b"hidden" in L.mmf_last_error()
        for F in (0, 8193):
            assert call(F=F) == ELIMIT and b"ffn" in L.mmf_last_error()
        for NL in (0, 9):
            assert call(NL=NL) == ELIMIT and b"layers" in L.mmf_last_error()
        assert call(T=0) == ELIMIT and b"empty" in L.mmf_last_error()
        assert call(B=0) == ELIMIT
        assert call(B=1 << 14, T=1 << 11) == ELIMIT and b"batch * steps" in L.mmf_last_error()
        assert call(dropout=1.0) == EINVAL and b"dropout" in L.mmf_last_error()
        assert call(dropout=-0.1) == EINVAL
        assert call() == EINVAL and b"null buffer" in L.mmf_last_error()        # in limits, no buffers
        assert call(H=256, F=8192, NL=8) == EINVAL and b"null buffer" in L.mmf_last_error()
    for bad in ((3, 37, 6, 2048, 1), (3, 37, 260, 2048, 1), (3, 37, 16, 0, 1), (3, 37, 16, 2048, 9), (3, 0, 16, 2048, 1)):
        assert L.mmf_transformer_encoder_saved_bytes(*bad) == 0
        assert L.mmf_transformer_encoder_workspace_bytes(*bad, 0) == 0
        assert L.mmf_transformer_encoder_workspace_bytes(*bad, 1) == 0


def test_size_queries_grow(nat):
    L = nat.lib()
    saved, ws = L.mmf_transformer_encoder_saved_bytes, L.mmf_transformer_encoder_workspace_bytes
    base = saved(3, 37, 16, 2048, 1)
    assert base > 4 * 3 * 37 * (2048 + 8 * 16)                    # the activations one layer keeps
    assert saved(3, 74, 16, 2048, 1) > base and saved(3, 37, 16, 2048, 2) > 1.9 * base
    assert 0 < ws(3, 37, 16, 2048, 1, 0) < ws(3, 37, 16, 2048, 1, 1)
    assert ws(3, 74, 16, 2048, 1, 0) > ws(3, 37, 16, 2048, 1, 0)
    assert ws(3, 74, 16, 2048, 1, 1) > ws(3, 37, 16, 2048, 1, 1)
    # the workspace holds one layer's scratch, reused by every layer
    assert ws(3, 37, 16, 2048, 2, 1) == ws(3, 37, 16, 2048, 1, 1)
    assert ws(256, 128, 256, 2048, 2, 1) > 4 * 256 * 128 * (2048 + 11 * 256)


def test_fake_shapes(enc_mod):
    B, T, cin, H, F = 3, 20, 17, 32, 24
    # (built outside the mode: nn.TransformerEncoder deep-copies its layer, which fake parameters do not
    # survive; the module then runs on fake copies of its parameters and buffers)
    e = enc_mod.TransformerSequenceEncoder(cin, H, 8, num_layers=2, dropout=0.0)
    with FakeTensorMode(), torch.device("cuda"):
        fake = {k: torch.empty(v.shape, dtype=v.dtype) for k, v in list(e.named_parameters()) + list(e.named_buffers())}
        out = torch.func.functional_call(e, fake, (torch.randn(B, T, cin), torch.tensor([20, 3, 1])))
        assert out.shape == (B, 8) and out.device.type == "cuda" and out.dtype == torch.float32
        x = torch.randn(B, T, H)
        lengths = torch.tensor([20, 3, 1])
        rng = torch.zeros(2, dtype=torch.int64)
        shapes = [(3 * H, H), (3 * H,), (H, H), (H,), (F, H), (F,), (H, F), (H,), (H,), (H,), (H,), (H,)]
        params = [torch.randn(s) for _ in range(2) for s in shapes]
        pooled, saved, rng_next = torch.ops.mmfusion.transformer_encoder_fwd(x, lengths, rng, params, True, 0.1, 1e-5)
        assert pooled.shape == (B, H) and pooled.dtype == torch.float32
        assert saved.dtype == torch.uint8 and saved.dim() == 1 and saved.numel() > 4 * 2 * B * T * (F + 8 * H)
        assert rng_next.shape == (2,) and rng_next.dtype == torch.int64
        for lens in (lengths, None):
            for need_dx in (True, False):
                g = torch.ops.mmfusion.transformer_encoder_bwd(x, lens, params, saved, pooled, True, 0.1, 1e-5, need_dx)
                assert len(g) == 1 + len(params)
                assert g[0].shape == (x.shape if need_dx else (0,))
                assert all(a.shape == p.shape and a.dtype == torch.float32 for a, p in zip(g[1:], params))


ORACLE_CASES = [tr.Case(3, 11, 7, 16, ffn=24, layers=2, lengths=(11, 6, 1), seed=1),
                tr.Case(2, 9, 5, 20, ffn=30, layers=1, lengths=None, seed=2),
                tr.Case(2, 6, 5, 8, ffn=12, layers=1, lengths=(6, 4), seed=3, train=False)]


@pytest.mark.parametrize("case", ORACLE_CASES, ids=lambda c: c.id)
def test_formula_oracle_matches_float64_torch(case):
    """tests/_transenc.stack_forward against the real nn.TransformerEncoder in float64: out, dx and every
    parameter gradient at 1e-12, with and without lengths."""
    sd, x, lengths, gout = tr.make_case(case)
    ref = tr.run_torch(case, sd, x, lengths, gout, torch.float64)
    got = tr.run_oracle(case, sd, x, lengths, gout, torch.float64)
    keys = tr.compared_keys(ref)
    assert len(keys) == 2 + 4 + 12 * case.layers
    for k in keys:
        assert close(got[k], ref[k], 1e-12), (case.id, k, diff_report(got[k], ref[k], 1e-12))


@pytest.mark.parametrize("name", ["transenc_train", "transenc_eval"])
def test_formula_oracle_matches_the_reference_fixture(name):
    """... and against what the reference itself recorded (float32): within fp32 rounding of it."""
    fx = load_fixture(name)
    sd = _fixture_sd(name)
    case = tr.Case(3, 37, 17, 16, lengths=(37, 20, 1), train=name.endswith("train"))
    got = tr.run_oracle(case, sd, torch.from_numpy(fx["x"]), torch.from_numpy(fx["lengths"]),
                        torch.from_numpy(fx["gout"]), torch.float64)
    for k in ["out", "dx"] + [k for k in fx if k.startswith("grad/")]:
        assert close(fx[k], got[k], 1e-4), (name, k, diff_report(fx[k], got[k], 1e-4))


def test_oracle_length_zero_sample_is_zero():
    """A sample of length 0: pooled = 0 (the output is the projection's bias) and zero input gradient,
    where torch's softmax over no key gives NaN."""
    case = tr.Case(2, 5, 4, 8, ffn=12, lengths=(5, 0), seed=4)
    sd, x, lengths, gout = tr.make_case(case)
    got = tr.run_oracle(case, sd, x, lengths, gout, torch.float64)
    assert all(bool(torch.isfinite(got[k]).all()) for k in tr.compared_keys(got))
    assert torch.equal(got["out"][1], sd["projection.bias"].double())
    assert float(got["dx"][1].abs().max()) == 0.0 and float(got["dx"][0].abs().max()) > 0.0
