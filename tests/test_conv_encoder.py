"""ConvSequenceEncoder / build_encoder without a GPU: the public surface against the reference's
'cnn' SequenceEncoder (src/encoders.py:87-97, 168-175, 400-451), the C-ABI's host-side validation
and the operators' fake kernels.  The numbers are covered by test_gpu_conv_encoder.py."""
import ctypes

import pytest
import torch
import torch.nn as nn
from torch._subclasses.fake_tensor import FakeTensorMode

KEYS = (["conv_net.0.weight", "conv_net.0.bias"]
        + [f"conv_net.1.{n}" for n in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
        + ["conv_net.3.weight", "conv_net.3.bias"]
        + [f"conv_net.4.{n}" for n in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")]
        + ["projection.weight", "projection.bias"])


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


def test_surface(enc_mod):
    e = enc_mod.ConvSequenceEncoder(17, 64, 16, num_layers=5, dropout=0.25)
    assert (e.encoder_type, e.hidden_dim, e.output_dim) == ("cnn", 64, 16)
    assert e.rnn is None and e.input_projection is None and e.transformer is None
    assert isinstance(e.dropout_layer, nn.Dropout) and e.dropout_layer.p == 0.25
    kinds = (nn.Conv1d, nn.BatchNorm1d, nn.ReLU, nn.Conv1d, nn.BatchNorm1d, nn.ReLU)
    assert isinstance(e.conv_net, nn.Sequential) and len(e.conv_net) == 6
    assert all(type(m) is k for m, k in zip(e.conv_net, kinds))
    assert (e.conv_net[0].in_channels, e.conv_net[0].out_channels, e.conv_net[3].in_channels) == (17, 64, 64)
    assert isinstance(e.pool, nn.AdaptiveAvgPool1d)
    assert isinstance(e.projection, nn.Linear) and e.projection.weight.shape == (16, 64)
    assert list(e.state_dict()) == KEYS
    d = enc_mod.ConvSequenceEncoder(8)
    assert (d.hidden_dim, d.output_dim, d.dropout_layer.p) == (256, 128, 0.1)


def test_same_seed_same_weights_as_torch_modules_in_reference_order(enc_mod):
    torch.manual_seed(5)
    e = enc_mod.ConvSequenceEncoder(17, 64, 16)
    torch.manual_seed(5)
    nn.Dropout(0.1)
    ref = {"conv_net.0": nn.Conv1d(17, 64, kernel_size=3, padding=1), "conv_net.1": nn.BatchNorm1d(64),
           "conv_net.3": nn.Conv1d(64, 64, kernel_size=3, padding=1), "conv_net.4": nn.BatchNorm1d(64),
           "projection": nn.Linear(64, 16)}
    sd = e.state_dict()
    for prefix, mod in ref.items():
        for k, v in mod.state_dict().items():
            assert torch.equal(sd[f"{prefix}.{k}"], v), f"{prefix}.{k}"


def test_errors(enc_mod):
    e = enc_mod.ConvSequenceEncoder(8, 32, 16)
    with pytest.raises(ValueError, match="Expected 3D input sequence, got shape"):
        e(torch.randn(4, 8))
    with pytest.raises(RuntimeError, match="ROCm device"):
        e(torch.randn(2, 5, 8))                      # a CPU tensor: the package's device error
    e.pool = None
    with pytest.raises(RuntimeError, match="CNN modules not initialized."):
        e(torch.randn(2, 5, 8))
    e = enc_mod.ConvSequenceEncoder(8, 32, 16)
    e.conv_net = None
    with pytest.raises(RuntimeError, match="CNN modules not initialized."):
        e(torch.randn(2, 5, 8))
    e = enc_mod.ConvSequenceEncoder(8, 32, 16)
    e.conv_net = nn.Sequential(*[nn.Identity() for _ in range(6)])
    with pytest.raises(NotImplementedError):        # no torch fallback
        e(torch.randn(2, 5, 8))


def test_sequence_encoder_cnn_still_not_implemented(enc_mod):
    with pytest.raises(NotImplementedError, match="ConvSequenceEncoder") as ei:
        enc_mod.SequenceEncoder(8, encoder_type="cnn")
    assert "build_encoder" in str(ei.value)


def test_build_encoder_dispatch(enc_mod):
    a = enc_mod.build_encoder("audio", 128, 64, {"type": "sequence", "encoder_type": "cnn", "hidden_dim": 32})
    assert type(a) is enc_mod.ConvSequenceEncoder and (a.hidden_dim, a.output_dim) == (32, 64)
    assert a.conv_net[0].in_channels == 128
    assert type(enc_mod.build_encoder("audio", 8, 16, {"encoder_type": "cnn", "hidden_dim": 32})) \
        is enc_mod.ConvSequenceEncoder
    s = enc_mod.build_encoder("imu_hand", 9, 16, {"encoder_type": "lstm", "hidden_dim": 64, "num_layers": 1})
    assert type(s) is enc_mod.SequenceEncoder and s.rnn.input_size == 9
    assert type(enc_mod.build_encoder("mocap", 9, 16, {"hidden_dim": 64})) is enc_mod.SequenceEncoder
    v = enc_mod.build_encoder("video", 48, 16, {"hidden_dim": 32})
    assert type(v) is enc_mod.FrameEncoder
    assert type(enc_mod.build_encoder("whatever", 48, 16, {"type": "frame", "hidden_dim": 32})) is enc_mod.FrameEncoder
    with pytest.raises(NotImplementedError, match="is not on the MI355X path"):
        enc_mod.build_encoder("audio", 8, 16, {"type": "mlp"})
    with pytest.raises(NotImplementedError, match=r"encoder for modality 'mystery' \(mlp\)"):
        enc_mod.build_encoder("mystery", 8, 16)
    cfg = {"type": "sequence", "encoder_type": "cnn"}
    enc_mod.build_encoder("audio", 8, 16, cfg)
    assert cfg == {"type": "sequence", "encoder_type": "cnn"}     # the caller's dict is not consumed


def test_from_config_builds_the_cooking_model(enc_mod):
    from harness import MultimodalFusionModel
    cfg = {"dataset": {"modalities": ["video", "audio"], "num_classes": 7},
           "model": {"output_dim": 32, "hidden_dim": 32, "num_heads": 4, "dropout": 0.1, "fusion_type": "hybrid",
                     "layer_norm": True,
                     "encoders": {"video": {"type": "frame", "input_dim": 1024, "hidden_dim": 64},
                                  "audio": {"type": "sequence", "encoder_type": "cnn", "input_dim": 128,
                                            "hidden_dim": 64}}}}
    m = MultimodalFusionModel.from_config(cfg)
    assert type(m.encoders["video"]) is enc_mod.FrameEncoder
    assert type(m.encoders["audio"]) is enc_mod.ConvSequenceEncoder
    assert m.encoders["audio"].conv_net[0].in_channels == 128
    keys = set(m.state_dict())
    assert "encoders.audio.conv_net.4.running_var" in keys and "encoders.video.attention.weight" in keys


def test_conv_encoder_limits_cpu(nat):
    """Host-side validation (include/mmfusion.h): shapes outside the limits are refused before
    anything touches the device (null device pointers here)."""
    L = nat.lib()
    assert L.mmf_conv_encoder_workspace_bytes(3, 37, 17, 64, 0) > 0
    assert L.mmf_conv_encoder_workspace_bytes(3, 37, 17, 64, 1) > L.mmf_conv_encoder_workspace_bytes(3, 37, 17, 64, 0)
    assert L.mmf_conv_encoder_workspace_bytes(256, 128, 128, 256, 1) > 2 * 4 * 256 * 128 * 256

    def fwd(B, T, cin, H):
        return L.mmf_conv_encoder_forward(B, T, cin, H, 1, *([None] * 7), 1e-5, *([None] * 6), 1e-5, *([None] * 7))

    def bwd(B, T, cin, H):
        return L.mmf_conv_encoder_backward(B, T, cin, H, 1, *([None] * 19))

    ELIMIT, EINVAL = 2, 1
    for call in (fwd, bwd):
        assert call(3, 37, 17, 48) == ELIMIT and b"multiple of 32" in L.mmf_last_error()     # hidden % 32
        assert call(3, 37, 17, 544) == ELIMIT                                                   # hidden > 512
        assert call(3, 37, 5000, 64) == ELIMIT and b"in_dim" in L.mmf_last_error()
        assert call(1 << 14, 1 << 11, 17, 64) == ELIMIT and b"batch * steps" in L.mmf_last_error()
        assert call(0, 37, 17, 64) == EINVAL and b"batch * steps == 0" in L.mmf_last_error()
        assert call(3, 0, 17, 64) == EINVAL
        assert call(3, 37, 0, 64) == EINVAL
        assert call(-1, 37, 17, 64) == EINVAL
        assert call(3, 37, 17, 64) == EINVAL and b"null buffer" in L.mmf_last_error()          # in limits, no buffers
    for bad in ((3, 37, 17, 48), (0, 37, 17, 64), (3, 37, 5000, 64)):
        assert L.mmf_conv_encoder_workspace_bytes(*bad, 1) == 0


def test_conv_encoder_fake_shapes(enc_mod):
    B, T, cin, H = 3, 20, 17, 64
    with FakeTensorMode(), torch.device("cuda"):
        e = enc_mod.ConvSequenceEncoder(cin, H, 32, dropout=0.0)
        out = e(torch.randn(B, T, cin))
        assert out.shape == (B, 32) and out.device.type == "cuda" and out.dtype == torch.float32
        x = torch.randn(B, T, cin)
        w1, w2 = torch.randn(H, 3, cin), torch.randn(H, 3, H)
        v = [torch.randn(H) for _ in range(10)]
        pooled, y1, y2, s1, s2 = torch.ops.mmfusion.conv_encoder_fwd(x, w1, v[0], v[1], v[2], v[3], v[4], w2, v[5],
                                                                     v[6], v[7], v[8], v[9], True, 1e-5, 1e-5)
        assert pooled.shape == (B, H) and y1.shape == y2.shape == (B, T, H) and s1.shape == s2.shape == (6, H)
        for need_dx in (True, False):
            g = torch.ops.mmfusion.conv_encoder_bwd(x, w1, w2, y1, y2, s1, s2, pooled, True, need_dx)
            assert len(g) == 9
            assert g[0].shape == (x.shape if need_dx else (0,))
            assert g[1].shape == w1.shape and g[5].shape == w2.shape
            assert all(g[i].shape == (H,) for i in (2, 3, 4, 6, 7, 8))
