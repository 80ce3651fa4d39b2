"""GRU sequence encoder without a GPU: the module surface against torch.nn.GRU and the
reference's fixtures (tests/golden/gen_gruenc.py), the factory, the C-ABI's host-side
validation, the operators' fake kernels, and the NumPy oracle (tests/_gru.py) itself against
float64 torch.nn.GRU."""
import numpy as np
import pytest
import torch

from _gru import gru_backward, gru_forward, gru_param_grads
from _util import load_fixture, rel_err


@pytest.fixture(scope="module")
def enc_mod(pkg_on_path):
    import encoders
    return encoders


@pytest.fixture(scope="module")
def nat(pkg_on_path):
    import mmf_native
    return mmf_native


def test_gru_module_matches_torch_layout(enc_mod):
    """encoders.GRU keeps nn.GRU's parameter names, shapes, order and initialisation (same seed ->
    same weights, state dicts interchangeable) without being an nn.RNNBase."""
    for layers, first in ((1, True), (2, True), (3, False)):
        torch.manual_seed(11)
        ref = torch.nn.GRU(9, 32, num_layers=layers, batch_first=first, dropout=0.2 if layers > 1 else 0.0)
        torch.manual_seed(11)
        mine = enc_mod.GRU(9, 32, num_layers=layers, batch_first=first, dropout=0.2 if layers > 1 else 0.0)
        assert not isinstance(mine, torch.nn.RNNBase)
        a, b = ref.state_dict(), mine.state_dict()
        assert list(a) == list(b)
        assert all(a[k].shape == b[k].shape and torch.equal(a[k], b[k]) for k in a)
        mine.load_state_dict(a)
        ref.load_state_dict(b)
        assert (mine.hidden_size, mine.num_layers, mine.batch_first) == (32, layers, first)
        assert mine.weight_ih_l0.shape == (96, 9) and mine.weight_hh_l0.shape == (96, 32)
    with pytest.raises(NotImplementedError):
        enc_mod.GRU(9, 32, bidirectional=True)
    with pytest.raises(NotImplementedError):
        enc_mod.GRU(9, 32, bias=False)


def test_gru_sequence_encoder_surface(enc_mod):
    e = enc_mod.GRUSequenceEncoder(17, 64, 16, num_layers=2)
    assert e.encoder_type == "gru" and e.hidden_dim == 64 and e.output_dim == 16
    assert e.conv_net is None and e.pool is None and e.input_projection is None and e.transformer is None
    assert isinstance(e.rnn, enc_mod.GRU) and e.rnn.dropout == 0.1 and e.rnn.batch_first
    assert sorted(e.state_dict()) == sorted(
        ["projection.weight", "projection.bias"]
        + [f"rnn.{p}_l{k}" for k in range(2) for p in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")])
    fx = load_fixture("gruenc_2layer_len")
    sd = {k[3:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("sd/")}
    e.load_state_dict(sd, strict=True)
    assert list(e.state_dict()) == list(sd)     # the reference's key order too
    assert torch.equal(e.rnn.weight_hh_l1, sd["rnn.weight_hh_l1"])
    assert hasattr(e, "encode_final_state")
    with pytest.raises(ValueError, match="Expected 3D input sequence"):
        e(torch.randn(4, 17))
    with pytest.raises(RuntimeError, match="ROCm device"):
        e(torch.randn(2, 5, 17))


def test_same_seed_same_weights_as_torch_construction(enc_mod):
    """Construction order: the GRU's parameters, then the projection (src/encoders.py:77-85)."""
    torch.manual_seed(5)
    e = enc_mod.GRUSequenceEncoder(8, 64, 16, num_layers=2, dropout=0.1)
    torch.manual_seed(5)
    rnn = torch.nn.GRU(8, 64, num_layers=2, batch_first=True, dropout=0.1)
    proj = torch.nn.Linear(64, 16)
    for k, v in rnn.state_dict().items():
        assert torch.equal(e.state_dict()[f"rnn.{k}"], v), k
    assert torch.equal(e.projection.weight, proj.weight) and torch.equal(e.projection.bias, proj.bias)


def test_factory_and_sequence_encoder_message(enc_mod):
    e = enc_mod.build_encoder("imu", 8, 16, {"encoder_type": "gru", "hidden_dim": 64})
    assert isinstance(e, enc_mod.GRUSequenceEncoder) and e.hidden_dim == 64 and e.output_dim == 16
    with pytest.raises(NotImplementedError, match="GRUSequenceEncoder"):
        enc_mod.SequenceEncoder(8, encoder_type="gru")
    with pytest.raises(NotImplementedError) as ei:
        enc_mod.SequenceEncoder(8, encoder_type="transformer")
    assert "gru" not in str(ei.value).lower() and "not on the MI355X path" in str(ei.value)


def test_gru_limits(nat):
    """Host-side validation returns MMF_ELIMIT before touching the device."""
    L = nat.lib()
    assert L.mmf_gru_sync_bytes(3, 256) == 2 * 4 * 3 * 256 * 8
    assert L.mmf_gru_sync_bytes(3, 256) == L.mmf_lstm_sync_bytes(3, 256)
    null = nat.ptr_array([0])
    # (8, 17, 4, 64): 8 x ceil(17 / 4) = 40 instances, over the 32 a launch holds
    for n, B, T, H in ((1, 1, 4, 96), (1, 1, 4, 320), (9, 1, 4, 64), (4, 33, 4, 64), (1, 0, 4, 64), (8, 17, 4, 64)):
        rc = L.mmf_gru_forward(n, B, T, H, null, null, null, null, null, null, None, None)
        assert rc == 2, (n, B, T, H)
        rc = L.mmf_gru_backward(n, B, T, H, null, null, null, null, null, null, None, None)
        assert rc == 2, (n, B, T, H)
    # a valid shape without a timeout word: MMF_EINVAL, still before the device
    assert L.mmf_gru_forward(1, 1, 4, 64, null, null, null, null, null, null, None, None) == 1
    assert L.mmf_gru_backward(1, 1, 4, 64, null, null, null, null, null, null, None, None) == 1
    # (8, 16, 4, 64) is 32 instances and passes the plan up to that same last check
    rc = L.mmf_gru_forward(8, 16, 4, 64, null, null, null, null, null, null, None, None)
    assert rc == 1 and b"timeout word" in L.mmf_last_error(), (rc, L.mmf_last_error())
    rc = L.mmf_gru_backward(8, 16, 4, 64, null, null, null, null, null, null, None, None)
    assert rc == 1 and b"timeout word" in L.mmf_last_error(), (rc, L.mmf_last_error())


def test_fake_kernels(enc_mod):
    """Shape propagation without a device: FakeTensorMode over fake cuda tensors."""
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode(), torch.device("cuda"):
        enc = enc_mod.GRUSequenceEncoder(12, 64, 16)
        out = enc(torch.randn(3, 9, 12))
        assert out.shape == (3, 16) and out.device.type == "cuda" and out.dtype == torch.float32
        xproj = [torch.empty(3, 9, 192) for _ in range(2)]
        w_hh = [torch.empty(192, 64) for _ in range(2)]
        b_hn = [torch.empty(64) for _ in range(2)]
        hs, gates, flag = torch.ops.mmfusion.gru_layer_fwd(xproj, w_hh, b_hn)
        assert [tuple(h.shape) for h in hs] == [(3, 9, 64)] * 2
        assert [tuple(g.shape) for g in gates] == [(3, 9, 256)] * 2
        assert tuple(flag.shape) == (1,) and flag.dtype == torch.int32
        dgates, flag = torch.ops.mmfusion.gru_layer_bwd(w_hh, hs, gates, [torch.empty_like(h) for h in hs])
        assert [tuple(g.shape) for g in dgates] == [(3, 9, 256)] * 2
        assert tuple(flag.shape) == (1,) and flag.dtype == torch.int32


def test_oracle_matches_float64_torch_gru():
    """tests/_gru.py (the formulas of csrc/gru.hip and of the autograd formula) against float64
    torch.nn.GRU: h, dx, dW_hh, db_hh, db_ih at 1e-12."""
    B, T, D, H = 3, 9, 5, 8
    torch.manual_seed(0)
    ref = torch.nn.GRU(D, H, batch_first=True).double()
    x = torch.randn(B, T, D, dtype=torch.float64, requires_grad=True)
    dh = torch.randn(B, T, H, dtype=torch.float64)
    out, _ = ref(x)
    (out * dh).sum().backward()
    w_ih, w_hh = ref.weight_ih_l0.detach().numpy(), ref.weight_hh_l0.detach().numpy()
    b_ih, b_hh = ref.bias_ih_l0.detach().numpy(), ref.bias_hh_l0.detach().numpy()
    fold = np.concatenate((b_hh[:2 * H], np.zeros(H)))
    xproj = x.detach().numpy() @ w_ih.T + b_ih + fold
    h, gates = gru_forward(xproj, w_hh, b_hh[2 * H:])
    dgates = gru_backward(w_hh, h, gates, dh.numpy())
    dxproj, dw_hh, db_hn = gru_param_grads(h, dgates)
    dx = dxproj @ w_ih
    db_ih = dxproj.reshape(-1, 3 * H).sum(0)
    db_hh = np.concatenate((db_ih[:2 * H], db_hn))
    tol = 1e-12
    assert rel_err(h, out.detach()) <= tol
    assert rel_err(dx, x.grad) <= tol
    assert rel_err(dw_hh, ref.weight_hh_l0.grad) <= tol
    assert rel_err(db_hh, ref.bias_hh_l0.grad) <= tol
    assert rel_err(db_ih, ref.bias_ih_l0.grad) <= tol
