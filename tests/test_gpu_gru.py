"""GRU sequence encoder on the persistent HIP recurrence (csrc/gru.hip): the raw C-ABI recurrence
against the NumPy float64 oracle (tests/_gru.py) including T = 1, instances of 4 + 1 rows,
several GRUs per launch and the C3 length (T = 1024, H = 256); the module against fixtures the
reference produced (tests/golden/gen_gruenc.py) and against float64 torch.nn.GRU; the batching
of several encoders, torch.compile and the launcher's patch of the reference's SequenceEncoder.
Tolerance: 1e-3 relative (BASELINE.json fp32 parity); the per-step comparison with float64 across
the launch envelope is tests/test_gpu_recurrence_envelope.py."""
import types

import numpy as np
import pytest
import torch

from _gru import gru_backward, gru_forward
from _rec import run_gru
from _util import close, diff_report, load_fixture, rel_err

TOL = 1e-3


@pytest.fixture(scope="module")
def enc_mod(pkg_on_path):
    import encoders
    return encoders


@pytest.fixture(scope="module")
def nat(pkg_on_path):
    import mmf_native
    return mmf_native


def _inputs(rng, B, T, H):
    """xproj ~ N(0, 1) with +2 on the z slice (z near 0.8 keeps the carry d z alive over many steps:
    without it the last step's gradient dies within a few steps and a wrong carry goes unseen),
    w_hh, b_hn ~ U(+-1/sqrt(H))."""
    bound = 1.0 / np.sqrt(H)
    xproj = rng.standard_normal((B, T, 3 * H)).astype(np.float32)
    xproj[..., H:2 * H] += 2.0
    w = rng.uniform(-bound, bound, size=(3 * H, H)).astype(np.float32)
    b_hn = rng.uniform(-bound, bound, size=H).astype(np.float32)
    return xproj, w, b_hn


@pytest.mark.gpu
@pytest.mark.parametrize("n,B,T,H", [(1, 1, 7, 64), (1, 2, 1, 128), (3, 5, 33, 64), (2, 4, 20, 192), (4, 9, 16, 256)])
def test_recurrence_matches_oracle(nat, n, B, T, H):
    rng = np.random.default_rng(1000 * n + B + T + H)
    xproj_l, w_l, b_l, dh_l, ref = [], [], [], [], []
    for _ in range(n):
        xproj, w, b_hn = _inputs(rng, B, T, H)
        dh = rng.standard_normal((B, T, H)).astype(np.float32)
        h, g = gru_forward(xproj, w, b_hn)
        ref.append((h, g, gru_backward(w, h, g, dh)))
        # the carry path is alive in the oracle: the last step's gradient alone still reaches t = 0
        last = np.zeros_like(dh)
        last[:, -1] = dh[:, -1]
        dg_last = gru_backward(w, h, g, last)
        assert np.abs(dg_last[:, 0]).max() >= 1e-3 * np.abs(dg_last).max()
        xproj_l.append(xproj); w_l.append(w); b_l.append(b_hn); dh_l.append(dh)
    hs, gs, dgs = run_gru(nat, xproj_l, w_l, b_l, dh_l)
    for i in range(n):
        h, g, dg = ref[i]
        errs = rel_err(hs[i], h), rel_err(gs[i], g), rel_err(dgs[i], dg)
        print(f"gru {i} (n={n} B={B} T={T} H={H}): rel_err h {errs[0]:.2e} gates {errs[1]:.2e} dgates {errs[2]:.2e}")
        assert errs[0] <= TOL, i
        assert errs[1] <= TOL, i
        assert errs[2] <= TOL, i


@pytest.mark.gpu
def test_null_dh_equals_zeros(nat):
    """A NULL dh entry is a zero upstream gradient."""
    n, B, T, H = 2, 3, 9, 64
    rng = np.random.default_rng(5)
    ins = [_inputs(rng, B, T, H) for _ in range(n)]
    dh = rng.standard_normal((B, T, H)).astype(np.float32)
    xp, w, bn = ([v[i] for v in ins] for i in range(3))
    _, _, with_null = run_gru(nat, xp, w, bn, [dh, None])
    _, _, with_zero = run_gru(nat, xp, w, bn, [dh, np.zeros_like(dh)])
    assert np.array_equal(with_null[0], with_zero[0]) and np.array_equal(with_null[1], with_zero[1])
    assert not with_null[1].any() and with_null[0].any()


@pytest.mark.gpu
def test_recurrence_c3_length(nat):
    """The C3 chunk: T = 1024 steps, H = 256, one row, all 4 modalities in one launch; dh on the last
    step only (its gradient reaches ~49 steps back: many parity flips of the double buffer)."""
    rng = np.random.default_rng(7)
    n, B, T, H = 4, 1, 1024, 256
    ins = [_inputs(rng, B, T, H) for _ in range(n)]
    xp, w, bn = ([v[i] for v in ins] for i in range(3))
    dh_l = [np.zeros((B, T, H), np.float32) for _ in range(n)]
    for d in dh_l:
        d[:, -1] = rng.standard_normal((B, H))       # only the final state feeds the projection
    hs, gs, dgs = run_gru(nat, xp, w, bn, dh_l)
    for i in (0, 3):
        h, g = gru_forward(xp[i], w[i], bn[i])
        dg = gru_backward(w[i], h, g, dh_l[i])
        errs = rel_err(hs[i], h), rel_err(dgs[i], dg)
        print(f"gru {i} (C3 length): rel_err h {errs[0]:.2e} dgates {errs[1]:.2e}")
        assert errs[0] <= TOL
        assert errs[1] <= TOL


FIXTURES = {
    # name: (input_dim, hidden, out), layers, train
    "gruenc_2layer_len": ((17, 64, 16), 2, False),
    "gruenc_h128": ((9, 128, 32), 1, True),
}


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(FIXTURES))
def test_sequence_encoder_matches_reference(enc_mod, name):
    (din, hidden, out_dim), layers, train = FIXTURES[name]
    fx = load_fixture(name)
    model = enc_mod.GRUSequenceEncoder(din, hidden, out_dim, num_layers=layers, dropout=0.0)
    model.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in fx.items() if k.startswith("sd/")}, strict=True)
    model = model.to("cuda:0").train(train)
    x = torch.from_numpy(fx["x"]).to("cuda:0").requires_grad_(True)
    lengths = torch.from_numpy(fx["lengths"]) if "lengths" in fx else None
    out = model(x, lengths)
    (out * torch.from_numpy(fx["gout"]).to("cuda:0")).sum().backward()
    assert close(out.detach(), fx["out"], TOL, 1e-7), diff_report(out.detach(), fx["out"], TOL, 1e-7)
    assert close(x.grad, fx["dx"], TOL, 1e-7), diff_report(x.grad, fx["dx"], TOL, 1e-7)
    for key, p in model.named_parameters():
        assert close(p.grad, fx[f"grad/{key}"], TOL, 1e-7), (key, diff_report(p.grad, fx[f"grad/{key}"], TOL, 1e-7))
    if lengths is not None:
        for b, n in enumerate(lengths.tolist()):
            assert not bool(x.grad[b, n:].any()), b      # padded steps: exactly zero
    assert not enc_mod.lstm_timed_out("cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("batch_first", [True, False])
@pytest.mark.parametrize("hidden,layers", [(64, 2), (256, 1)])
def test_gru_module_forward_matches_torch(enc_mod, hidden, layers, batch_first):
    """GRU(...)(x) -> output, h_n on the HIP recurrence == float64 torch.nn.GRU on the CPU with the same
    weights; d(input) and parameter gradients through output and h_n."""
    torch.manual_seed(5)
    ref = torch.nn.GRU(12, hidden, num_layers=layers, batch_first=batch_first).train()
    mine = enc_mod.GRU(12, hidden, num_layers=layers, batch_first=batch_first).train()
    mine.load_state_dict(ref.state_dict())
    ref, mine = ref.double(), mine.to("cuda:0")
    x = torch.randn(3, 25, 12)
    if not batch_first:
        x = x.transpose(0, 1).contiguous()
    outs = []
    for m, xin in ((ref, x.double()), (mine, x.to("cuda:0"))):
        xi = xin.clone().requires_grad_(True)
        out, h = m(xi)
        (out.square().sum() + h.sum()).backward()
        outs.append((out.detach(), h.detach(), xi.grad, [p.grad for p in m.parameters()]))
    (ro, rh, rdx, rg), (mo, mh, mdx, mg) = outs
    assert mo.shape == ro.shape and mh.shape == rh.shape == (layers, 3, hidden)
    for a, b in ((mo, ro), (mh, rh), (mdx, rdx)):
        assert rel_err(a, b) <= TOL
    for (key, _), a, b in zip(ref.named_parameters(), mg, rg):
        assert rel_err(a, b) <= TOL, key
    assert not enc_mod.lstm_timed_out("cuda:0")


@pytest.mark.gpu
def test_encode_sequences_batches_modalities(enc_mod):
    """Several modalities' GRUs in shared launches == each encoder on its own."""
    torch.manual_seed(3)
    dims = {"imu_hand": 17, "imu_chest": 17, "heart_rate": 1}
    encs = {m: enc_mod.GRUSequenceEncoder(d, 128, 32, num_layers=2).to("cuda:0").eval() for m, d in dims.items()}
    seqs = {m: torch.randn(3, 40, d, device="cuda:0") for m, d in dims.items()}
    lengths = torch.tensor([40, 17, 2])
    together = enc_mod.encode_sequences(encs, seqs, lengths)
    assert list(together) == list(seqs)
    for m in dims:
        alone = encs[m](seqs[m], lengths)
        assert torch.equal(together[m], alone), m


@pytest.mark.gpu
def test_encode_sequences_mixed_kinds(enc_mod):
    """One LSTM and two GRU encoders: one batched call per kind, results in the input order."""
    torch.manual_seed(4)
    encs = {"a": enc_mod.GRUSequenceEncoder(5, 64, 16, num_layers=1),
            "b": enc_mod.SequenceEncoder(7, 64, 16, num_layers=1),
            "c": enc_mod.GRUSequenceEncoder(3, 64, 16, num_layers=1)}
    encs = {m: e.to("cuda:0").eval() for m, e in encs.items()}
    seqs = {m: torch.randn(2, 19, e.rnn.input_size, device="cuda:0") for m, e in encs.items()}
    together = enc_mod.encode_sequences(encs, seqs)
    assert list(together) == ["a", "b", "c"]
    for m in encs:
        assert torch.equal(together[m], encs[m](seqs[m])), m


@pytest.mark.gpu
def test_gru_encoder_compile_fullgraph_bit_identical(enc_mod):
    """torch.compile(fullgraph=True) of the encoder: one graph, output and dx equal to eager bit for bit."""
    torch.manual_seed(9)
    enc = enc_mod.GRUSequenceEncoder(12, 64, 16, num_layers=1).to("cuda:0").eval()
    x = torch.randn(3, 21, 12, device="cuda:0")

    def run(fn):
        xi = x.clone().requires_grad_(True)
        out = fn(xi)
        out.square().sum().backward()
        return out.detach(), xi.grad

    want = run(enc)
    torch._dynamo.reset()
    try:
        got = run(torch.compile(enc, fullgraph=True))
    finally:
        torch._dynamo.reset()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


@pytest.mark.gpu
def test_patch_encoders_routes_reference_gru(enc_mod, pkg_on_path):
    """mmf_launch.patch_encoders: a SequenceEncoder shaped like the reference's, holding a real
    torch.nn.GRU, runs its 'gru' forward on the HIP recurrence."""
    import mmf_launch

    class FrameEncoder(torch.nn.Module):
        def attention_pool(self, frames, mask=None):
            raise AssertionError("not used")

    class SequenceEncoder(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.encoder_type = "gru"
            self.dropout_layer = torch.nn.Dropout(0.1)
            self.rnn = torch.nn.GRU(11, 64, num_layers=2, batch_first=True, dropout=0.1)
            self.projection = torch.nn.Linear(64, 16)

        def forward(self, sequence, lengths=None):
            raise AssertionError("the patched forward must serve encoder_type 'gru'")

    ns = types.SimpleNamespace(FrameEncoder=FrameEncoder, SequenceEncoder=SequenceEncoder)
    mmf_launch.patch_encoders(ns)
    torch.manual_seed(13)
    stub = SequenceEncoder().to("cuda:0").eval()
    mine = enc_mod.GRUSequenceEncoder(11, 64, 16, num_layers=2).to("cuda:0").eval()
    mine.load_state_dict(stub.state_dict(), strict=True)
    x = torch.randn(3, 14, 11, device="cuda:0")
    lengths = torch.tensor([14, 6, 1])
    assert torch.equal(stub(x, lengths), mine(x, lengths))
    assert torch.equal(stub(x), mine(x))
