"""Every length of k-loop that gemm_lds_kernel's fp32 forms (csrc/gemm.hip, gemm_lds_body)
distinguish, through all three operand-mode forms, against the float64 oracle and bit for bit
against the kernel's previous version.

The k-loop walks k-tiles of 16 through a 3-deep LDS ring.  When the issuing cursor moves to another
source (and in the prologue) it computes that source's running pointers and lane offsets; a whole
tile of a row_div == 1 source is then issued from them (between the MFMAs once the source is the
staged one), a partial last tile and row_div != 1 operands through the clamped per-tile addresses.
The consuming side learns a tile's valid depth from a queue the issue fills.  The cases give every
one of those paths contractions that begin and end on it:

  kloop_w4_12_16    projection widths (K of the RK x RK projection GEMM, N of the RK x KR dX GEMM)
  kloop_w20_32_44   4 .. 80: 1, 2, 3, 4 and 5 k-tiles -- a prologue that issues fewer tiles than
  kloop_w48_52      the ring holds, a ring that wraps, k tails of 4 and 12, a lone partial tile
  kloop_w64_80      (widths 4 and 12).  B L = 5 x 100 rows: a ragged last row tile, ragged column
                    tiles for dX, and weight-gradient slabs (KR x KR, split_rows: 4 of 128 rows) of
                    128, 128, 128 and 116 rows, so the last slab ends in a partial tile.
  kloop_dz_h4       L = 128, B = 3: poole_in_dz puts the K = heads sources (4 and 8) last in the
  kloop_dz_h8       dZ GEMM, so its contraction ends on a partial tile right after a source switch.
  kloop_hidden64    hidden 64: N < 128 on every output.

All of them run the way the plan builds them (tests/_seqstep.py: one forward_backward() at
"highest", dropout 0.1 replayed), with tests/test_gpu_gemm_envelope.py's masks, comparison, C and
CAP.  CAP = 1e-4 is a condition: on the CPU the fp32 oracle alone stays below 1.6e-6 of each
slice's maximum for these seeds (tests/_seqstep.oracle_step at float32 against float64, plain ReLU;
the largest, 1.51e-6, is gating_layers.m0.bias of kloop_dz_h8).  Each case asserts from the launch
records that gemm_lds_kernel's RK x RK, RK x KR and KR x KR forms ran and gemm_generic_kernel did
not.

Bit-identity: tests/golden/kloop_parent_hashes.json (tests/golden/gen_kloop_hashes.py, run on the
MI355X with the library built from the commit before the k-loop change) holds the SHA-256 of the
float32 bytes of the loss, the logits and every parameter and input gradient of kloop_w20_32_44 and
kloop_dz_h8; the k-loop change moves address work and DMA issue, not sums, so they must not move.  On
kloop_w20_32_44 also: two steps from the same rng state are bit-identical, and a step from
NaN-filled allocator blocks equals one from clean blocks.
"""
import hashlib
import json
from pathlib import Path

import pytest
import torch

import _seqstep
from test_gpu_gemm_envelope import C, CAP, P_DROP, _case

pytestmark = pytest.mark.gpu

KLOOP_CASES = [
    _case("kloop_w4_12_16", (4, 12, 16), (100,) * 3, batch=5, hidden=128, heads=4, seed=501),
    _case("kloop_w20_32_44", (20, 32, 44), (100,) * 3, batch=5, hidden=128, heads=4, seed=502),
    _case("kloop_w48_52", (48, 52), (100,) * 2, batch=5, hidden=128, heads=4, seed=503),
    _case("kloop_w64_80", (64, 80), (100,) * 2, batch=5, hidden=128, heads=4, seed=504),
    _case("kloop_dz_h4", (8, 16, 24), (128,) * 3, batch=3, hidden=128, heads=4, seed=505),
    _case("kloop_dz_h8", (8, 16, 24), (128,) * 3, batch=3, hidden=128, heads=8, seed=506),
    _case("kloop_hidden64", (12, 40), (100,) * 2, batch=5, hidden=64, heads=4, seed=507),
]
BY_NAME = {c.name: c for c in KLOOP_CASES}
HASHED = ("kloop_w20_32_44", "kloop_dz_h8")
HASH_FILE = Path(__file__).resolve().parent / "golden" / "kloop_parent_hashes.json"
FORMS = ["gemm_lds_kernel<0, 0, 16, 3, 0>", "gemm_lds_kernel<0, 1, 16, 3, 0>", "gemm_lds_kernel<1, 1, 16, 3, 0>"]


def output_hashes(got):
    """{tensor name: SHA-256 of its float32 bytes}."""
    out = {}
    for key in sorted(got):
        t = got[key].detach().cpu().contiguous()
        assert t.dtype == torch.float32, (key, t.dtype)
        out[key] = hashlib.sha256(t.numpy().tobytes()).hexdigest()
    return out


@pytest.fixture(scope="module")
def env(pkg_on_path):
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible")
    import fusion
    import mmf_native
    import train_step
    mmf_native.lib()
    return fusion, mmf_native, train_step


@pytest.fixture()
def highest():
    prev = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision("highest")
    yield
    torch.set_float32_matmul_precision(prev)


def check_forms(name, case, launches):
    ran = [k for _, k, *_ in launches]
    print(f"KLOOP {name} kernels: {sorted(set(ran))}")
    for want in FORMS:
        assert any(k.startswith(want) for k in ran), (want, sorted(set(ran)))
    assert not any(k.startswith("gemm_generic_kernel") for k in ran), sorted(set(ran))
    stages = {s: k for s, k, *_ in launches}
    print(f"KLOOP {name} bwd.dZ_gemm: {stages.get('bwd.dZ_gemm')}; bwd.wgrad_gemm: "
          f"{[k for s, k, *_ in launches if s == 'bwd.wgrad_gemm']}")
    assert stages.get("bwd.dZ_gemm", "").startswith(FORMS[1]), stages.get("bwd.dZ_gemm")
    if name.startswith("kloop_dz"):
        # poole_in_dz: the K = heads sources ride in the dZ GEMM (its FLOPs hold them)
        B, H, nh, nmod = case.batch, case.hidden, case.heads, len(case.names)
        dz = sum(fl for s, _, _, fl, _ in launches if s == "bwd.dZ_gemm")
        want = sum(2.0 * B * case.seq[m] * H * (nmod - 1) * (2 * H + nh) for m in case.names)
        assert abs(dz - want) <= 1e-5 * want, (dz, want)
        assert not any(k.startswith("pool_e") for k in ran), sorted(set(ran))


@pytest.mark.parametrize("name", [c.name for c in KLOOP_CASES])
def test_kloop_step_vs_fp64(env, highest, name):
    fusion, nat, train_step = env
    case = BY_NAME[name]
    step, sd, got, launches, seed, offset = _seqstep.device_step(nat, fusion, train_step, case, P_DROP)
    ref64, ref32 = _seqstep.gated_references(step, case, sd, seed, offset, P_DROP, f"KLOOP {name}")
    bad, _, _ = _seqstep.compare(got, ref64, ref32, f"KLOOP {name}", C, CAP)
    check_forms(name, case, launches)
    assert not bad, "\n".join(bad)
    if name in HASHED:
        want = json.loads(HASH_FILE.read_text())[name]
        have = output_hashes(got)
        assert sorted(have) == sorted(want), (sorted(have), sorted(want))
        moved = [k for k in sorted(want) if have[k] != want[k]]
        assert not moved, f"not bit-identical to the previous k-loop: {moved}"


def _fresh_step(env, before=None):
    """kloop_w20_32_44's outputs from a fresh step object at the pinned rng state."""
    fusion, _, train_step = env
    case = BY_NAME["kloop_w20_32_44"]
    torch.cuda.empty_cache()
    if before is not None:
        before()
    step, _ = _seqstep.make_step(fusion, train_step, case, P_DROP)
    step.forward_backward()
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in _seqstep.step_outputs(step, case).items()}


def test_kloop_is_deterministic(env, highest):
    """Two steps from the same rng state are bit-identical in every output."""
    a = _fresh_step(env)
    b = _fresh_step(env)
    assert set(a) == set(b)
    for key in a:
        assert bool(torch.isfinite(a[key]).all()), key
        assert torch.equal(a[key], b[key]), key


def test_kloop_reads_no_uninitialized_memory(env, highest):
    """The step whose buffers come from NaN-filled allocator blocks equals the step from clean ones
    bit for bit: no LDS tile element past a k tail and no slab or workspace element is read before
    the step wrote it."""
    from test_gpu_headline import _poison_allocator
    dev = torch.device("cuda", 0)
    poisoned = _fresh_step(env, before=lambda: _poison_allocator(dev, big_mb=512, small_n=256))
    clean = _fresh_step(env)
    for key in clean:
        assert bool(torch.isfinite(poisoned[key]).all()), (key, int((~torch.isfinite(poisoned[key])).sum()))
        assert torch.equal(poisoned[key], clean[key]), key
