"""The Transformer sequence encoder (csrc/transformer.hip) per token and across its launch envelope,
against the float64 oracle of tests/_transenc.py.

tests/test_gpu_transformer_encoder.py sees the forward only after the mean over T and a Linear, at
ffn <= 96 and n <= 260 rows.  Here every tensor the forward saves (tr_saved(): per layer QKV, O, LSE, z1,
(mean, rstd), y1, Drop(ReLU(linear1)), z2, its statistics, y2) is read back from the bytes
torch.ops.mmfusion.transformer_encoder_fwd returns (_transenc.saved_views, tied to
mmf_transformer_encoder_saved_bytes) and compared one slice per valid token, at the shipped width and
ffn, at the limits tr_check promises and at the head dims, row counts and lengths where launch_gemm,
wgrad_hint / split_rows, ln_chunks / ln_group and the attention launcher take another path.

Every case runs in train mode with dropout 0.1 replayed from Philox (a fixed (seed, offset)).  No seed
keeps every linear1 pre-activation clear of the ReLU kink at these sizes, so the device's decision -- the
sign of the saved h -- is handed to both oracles within |pre| <= 1e-5 (|y1| |W1|^T + |b1|)
(_transenc.device_gates, which asserts that outside the band the device passes nothing float64 puts
clearly <= 0 and blocks nothing clearly > 0).  Per case, in this order: (a) the CPU-side conditions
(_transenc.check_conditions: every compared slice's maximum >= 1e-6 of its tensor's, the fp32 oracle's own
worst slice error <= 2.5e-5), first on the oracles under their own signs before the device runs, again on
the gated ones; (b) the device run; (c) _transenc.compare_envelope: _util.close_sliced(got, float64, fp32
oracle, c = 64, cap = 1e-4) on every saved tensor (one slice per valid token, LSE per (sample, head)), out
(per sample), dx (per valid token, every padded row exactly 0.0), every parameter gradient (one slice), and
the K third of each in_proj_bias gradient (mathematically zero) under _util.zero_grad_bound.  c = 64 is
tests/test_gpu_gemm_envelope.py's for the same GEMM, split-K and reduce kernels and 1e-4 the project's
cap; neither is tuned to this module.

The cases (_transenc.ENVELOPE_CASES) are the ten shapes the issue names and seven *_tail cases.  In the ten
the shortest sample comes last, so the trailing rows of the (B T) row space are padding: the ragged last
split-K slab, LayerNorm chunk, reduce group and forward workgroup hold rows whose gradient is exactly zero
and whose saved rows are not compared, and a kernel that mishandled such a tail would pass them.  A *_tail
case is the same shape with the lengths reversed, so those tails hold valid tokens (_transenc.tail_rows,
asserted in check_plan: every row of the last slab, chunk and forward workgroup valid); it has its base
case's plan and forms.

The forms are asserted from the launch records (check_forms): per stage the kernel expected_forms() derives
from the restated job_fast / job_small_slab rules, the FLOPs of the weight-gradient launches per form, the
partial_reduce_kernel bytes (4 (nsplit + 1) M (N + 1) per job: the restated split counts are the device's)
and the ln_col_reduce FLOPs (chunks and groups).  DESIGN.md section 3 has the table of what each case
selected on the MI355X and the measured ratios; profiles/transformer_envelope/pytest.log every tensor.

Measured on the MI355X (worst e_dev / max(e_32, 2^-24) over the case's tensors / largest e_dev):
    tr_long_64slabs 11.41 / 1.7e-6 (p = 0: 10.69 / 1.9e-6)   tr_default_ffn 3.22 / 1.1e-5
    tr_ragged_h252 4.34 / 1.0e-6     tr_h4 5.35 / 9.8e-7      tr_h12 3.88 / 6.0e-7     tr_h48 3.26 / 5.9e-7
    tr_generic_rows 3.66 / 4.7e-7    tr_scalar_epi_wide 3.54 / 1.0e-6                  tr_ffn_max 6.70 / 2.2e-6
    tr_chunk_edges 3.70 / 2.1e-6
    tr_long_64slabs_tail 10.06 / 1.7e-6   tr_default_ffn_tail 3.99 / 1.3e-6   tr_ragged_h252_tail 4.34 / 9.2e-7
    tr_h12_tail 5.61 / 6.3e-7   tr_scalar_epi_wide_tail 3.21 / 9.9e-7   tr_ffn_max_tail 8.58 / 1.6e-6
    tr_chunk_edges_tail 3.99 / 1.3e-6
The worst, 11.41, is the O rows of tr_long_64slabs (a softmax over up to 1,020 keys); no slice is beyond
c and no kernel defect was found.
"""
import pytest
import torch

import _philox
from _transenc import (C, CAP, ENVELOPE_CASES as CASES, GEN, HEADS, LDS, P_DROP, RNG, SAVED_NAMES, check_conditions,
                       compare_envelope, compared_keys, envelope_slices, gated_references, ln_plan, make_case,
                       run_device, run_device_saved, run_oracle, tail_rows, wgrad_plan)

pytestmark = pytest.mark.gpu


def expected_forms(case):
    """{stage: the kernels of its launches, per layer}.  A GEMM is on the LDS-DMA kernel when its contraction
    and the leading dimensions of both operands are multiples of 4 (a B operand stored (K, N) also needs
    N % 4 == 0), else on the generic one; none has N = 128, so none is weight-stationary."""
    H, F, hd = case.hidden, case.ffn, case.hidden // HEADS

    def gemm(bmode, ok):
        return [(LDS if ok else GEN).format(0, bmode)]

    a = 32 if hd <= 32 else 64
    prep_vec = hd % 4 == 0 and (hd // 4) & (hd // 4 - 1) == 0
    wg = sorted({j[-1] for j in wgrad_plan(case)})
    ln_bwd = ["add_layernorm_bwd", "ln_col_reduce", "ln_col_reduce"]
    return {
        "transformer.fwd.qkv_gemm": gemm(0, True), "transformer.fwd.attn": [f"attn_fwd_kernel<{a}, 0, 0>"],
        "transformer.fwd.out_gemm": gemm(0, True), "transformer.fwd.norm1": ["add_layernorm_fwd"],
        "transformer.fwd.linear1_gemm": gemm(0, True), "transformer.fwd.linear2_gemm": gemm(0, F % 4 == 0),
        "transformer.fwd.norm2": ["add_layernorm_fwd"],
        "transformer.bwd.norm2": ln_bwd, "transformer.bwd.dh_gemm": gemm(1, F % 4 == 0),
        "transformer.bwd.dy1_gemm": gemm(1, F % 4 == 0), "transformer.bwd.norm1": ln_bwd,
        "transformer.bwd.dO_gemm": gemm(1, True),
        "transformer.bwd.attn": ["attn_bwd_prep_vec_kernel" if prep_vec else "attn_bwd_prep_kernel",
                                 f"attn_bwd_dkv_kernel<{a}, 0>", f"attn_bwd_dq_kernel<{a}, 0>"],
        "transformer.bwd.dx_gemm": gemm(1, True),
        "transformer.bwd.wgrad_gemm": wg, "transformer.bwd.wgrad_reduce": ["partial_reduce_kernel"],
    }


# what each case exists for: (label -> (hint, nsplit, kchunk, last slab, kernel)) and its LayerNorm plan,
# derived by hand from the code; wgrad_plan / ln_plan must restate them and the launch records confirm them
SMALL, WG_LDS, WG_GEN = "small_slab_kernel", LDS.format(1, 1), GEN.format(1, 1)
WANT_PLAN = {
    "tr_long_64slabs": ({"linear2": (32, 32, 64, 56, WG_LDS), "linear1": (32, 32, 64, 56, WG_LDS),
                         "out_proj": (64, 64, 32, 24, WG_LDS), "in_proj": (64, 64, 32, 24, WG_LDS)},
                        (64, 24, 8, 8, 8, 2)),
    "tr_default_ffn": ({"linear2": (64, 4, 32, 15, SMALL), "linear1": (64, 4, 32, 15, SMALL),
                        "out_proj": (64, 4, 32, 15, SMALL), "in_proj": (64, 4, 32, 15, SMALL)}, (4, 15, 2, 2, 2, 1)),
    "tr_ragged_h252": ({"linear2": (64, 5, 32, 13, SMALL), "linear1": (64, 5, 32, 13, SMALL),
                        "out_proj": (64, 5, 32, 13, SMALL), "in_proj": (64, 5, 32, 13, SMALL)}, (5, 13, 3, 2, 2, 2)),
    "tr_h4": ({k: (64, 1, 32, 27, SMALL) for k in ("linear2", "linear1", "out_proj", "in_proj")}, (1, 27, 1, 1, 1, 1)),
    "tr_h12": ({k: (64, 5, 32, 12, WG_LDS) for k in ("linear2", "linear1", "out_proj", "in_proj")}, (5, 12, 3, 2, 2, 1)),
    "tr_h48": ({k: (64, 5, 32, 12, WG_LDS) for k in ("linear2", "linear1", "out_proj", "in_proj")}, (5, 12, 3, 2, 2, 1)),
    # ffn % 4 != 0 takes the two ffn weight gradients off the LDS-DMA kernel; out_proj's and in_proj's stay on it
    "tr_generic_rows": ({"linear2": (64, 5, 32, 12, SMALL), "linear1": (64, 5, 32, 12, SMALL),
                         "out_proj": (64, 5, 32, 12, WG_LDS), "in_proj": (64, 5, 32, 12, WG_LDS)}, (5, 12, 3, 2, 2, 1)),
    # 5 x 256 x 2047 = 2,620,160 > 2^20: the ffn weight gradients leave small_slab_kernel for the generic kernel
    "tr_scalar_epi_wide": ({"linear2": (32, 5, 32, 12, WG_GEN), "linear1": (32, 5, 32, 12, WG_GEN),
                            "out_proj": (64, 5, 32, 12, WG_LDS), "in_proj": (64, 5, 32, 12, WG_LDS)}, (5, 12, 3, 2, 2, 2)),
    # n = 66 is no multiple of 4; 3 x 64 x 8193 = 1,573,056 > 2^20
    "tr_ffn_max": ({"linear2": (16, 3, 32, 2, WG_GEN), "linear1": (16, 3, 32, 2, WG_GEN),
                    "out_proj": (64, 3, 32, 2, SMALL), "in_proj": (64, 3, 32, 2, SMALL)}, (3, 2, 2, 2, 1, 1)),
    "tr_chunk_edges": ({k: (64, 21, 32, 10, SMALL) for k in ("linear2", "linear1", "out_proj", "in_proj")},
                       (21, 10, 5, 5, 1, 1)),
}


# (query blocks of 128, keys per LDS chunk of attn_fwd_kernel, a length that ends inside a key chunk) by the
# kernels' constants: properties of the shape, which the launch records do not carry
WANT_ATTN = {"tr_long_64slabs": (8, 64, True), "tr_default_ffn": (1, 128, True), "tr_ragged_h252": (1, 64, True),
             "tr_h4": (1, 128, True), "tr_h12": (1, 128, True), "tr_h48": (1, 128, True),
             "tr_generic_rows": (1, 128, True), "tr_scalar_epi_wide": (1, 64, True), "tr_ffn_max": (1, 128, True),
             "tr_chunk_edges": (2, 128, True)}


def check_plan(name, case):
    """Print the restated split, LayerNorm and attention numbers and assert they are what the case exists
    for; a *_tail case has the plan of its base case and valid tokens in every ragged tail."""
    base = name[:-len("_tail")] if name.endswith("_tail") else name
    n, hd = case.B * case.T, case.hidden // HEADS
    plan, ln = wgrad_plan(case), ln_plan(case)
    for label, M, N, hint, nsplit, kchunk, last, kern in plan:
        print(f"TRENV {name} wgrad {label} ({M} x {N} over {n} rows): hint {hint}, nsplit {nsplit}, kchunk {kchunk}, "
              f"last slab {last} rows, {kern}")
        assert 0 < last <= kchunk and (nsplit - 1) * kchunk + last == n
    print(f"TRENV {name} LayerNorm: forward {-(-n // 4)} workgroups ({(n - 1) % 4 + 1} rows in the last), backward "
          f"{ln[0]} chunks (last {ln[1]} rows) in {ln[3]} groups of {ln[2]} (last {ln[4]}), {ln[5]} column blocks in "
          f"ln_col_reduce")
    kc = 128 if hd <= 32 else 64
    attn = (-(-case.T // 128), kc, any(v % kc for v in case.lengths))
    print(f"TRENV {name} attention: head_dim {hd}, {attn[0]} query blocks, key chunks of {kc}, lengths {case.lengths}")
    tails = tail_rows(case)
    print(f"TRENV {name} valid rows in the ragged tails (valid, rows): {tails}")
    want, want_ln = WANT_PLAN[base]
    assert {j[0]: (j[3], j[4], j[5], j[6], j[7]) for j in plan} == want, (name, plan)
    assert ln == want_ln, (name, ln)
    assert attn == WANT_ATTN[base], (name, attn)
    if base == "tr_chunk_edges":   # lengths on and next to the 64- and 128-key edges
        assert sorted(case.lengths) == [1, 64, 128, 129, 130]
    if name != base:
        for key, (valid, rows) in tails.items():
            assert valid == rows or (key == "ln_group" and valid > 0), (name, key, valid, rows)


def approx(want):
    """The launch records carry six significant digits."""
    return pytest.approx(want, rel=1e-5, abs=0.0)


def check_forms(name, case, launches, p):
    """The launch records show the forms and counts the case exists for."""
    by_stage = {}
    for stage, kern, _, fl, by in launches:
        by_stage.setdefault(stage, []).append((kern, fl, by))
    print(f"TRENV {name} launches: " + "; ".join(f"{s.replace('transformer.', '')}: {[k for k, _, _ in v]}"
                                                 for s, v in by_stage.items()))
    L, n, H, F = case.layers, case.B * case.T, case.hidden, case.ffn
    want = expected_forms(case)
    for stage, kerns in want.items():
        ran = sorted(k for k, _, _ in by_stage.get(stage, []))
        if stage == "transformer.bwd.wgrad_gemm":   # (a form may take more than one launch)
            assert sorted(set(ran)) == kerns and len(ran) >= L * len(kerns), (name, stage, ran, kerns)
        else:
            assert ran == sorted(kerns * L), (name, stage, ran, kerns)
    for stage in ("transformer.fwd.rng", "transformer.fwd.mask", "transformer.fwd.pool", "transformer.bwd.mask",
                  "transformer.bwd.pool"):
        assert len(by_stage.get(stage, [])) == 1, (name, stage, by_stage.get(stage))
    assert set(by_stage) == set(want) | {"transformer.fwd.rng", "transformer.fwd.mask", "transformer.fwd.pool",
                                         "transformer.bwd.mask", "transformer.bwd.pool"}, sorted(by_stage)
    plan = wgrad_plan(case)
    # where each weight gradient went: the FLOPs its form's launches record
    for kern in want["transformer.bwd.wgrad_gemm"]:
        got_fl = sum(fl for k, fl, _ in by_stage["transformer.bwd.wgrad_gemm"] if k == kern)
        want_fl = L * sum(2.0 * M * N * n for _, M, N, *_, kk in plan if kk == kern)
        print(f"TRENV {name} {kern} weight-gradient FLOPs recorded {got_fl:.6e}, restated {want_fl:.6e}")
        assert abs(got_fl - want_fl) <= 1e-5 * want_fl, (name, kern, got_fl, want_fl)
    # the split counts the device ran are the restated ones
    red = sum(by for _, _, by in by_stage["transformer.bwd.wgrad_reduce"])
    want_red = L * sum(4.0 * (nsplit + 1) * M * (N + 1) for _, M, N, _, nsplit, *_ in plan)
    print(f"TRENV {name} partial_reduce_kernel bytes recorded {red:.6e}, restated {want_red:.6e}")
    assert abs(red - want_red) <= 1e-5 * want_red, (name, red, want_red)
    # the LayerNorm backward's chunks and groups: ln_col_reduce records chunks x 2H, then groups x 2H
    chunks, _, _, ngroup, _, _ = ln_plan(case)
    for stage in ("transformer.bwd.norm1", "transformer.bwd.norm2"):
        fl = [f for k, f, _ in by_stage[stage] if k == "ln_col_reduce"]
        assert fl == approx([1.0 * chunks * 2 * H, 1.0 * ngroup * 2 * H] * L), (name, stage, fl, chunks, ngroup)
        by = [b for k, _, b in by_stage[stage] if k == "add_layernorm_bwd"]
        assert by == approx([(16.0 if p > 0 else 12.0) * n * H] * L), (name, stage, by)   # dr is written only under dropout
    # the K = ffn contraction and the ffn-wide outputs: linear2's, linear1's and the gated dH GEMM's FLOPs
    for stage in ("transformer.fwd.linear1_gemm", "transformer.fwd.linear2_gemm", "transformer.bwd.dh_gemm",
                  "transformer.bwd.dy1_gemm"):
        assert [f for _, f, _ in by_stage[stage]] == approx([2.0 * n * H * F] * L), (name, stage, by_stage[stage])
    fl = [f for _, f, _ in by_stage["transformer.fwd.attn"]]
    assert fl == approx([4.0 * case.B * case.T * case.T * H] * L), (name, fl)


@pytest.fixture(scope="module")
def env(pkg_on_path):
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible")
    import encoders
    import mmf_native
    mmf_native.lib()
    return encoders, mmf_native


def cached_masks(p):
    """_philox.mask_provider at the module's (seed, offset), each site's mask built once."""
    if p <= 0.0:
        return None
    fn, memo = _philox.mask_provider(RNG[0], RNG[1], p), {}

    def masks(site, t):
        key = (site, tuple(t.shape))
        if key not in memo:
            memo[key] = fn(site, t)
        return memo[key]
    return masks


def run_case(env, name, p):
    enc_mod, nat = env
    case = CASES[name]
    tag = f"TRENV {name}" + ("" if p > 0 else " p=0")
    check_plan(name, case)
    sd, x, lengths, gout = make_case(case)
    masks = cached_masks(p)
    # (a) the conditions, from the oracles under their own signs, before the device runs
    own64 = run_oracle(case, sd, x, lengths, gout, torch.float64, p=p, mask_fn=masks)
    own32 = run_oracle(case, sd, x, lengths, gout, torch.float32, p=p, mask_fn=masks)
    check_conditions(own64, own32, case.layers, tag + " (own signs)")
    # (b) the device
    got, launches = run_device_saved(enc_mod, nat, case, sd, x, lengths, gout, dropout=p, rng=RNG)
    h_dev = {k: got[f"h/{k}"] for k in range(case.layers)}
    ref64, ref32, _ = gated_references(case, sd, x, lengths, gout, h_dev, p, masks, tag)
    check_conditions(ref64, ref32, case.layers, tag + " (device gates)")
    # (c) the comparison, then the forms
    bad, _, _ = compare_envelope(got, ref64, ref32, case.layers, tag, C, CAP)
    check_forms(name[:-len("_tail")] if name.endswith("_tail") else name, case, launches, p)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name", list(CASES))
def test_envelope_vs_fp64(env, name):
    run_case(env, name, P_DROP)


def test_long_without_dropout(env):
    """tr_long_64slabs in train mode at p = 0: add_layernorm_bwd's dr == nullptr path (dr = dz) at this size."""
    run_case(env, "tr_long_64slabs", 0.0)


def test_direct_entry_is_the_module_path(env):
    """run_device_saved (the ops called directly) and run_device (the module) give the same bits."""
    enc_mod, nat = env
    case = CASES["tr_h12"]
    sd, x, lengths, gout = make_case(case)
    a = run_device(enc_mod, case, sd, x, lengths, gout, dropout=P_DROP, rng=RNG)
    b, _ = run_device_saved(enc_mod, nat, case, sd, x, lengths, gout, dropout=P_DROP, rng=RNG)
    assert set(compared_keys(a)) == set(compared_keys(b))
    for k in compared_keys(a):
        assert torch.equal(a[k], b[k]), k


def _everything(res, case):
    """The saved rows of the valid tokens, out, the valid dx rows and every gradient (K thirds included)."""
    valid = torch.arange(case.T).unsqueeze(0) < torch.tensor(case.lengths).unsqueeze(1)
    out = {k: t for k, (t, _) in envelope_slices(res, valid, case.layers).items() if not k.startswith("grad/")}
    out.update({k: res[k] for k in res if k.startswith("grad/")})
    return out, valid


def test_long_reruns_and_padding(env):
    """Reference-free, on tr_long_64slabs: two runs from one rng state give the same bits in every saved
    tensor, out, dx and every gradient; a run whose padded inputs are replaced by values of magnitude 1e3
    gives the same bits in out, the valid dx rows, every gradient and every saved row of a valid token."""
    enc_mod, nat = env
    case = CASES["tr_long_64slabs"]
    sd, x, lengths, gout = make_case(case)
    a, _ = run_device_saved(enc_mod, nat, case, sd, x, lengths, gout, dropout=P_DROP, rng=RNG)
    b, _ = run_device_saved(enc_mod, nat, case, sd, x, lengths, gout, dropout=P_DROP, rng=RNG)
    assert set(a) == set(b) and all(f"{s}/{k}" in a for s in SAVED_NAMES for k in range(case.layers))
    for k in a:
        assert torch.equal(a[k], b[k]), (k, "two runs differ")
        assert k.startswith("lse/") or bool(torch.isfinite(a[k]).all()), k
    ea, valid = _everything(a, case)
    x2 = torch.where(valid.unsqueeze(-1), x, 1e3 * torch.randn(x.shape, generator=torch.Generator().manual_seed(1)))
    c, _ = run_device_saved(enc_mod, nat, case, sd, x2, lengths, gout, dropout=P_DROP, rng=RNG)
    ec, _ = _everything(c, case)
    assert float(c["dx"][~valid].abs().max()) == 0.0
    for k in ea:
        assert torch.equal(ea[k], ec[k]), (k, "the padded inputs reach it")


LIMITS = [((1, 2, 260, 8, 1), "hidden 260 is not a multiple of 4 in 4..256"),
          ((1, 2, 6, 8, 1), "hidden 6 is not a multiple of 4 in 4..256"),
          ((1, 2, 8, 8193, 1), "ffn 8193 outside 1..8192"),
          ((1, 2, 8, 8, 9), "layers 9 outside 1..8")]


@pytest.mark.parametrize("shape,text", LIMITS, ids=["hidden260", "hidden6", "ffn8193", "layers9"])
def test_host_limits(env, shape, text):
    """A shape outside tr_check's limits is refused with the library's text before any launch: the byte-size
    entry points return 0, and the forward raises with no launch recorded."""
    _, nat = env
    B, T, H, F, L = shape
    lib = nat.lib()
    assert lib.mmf_transformer_encoder_saved_bytes(B, T, H, F, L) == 0
    assert text in lib.mmf_last_error().decode()
    assert lib.mmf_transformer_encoder_workspace_bytes(B, T, H, F, L, 1) == 0
    z = lambda *s: torch.zeros(*s, device="cuda")   # noqa: E731
    params = [z(3 * H, H), z(3 * H), z(H, H), z(H), z(F, H), z(F), z(H, F), z(H), z(H), z(H), z(H), z(H)] * L
    rng = torch.tensor(RNG, dtype=torch.int64, device="cuda")
    nat.profile_begin()
    try:
        with pytest.raises(RuntimeError, match=text.replace(".", r"\.")):
            torch.ops.mmfusion.transformer_encoder_fwd(z(B, T, H), None, rng, params, True, 0.1, 1e-5)
        torch.cuda.synchronize()
    finally:
        _, launches = nat.profile_end()
    assert launches == [], launches
