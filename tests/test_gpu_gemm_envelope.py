"""The sequence step's GEMM forms (csrc/gemm.hip) across their launch envelope, against the float64
oracle.

launch_gemm and the weight-gradient planner (plan_wgrads in csrc/hybrid.hip, split_rows /
plan_wgrad* in csrc/capi_util.h) choose their forms by size, and most of them are selected only
far above the shapes of the other modules on the float64 rule (at most 2,052 rows).  The cases
below are the smallest shapes that select each form on a 256-CU device with D, H <= 128; they
run the way the plan builds them, through train_step.HybridTrainStep (tests/_seqstep.py: one
forward_backward() at "highest", dropout 0.1 replayed from Philox, the device's ReLU decisions
handed to the oracle within rounding of zero).  Every case has mixed mask rows: a seeded keep rate
of 0.9, sample 1 with the fractional weights 0.5 and 0.25, sample 2 fully masked.

  env_wsr_persist   B L = 6,144 rows, 15 big weight gradients in one launch at the sized split
                    (hint path: 3 CUs / jobs per launch); the 12 Q/K projections are 576 row tiles
                    > 2 CUs, so 64 of gemm_wsr_kernel's 512 workgroups take a second tile.  None
                    of those runs straddles two groups here (they are tiles 9j + 7, 9j + 8 and a
                    group starts every 48): the walk across a group boundary is env_two_launches'
                    and env_nonpool's.  pcol_in_proj (seq_head_kernel and the tail kernels read the
                    projection epilogue's column sums; no head_fwd_kernel), poole_in_dz (the dZ
                    GEMM's recorded FLOPs hold the K = heads sources; no pool_e launch), the
                    interleaved tile order.
  env_two_launches  66 big weight gradients: two full launches of 32 (nfull = 64) and a
                    remainder launch of 2 whose jobs ask for the 256-slab maximum; 164 reduce
                    jobs in four launches of at most 48; two weight-stationary launches of 1,024
                    and 896 row tiles in groups of 32: in the second, 12 workgroups take their
                    second tile from the next group.
  env_ragged        4,100 / 2,952 / 5,330 rows: a ragged last M tile, last slabs of 4 and 50 rows
                    under the hint and a short one on the default split; every tile straddles
                    samples, so pool_e and the generic head run and the Q/K projections fall off
                    the weight-stationary kernel onto gemm_lds_kernel.
  env_generic       input widths 17 and 30, H = 96: gemm_generic_kernel for the projection
                    (RK x RK) and dX (RK x KR) at 4,125 rows.  Its weight gradients (65 slabs of
                    64 rows, the last 29) do NOT reach gemm_generic_kernel<1, 1>: a slab set of at
                    most 2^20 elements with kchunk <= 256 goes to small_slab_kernel
                    (job_small_slab), and 65 x 96 x 97 = 605,280.  The case asserts what it does
                    select; the sized split on gemm_generic_kernel<1, 1> is env_generic_kr's.
  env_generic_kr    the same at H = 128 and input widths 127 and 30: 65 x 128 x 129 = 1,073,280 and
                    65 x 128 x 128 = 1,064,960 > 2^20, so the four Q/K weight gradients (K = 4,125,
                    no multiple of 4) and the 127-wide projection's own run
                    gemm_generic_kernel<1, 1> with 65 slabs and a 29-row last one (asserted from
                    the launch's recorded FLOPs); the 30-wide projection's stays on
                    small_slab_kernel.
  env_nonpool       16 heads: the pooled plan is off; four big weight gradients per pair, the
                    out_proj one with a broadcast operand (row_div = Lq) and alpha = 1 / Lq; 27
                    big jobs.  Its 576-tile weight-stationary launch has groups of 32 tiles: 2
                    workgroups take their second tile from the next group.

Each case asserts from the launch records that its form ran (EXPECT, ABSENT and the counts in
check_forms), and from a restatement of split_rows and plan_wgrads' hint arithmetic (wgrad_plan)
that the device's CU count gives its contractions the split the case exists for; the table is
printed.  The restatement is tied to the device: the bytes the partial_reduce_kernel launches
record (per job 4 (nsplit + 1) M (N + 1)) must equal those of the restated split counts, the dZ
GEMM's recorded FLOPs those of its restated sources, and gemm_wsr_kernel's item partition, restated
too (wsr_runs), must give the second tiles and the group crossings the cases claim.  A device with
another CU count fails there instead of testing something else.

Comparison: tests/_seqstep.compare -- logits and dx/<m> one slice per sample, every parameter
gradient and the loss one slice, *key_proj.bias under zero_grad_bound -- with the CAP of
tests/test_gpu_attn_headdims.py and C by that module's rule (the next power of two at or above
twice the worst measured e_dev / max(e_32, 2^-24)).  CAP = 1e-4 is a condition; the fp32 oracle
alone stays below 2.4e-6 of each tensor's maximum at these shapes.  Parameter gradients stay one
slice because the fp32 oracle itself reaches 1.9e-5 per weight row and 3e-4 per bias element.

Measured on the MI355X at "highest" (worst ratio over the case's tensors / largest e_dev;
profiles/gemm_envelope/pytest.log has every tensor):
    env_wsr_persist 4.76 / 2.3e-6     env_two_launches 17.11 / 1.8e-6    env_ragged 13.12 / 1.8e-6
    env_generic 10.10 / 6.4e-6        env_generic_kr 9.15 / 1.7e-6       env_nonpool 3.71 / 9.5e-7
Twice the worst is 34.2 > 32, so this module takes C = 64, not that module's 32.  The worst,
17.11, is gating_layers.m1.bias of env_two_launches, and 13.12 and 10.61 are gating_layers.m1.bias
and .m2.bias of env_ragged: the tensor tests/test_gpu_attn_headdims.py already names as its worst.
It is a cancelling sum twice over, sum_b dscore[b, m] with dscore = w (g - sum_m w g).  In the
float64 oracle the 32 terms of env_two_launches' m1 sum to -1.02e-4 while their magnitudes sum to
8.30e-4, so the device's 1.02e-6 of the result is 1.3e-7 (2 ulp) of what it added up; the fp32
oracle happens to land within 6e-8.  The same tensor of env_generic is 6.4e-6 away at a ratio of
8.2 (magnitudes 73 times the sum).  Outside the gating layers the largest ratio is 10.10, one
sample's logits of env_generic (6.0e-7 from float64), and the largest of any weight or input
gradient that a GEMM form of this module produces is 5.99 (a query_proj.bias of
env_two_launches): no kernel defect was found, and nothing is allowed for one.

Two more tests on env_two_launches: two steps from the same rng state are bit-identical (the
fixed-order split-K reduce), and the step from NaN-filled allocator blocks equals the step from
clean ones bit for bit.
"""
import numpy as np
import pytest
import torch

import _seqstep
from cases import HybridCase, pair_names
from test_gpu_attn_headdims import CAP

pytestmark = pytest.mark.gpu
C = 64.0         # see the docstring: twice this module's worst measured ratio is 34.2
P_DROP = 0.1


def env_mask(batch, nmod, seed):
    """Mask rows: Bernoulli(0.9) per entry (an empty row gets one modality back), then sample 0
    complete, sample 1 with fractional weights, sample 2 fully masked."""
    rng = np.random.default_rng(seed)
    mask = (rng.uniform(size=(batch, nmod)) < 0.9).astype(np.float32)
    for b in range(batch):
        if mask[b].sum() == 0:
            mask[b, rng.integers(nmod)] = 1.0
    mask[0] = 1.0
    mask[1] = 1.0
    mask[1, 0], mask[1, -1] = 0.5, 0.25
    mask[2] = 0.0
    return mask.tolist()


def _case(name, dims, seq, batch, hidden, heads, seed, classes=5):
    names = [f"m{i}" for i in range(len(dims))]
    return HybridCase(name, names, dict(zip(names, dims)), dict(zip(names, seq)), batch=batch, hidden=hidden,
                      heads=heads, classes=classes, seed=seed, mask=env_mask(batch, len(dims), seed), full=False)


ENV_CASES = [
    _case("env_wsr_persist", (128, 128, 128), (128, 128, 128), batch=48, hidden=128, heads=4, seed=401),
    _case("env_two_launches", (8, 16, 32, 64, 16, 32), (128,) * 6, batch=32, hidden=128, heads=4, seed=402),
    _case("env_ragged", (20, 24, 36), (100, 72, 130), batch=41, hidden=128, heads=4, seed=403),
    _case("env_generic", (17, 30), (125, 125), batch=33, hidden=96, heads=4, seed=404),
    _case("env_generic_kr", (127, 30), (125, 125), batch=33, hidden=128, heads=4, seed=405),
    _case("env_nonpool", (20, 24, 36), (128, 128, 128), batch=32, hidden=128, heads=16, seed=406),
]
BY_NAME = {c.name: c for c in ENV_CASES}
WGRAD = "gemm_lds_kernel<1, 1, 16, 3, 0>"   # KR x KR on the LDS-DMA kernel at "highest"
EXPECT = {   # name prefixes of the launches each case exists for
    # (seq_head_kernel and the tail kernels read mean_L P_m from the projection epilogue's column sums)
    "env_wsr_persist": ["gemm_wsr_kernel<0>", WGRAD, "gemm_lds_kernel<0, 1, 16, 3, 0>", "partial_reduce_kernel",
                        "seq_head_kernel<128, 1>", "tail_u_kernel", "tail_ob_mfma_kernel"],
    "env_two_launches": ["gemm_wsr_kernel<0>", WGRAD, "partial_reduce_kernel"],
    "env_ragged": ["gemm_lds_kernel<0, 0, 16, 3, 0>", WGRAD, "pool_e", "head_fwd_kernel", "head_bwd_kernel"],
    "env_generic": ["gemm_generic_kernel<0, 0>", "gemm_generic_kernel<0, 1>", "small_slab_kernel"],
    "env_generic_kr": ["gemm_generic_kernel<0, 0>", "gemm_generic_kernel<0, 1>", "gemm_generic_kernel<1, 1>"],
    "env_nonpool": ["attn_fwd_kernel<32", "attn_bwd_dkv_kernel<32", "attn_bwd_dq_kernel<32", WGRAD],
}
ABSENT = {   # and the forms the case must have fallen off
    "env_wsr_persist": ["pool_e", "head_fwd_kernel", "gemm_generic_kernel"],
    "env_two_launches": ["pool_e"],
    "env_ragged": ["gemm_wsr_kernel", "seq_head_kernel", "tail_"],
    "env_generic": ["gemm_generic_kernel<1, 1>"],
}

# ---- csrc/capi_util.h split_rows and csrc/hybrid.hip plan_wgrads' hint, restated
K_BIG_ROWS, MAX_GROUPS, REDUCE_JOBS, POOL_PB_CAP = 4096, 32, 48, 4096


def split_rows(rows, hint=0):
    """(nsplit, kchunk) of a weight-gradient contraction over `rows`."""
    if hint > 0:
        kchunk = (-(-rows // hint) + 31) & ~31
        return -(-rows // kchunk), kchunk
    chunk = min(max(rows // 4, 64), 512)
    nsplit = min(max(-(-rows // chunk), 1), 64)
    kchunk = (-(-rows // nsplit) + 31) & ~31
    return -(-rows // kchunk), kchunk


def pooled(case):
    """resolve_plan's pool: at most 8 heads and heads x Lk within the pooled helpers' LDS budget."""
    return case.heads <= 8 and all(max(case.seq[m], 1) * case.heads <= POOL_PB_CAP for m in case.names)


def wgrad_plan(case, cus):
    """The long (B L-row) weight-gradient contractions of the case in plan order:
    ([(label, rows, hint, nsplit, kchunk, last slab's rows)], nbig, nfull, rem)."""
    B, nh = case.batch, case.heads
    L = {m: max(case.seq[m], 1) for m in case.names}
    pairs = [tuple(p.split("_to_")) for p in pair_names(case.names)]
    pool = pooled(case)
    jobs = []
    for q, k in pairs:
        if not pool:
            jobs += [(f"{q}_to_{k}.out_proj", B * L[q]), (f"{q}_to_{k}.value_proj", B * L[k])]
        if L[k] > 1:   # (a single key leaves the query and key projections no gradient)
            jobs += [(f"{q}_to_{k}.query_proj", B * L[q]), (f"{q}_to_{k}.key_proj", B * L[k])]
    jobs += [(f"projections.{m}", B * L[m]) for m in case.names]
    nbig = sum(rows >= K_BIG_ROWS for _, rows in jobs)
    rem = nbig % MAX_GROUPS
    nfull = nbig - rem
    out, bi = [], 0
    for label, rows in jobs:
        hint = 0
        if rows >= K_BIG_ROWS:
            hint = max(1, min(3 * cus // (MAX_GROUPS if bi < nfull else rem), 256))
            bi += 1
        nsplit, kchunk = split_rows(rows, hint)
        out.append((label, rows, hint, nsplit, kchunk, rows - (nsplit - 1) * kchunk))
    return out, nbig, nfull, rem


def reduce_bytes(case, cus):
    """The bytes launch_reduce records over the step's partial_reduce_kernel launches: per reduce job
    4 nbatch (nsplit + 1) M (N + 1 with a bias gradient), nsplit from the restated plan -- what ties
    the restated split counts to the ones the device ran."""
    B, H, nh, nmod = case.batch, case.hidden, case.heads, len(case.names)
    assert all(case.seq[m] > 1 for m in case.names)   # (no single-key pair: no plan_zero job)
    short = split_rows(B)[0]
    jobs = [(case.classes, H, 1, short, 1), (H, H, 1, short, 1)] + [(1, H, 1, short, 1)] * nmod   # classifier, gates
    if pooled(case):   # per pair: out_proj, value_proj.weight and .bias as strided batches over the heads
        jobs += [(H, H, 1, short, 1), (H // nh, H, nh, short, 0), (H // nh, 1, nh, short, 0)] * len(pair_names(case.names))
    for label, _, _, nsplit, _, _ in wgrad_plan(case, cus)[0]:
        jobs.append((H, case.dims[label.split(".")[1]] if label.startswith("projections.") else H, 1, nsplit, 1))
    return sum(4.0 * nbatch * (nsplit + 1) * m * (n + db) for m, n, nbatch, nsplit, db in jobs), len(jobs)


def dz_flops(case):
    """(the FLOPs launch_gemm records for the dZ GEMM, the part of them in poole_in_dz's K = heads
    sources): per modality 2 B L H x the summed K of its sources -- dQ W_q and dK W_k of its pairs
    (dV W_v too off the pooled plan), and pbar^T dU per pair keyed by it where poole_in_dz holds."""
    B, H, nh, nmod = case.batch, case.hidden, case.heads, len(case.names)
    pool = pooled(case)
    total = extra = 0.0
    for m in case.names:
        L = case.seq[m]
        pe = pool and L % 128 == 0 and H % 4 == 0 and nh % 4 == 0
        total += 2.0 * B * L * H * (nmod - 1) * ((2 if pool else 3) * H + (nh if pe else 0))
        extra += 2.0 * B * L * H * (nmod - 1) * (nh if pe else 0)
    return total, extra


def wsr_runs(items, tiles_per_group, cus):
    """gemm_wsr_kernel's partition of `items` row tiles over its grid of min(items, 2 CUs) workgroups
    (workgroup x takes [x items / nwg, (x + 1) items / nwg)): (workgroups with more than one tile,
    workgroups whose run straddles two groups of tiles_per_group tiles)."""
    nwg = min(items, 2 * cus)
    runs = [(x * items // nwg, (x + 1) * items // nwg) for x in range(nwg)]
    multi = sum(b - a > 1 for a, b in runs)
    cross = sum(b > a and a // tiles_per_group != (b - 1) // tiles_per_group for a, b in runs)
    return multi, cross


def check_plan(name, case, cus):
    """Print the split table of the case and assert the properties it exists for."""
    plan, nbig, nfull, rem = wgrad_plan(case, cus)
    print(f"ENVELOPE {name} on {cus} CUs: {nbig} big jobs, nfull {nfull}, rem {rem}")
    seen = set()
    for label, rows, hint, nsplit, kchunk, last in plan:
        if (rows, hint) not in seen:
            print(f"ENVELOPE {name} {label}: rows {rows}, hint {hint}, nsplit {nsplit}, kchunk {kchunk}, last slab {last}")
        seen.add((rows, hint))
        assert 0 < last <= kchunk and (nsplit - 1) * kchunk + last == rows
    hinted = [j for j in plan if j[2] > 0]
    if name == "env_wsr_persist":
        assert (nbig, nfull) == (15, 0) and len(hinted) == 15, (nbig, nfull)
        assert all(nsplit > split_rows(rows)[0] for _, rows, _, nsplit, _, _ in hinted), hinted
    elif name == "env_two_launches":
        assert (nbig, nfull, rem) == (66, 64, 2), (nbig, nfull, rem)
        assert len({j[2] for j in hinted}) == 2, "the remainder launch takes its own split count"
        # the remainder's jobs ask for the 256-slab maximum and get 32-row slabs
        assert [j[2:5] for j in hinted[-2:]] == [(256, case.batch * 128 // 32, 32)] * 2, hinted[-2:]
        # reduce jobs: the classifier's 2, a gate and a projection per modality, 5 per pooled pair
        assert 2 + 2 * len(case.names) + 5 * len(pair_names(case.names)) > 3 * REDUCE_JOBS
    elif name == "env_ragged":
        assert sorted(hint > 0 for _, _, hint, *_ in plan[-3:]) == [False, True, True], "both split rules"
        for label, rows, hint, nsplit, kchunk, last in plan:
            assert (hint > 0) == (rows >= K_BIG_ROWS)
            assert last < kchunk, (label, "the last slab is not short", last, kchunk)
            if hint > 0:
                assert last % 32 != 0, (label, "the last slab is a multiple of 32", last)
        assert {rows % 128 != 0 for _, rows, *_ in plan} == {True}, "a ragged last M tile everywhere"
    elif name in ("env_generic", "env_generic_kr"):
        assert len(hinted) == len(plan) == 6
        H = case.hidden
        for label, rows, hint, nsplit, kchunk, last in plan:
            # off the LDS-DMA kernel (job_fast): K % 4 != 0, and the projections' N = D % 4 != 0 too
            assert rows % 4 != 0 and all(d % 4 != 0 for d in case.dims.values())
            assert last < kchunk and last % 32 != 0, (label, last, kchunk)
            if "projections" not in label:
                # job_small_slab: at most 2^20 slab elements (bias column included), kchunk <= 256
                small = nsplit * H * (H + 1) <= (1 << 20) and kchunk <= 256
                assert small == (name == "env_generic"), (label, nsplit, H, kchunk)
            elif name == "env_generic_kr":
                D = case.dims[label.split(".")[1]]
                assert (nsplit * H * (D + 1) > (1 << 20)) == (D == 127), (label, nsplit, D)
    elif name == "env_nonpool":
        assert (nbig, nfull) == (27, 0) and len(hinted) == 27, (nbig, nfull)
        assert sum("out_proj" in j[0] for j in hinted) == 6


def check_forms(name, case, launches, cus):
    """The launch records show the form the case exists for."""
    ran = [k for _, k, *_ in launches]
    print(f"ENVELOPE {name} kernels: {sorted(set(ran))}")
    for want in EXPECT[name]:
        assert any(k.startswith(want) for k in ran), (want, sorted(set(ran)))
    for gone in ABSENT.get(name, []):
        assert not any(k.startswith(gone) for k in ran), (gone, sorted(set(ran)))
    H = case.hidden
    items = [round(fl / (2.0 * 128 * 128 * H)) for _, k, _, fl, _ in launches if k == "gemm_wsr_kernel<0>"]
    wg = [k for s, k, *_ in launches if s == "bwd.wgrad_gemm"]
    red = [by for s, k, _, _, by in launches if s == "bwd.wgrad_reduce" and k == "partial_reduce_kernel"]
    print(f"ENVELOPE {name} bwd.wgrad_gemm: {wg}; bwd.wgrad_reduce: {len(red)} launches")

    # the split counts the device ran are the restated ones: the reduce launches' recorded bytes
    want_by, njobs = reduce_bytes(case, cus)
    print(f"ENVELOPE {name} reduce bytes recorded {sum(red):.6e}, restated {want_by:.6e} over {njobs} jobs")
    assert len(red) == -(-njobs // REDUCE_JOBS), (len(red), njobs)
    assert abs(sum(red) - want_by) <= 1e-5 * want_by, (sum(red), want_by)
    # the dZ GEMM's sources: with poole_in_dz the K = heads sources ride in it (nsrc > 1)
    dz = sum(fl for s, _, _, fl, _ in launches if s == "bwd.dZ_gemm")
    want_dz, extra = dz_flops(case)
    print(f"ENVELOPE {name} dZ GEMM FLOPs recorded {dz:.6e}, restated {want_dz:.6e}, of them E_m sources {extra:.6e}")
    assert abs(dz - want_dz) <= 1e-5 * want_dz, (dz, want_dz)
    assert (extra > 0) == (name in ("env_wsr_persist", "env_two_launches")), (name, extra)

    # the weight-stationary grid: workgroups with a second tile, and runs that straddle two groups
    # (every weight-stationary job of these cases has B L / 128 row tiles)
    parts = [wsr_runs(n, case.batch * case.seq[case.names[0]] // 128, cus) for n in items]
    print(f"ENVELOPE {name} gemm_wsr_kernel<0> row tiles per launch {items}: (workgroups with a second tile, "
          f"workgroups across a group boundary) {parts}")
    if name == "env_wsr_persist":
        # more row tiles than the persistent grid has workgroups: a second tile per workgroup
        assert max(items) > 2 * cus and parts[0][0] > 0, (items, cus, parts)
        assert wg.count(WGRAD) == 1, wg
    elif name == "env_two_launches":
        assert wg.count(WGRAD) >= 3, wg
        assert len(red) >= 2, red
        assert len(items) >= 2 and max(items) == MAX_GROUPS * case.batch, items
        assert sum(c for _, c in parts) > 0, ("no workgroup walks across a group boundary", items, parts)
    elif name == "env_generic_kr":
        # the generic KR x KR launch holds the four Q/K weight gradients and the 127-wide projection's
        gen = [fl for s, k, _, fl, _ in launches if s == "bwd.wgrad_gemm" and k == "gemm_generic_kernel<1, 1>"]
        want = 2.0 * H * (4 * H + 127) * case.batch * 125
        assert len(gen) == 1 and abs(gen[0] - want) <= 1e-5 * want, (gen, want)
    elif name == "env_nonpool":
        assert wg.count(WGRAD) == 1, wg
        assert sum(c for _, c in parts) > 0, ("no workgroup walks across a group boundary", items, parts)


@pytest.fixture(scope="module")
def env(pkg_on_path):
    if not torch.cuda.is_available():
        pytest.fail("no ROCm device visible")
    import fusion
    import mmf_native
    import train_step
    mmf_native.lib()
    return fusion, mmf_native, train_step


def device_cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.parametrize("name", [c.name for c in ENV_CASES])
def test_envelope_step_vs_fp64(env, name):
    fusion, nat, train_step = env
    case = BY_NAME[name]
    cus = device_cus()
    check_plan(name, case, cus)
    prev = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision("highest")
    try:
        step, sd, got, launches, seed, offset = _seqstep.device_step(nat, fusion, train_step, case, P_DROP)
    finally:
        torch.set_float32_matmul_precision(prev)
    ref64, ref32 = _seqstep.gated_references(step, case, sd, seed, offset, P_DROP, f"ENVELOPE {name}")
    bad, _, _ = _seqstep.compare(got, ref64, ref32, f"ENVELOPE {name}", C, CAP)
    check_forms(name, case, launches, cus)
    assert not bad, "\n".join(bad)


def _two_launch_step(env, before=None):
    """env_two_launches' outputs from a fresh step object at the pinned rng state."""
    fusion, _, train_step = env
    case = BY_NAME["env_two_launches"]
    torch.cuda.empty_cache()
    if before is not None:
        before()
    step, _ = _seqstep.make_step(fusion, train_step, case, P_DROP)
    step.forward_backward()
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in _seqstep.step_outputs(step, case).items()}


@pytest.fixture()
def highest():
    prev = torch.get_float32_matmul_precision()
    torch.set_float32_matmul_precision("highest")
    yield
    torch.set_float32_matmul_precision(prev)


def test_two_launches_is_deterministic(env, highest):
    """Two steps from the same rng state are bit-identical in every output, and so is a second
    forward_backward() of the same step object: the split-K reduce sums its slabs in a fixed order."""
    fusion, _, train_step = env
    case = BY_NAME["env_two_launches"]
    a = _two_launch_step(env)
    step, _ = _seqstep.make_step(fusion, train_step, case, P_DROP)
    step.forward_backward()
    b = {k: v.clone() for k, v in _seqstep.step_outputs(step, case).items()}
    step.rng.copy_(torch.tensor([_seqstep.SEED, _seqstep.OFFSET], dtype=torch.int64))
    step.forward_backward()
    c = _seqstep.step_outputs(step, case)
    assert set(a) == set(b) == set(c)
    for key in a:
        assert bool(torch.isfinite(a[key]).all()), key
        assert torch.equal(a[key], b[key]), (key, "two step objects differ")
        assert torch.equal(b[key], c[key]), (key, "the second call of one step object differs")


def test_two_launches_reads_no_uninitialized_memory(env, highest):
    """The step whose buffers come from NaN-filled allocator blocks equals the step from clean
    ones bit for bit: no slab, partial or workspace element is read before the step wrote it."""
    from test_gpu_headline import _poison_allocator
    dev = torch.device("cuda", 0)
    poisoned = _two_launch_step(env, before=lambda: _poison_allocator(dev, big_mb=512, small_n=256))
    clean = _two_launch_step(env)
    for key in clean:
        assert bool(torch.isfinite(poisoned[key]).all()), (key, int((~torch.isfinite(poisoned[key])).sum()))
        assert torch.equal(poisoned[key], clean[key]), key
