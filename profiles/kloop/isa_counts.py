"""Counts over one k-tile body of gemm_lds_kernel<{0,0},{0,1},{1,1},16,3,0> in a hipcc -S listing of csrc/gemm.hip.
Window: from the label of the basic block that holds the tile's first fp32 MFMA to its 32nd MFMA (straight-line text,
branched-around blocks included).  Staging that runs ahead of that block (the previous kernel's per-tile address work)
is outside it.  full_waits_between / s_loads_between: between the first and the 32nd MFMA only.
usage: python profiles/kloop/isa_counts.py <listing.s> ..."""
import re, sys
def analyse(path):
    lines = open(path).read().splitlines()
    out = {}
    for form in ("ILi0ELi0", "ILi0ELi1", "ILi1ELi1"):
        pat = re.compile(r"^_ZN3mmf12_GLOBAL__N_115gemm_lds_kernel%sELi16ELi3ELi0ELi0ELi0E.*:" % form)
        start = next(i for i, l in enumerate(lines) if pat.match(l))
        end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
        mf = [i for i in range(start, end) if "v_mfma_f32_32x32x2_f32" in lines[i]]
        a, b = mf[0], mf[31]
        # back up to the first fragment ds_read before the first MFMA (contiguous block start: the label)
        k = a
        while not lines[k].startswith(".LBB"): k -= 1
        body = [l.strip() for l in lines[k:b + 1] if l.strip() and not l.strip().startswith(";")]
        between = [l.strip() for l in lines[a:b + 1]]
        out[form] = dict(
            full_waits_between=sum(1 for l in between if l.startswith("s_waitcnt") and "lgkmcnt(0)" in l),
            counted_waits=sum(1 for l in body if l.startswith("s_waitcnt") and re.search(r"lgkmcnt\([1-9]", l)),
            s_loads_between=sum(1 for l in between if l.startswith("s_load")),
            valu=sum(1 for l in body if l.startswith("v_") and not l.startswith("v_mfma") and not l.startswith("v_readlane") and not l.startswith("v_writelane")),
            ds_reads=sum(1 for l in body if l.startswith("ds_read")),
            insts=len([l for l in body if not l.startswith(".")]))
    return out
for p in sys.argv[1:]:
    print(p)
    for f, d in analyse(p).items(): print(" ", f, d)
