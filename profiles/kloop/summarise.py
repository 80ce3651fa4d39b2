"""Prints the figures of README.md from the raw files of this directory: python profiles/kloop/summarise.py"""
import csv
import glob
import json
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
STAGES = ("fwd.proj_gemm", "bwd.dZ_gemm", "bwd.dx_gemm", "bwd.wgrad_gemm")
MICRO = ("proj", "dZ", "dZ_K256", "dZ_K1024", "dZ_Al2", "wgrad")


def ab(d):
    arms = sorted({re.sub(r"_\d+\.json$", "", os.path.basename(f)) for f in glob.glob(os.path.join(HERE, d, "ab", "*.json"))})
    print(f"## {d}/ab: ms_per_step of each run; mean; max - min; per-launch-group stage times (us, min-max over the runs)")
    for arm in arms:
        rows = [json.loads(open(f).read().strip().splitlines()[-1]) for f in sorted(glob.glob(os.path.join(HERE, d, "ab", arm + "_*.json")))]
        ms = [r["ms_per_step"] for r in rows]
        st = {k: "%.1f-%.1f" % (1e3 * min(r["stage_ms"][k] for r in rows), 1e3 * max(r["stage_ms"][k] for r in rows)) for k in STAGES}
        print(f"{arm:8s} {' '.join('%.4f' % m for m in ms)}  mean {sum(ms) / len(ms):.4f}  range {max(ms) - min(ms):.4f}  {st}")


def micro(d):
    arms = sorted({re.sub(r"^micro_(.*)_run\d+\.txt$", r"\1", os.path.basename(f)) for f in glob.glob(os.path.join(HERE, d, "micro_*.txt"))})
    print(f"## {d}: gemm_micro, us of runs 1 2 3; slope = (dZ_K1024 - dZ_K256) / 48 k-tile rounds")
    for arm in arms:
        vals = {}
        for f in sorted(glob.glob(os.path.join(HERE, d, f"micro_{arm}_run*.txt"))):
            for line in open(f):
                p = line.split()
                if len(p) >= 2 and p[0] in MICRO:
                    vals.setdefault(p[0], []).append(float(p[1]))
        slope = [(a - b) / 48 for a, b in zip(vals["dZ_K1024"], vals["dZ_K256"])]
        print(f"{arm:8s} " + "  ".join(f"{k} {'/'.join('%.1f' % v for v in vals[k])}" for k in MICRO) + "  slope " + "/".join("%.2f" % s for s in slope))


def kernels(d):
    for arm in ("parent", "new"):
        f = os.path.join(HERE, d, f"c2_kernel_stats_{arm}.csv")
        if os.path.exists(f):
            for row in csv.reader(open(f)):
                if row and "gemm_lds_kernel" in row[0]:
                    print(f"{d} {arm} {re.search(r'gemm_lds_kernel<[^>]*>', row[0]).group(0)}: calls {row[1]}, average {float(row[3]) / 1e3:.1f} us, min {float(row[5]) / 1e3:.1f}, max {float(row[6]) / 1e3:.1f}")


for d in ("steps1", "steps2", "final"):
    if os.path.isdir(os.path.join(HERE, d)):
        ab(d)
        micro(d)
        kernels(d)
