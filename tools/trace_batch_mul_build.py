#!/usr/bin/env python3
"""Per-launch durations of one table build of msm377_g1_batch_mul_device at each width, from a kernel trace:

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/trace_batch_mul_build.py run
    python tools/trace_batch_mul_build.py report DIR > profiles/batch_mul/build_trace.txt

`run` makes one warm-up build (the scratch is allocated there) and then one cold n = 1 call per width on a fresh base;
`report` prints the launches of those two calls in order (durations under the profiler's clock)."""
import csv
import glob
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run():
    import torch

    import webgpu_msm_bls12_377_amd as msm

    eng = msm.MsmEngine(1 << 16)
    d_pts = torch.empty(96 * 8, dtype=torch.uint8, device="cuda")
    eng.generate_bases_device(0xC01D, 8, d_pts.data_ptr())
    bases = bytes(d_pts.cpu().numpy().tobytes())
    d_s = torch.full((32,), 0x5A, dtype=torch.uint8, device="cuda")
    d_out = torch.empty(96, dtype=torch.uint8, device="cuda")
    for k, c in enumerate((8, 8, 16)):  # the first call is the warm-up
        eng.set_mul_window(c)
        eng.batch_mul_device(bases[96 * k : 96 * k + 96], d_s.data_ptr(), 1, d_out.data_ptr())
    eng.close()


def report(folder):
    files = glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True)
    rows = [r for f in files for r in csv.DictReader(open(f)) if "k_bm_" in r["Kernel_Name"] or "k_bmm_" in r["Kernel_Name"]]  # the build kernels are the multi-base call's
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    starts = [i for i, r in enumerate(rows) if "k_bmm_row_bases" in r["Kernel_Name"]]
    print("# one cold n = 1 call per width: the build's launches, then the call's own four; us under rocprofv3 --kernel-trace")
    for width, i in zip((8, 16), starts[1:]):
        j = starts[starts.index(i) + 1] if starts.index(i) + 1 < len(starts) else len(rows)
        t0 = int(rows[i]["Start_Timestamp"])
        print("width %d" % width)
        for r in rows[i:j]:
            s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
            name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").replace("msm377::", "")
            print("  %9.1f .. %9.1f  dur %8.1f  %s" % ((s - t0) / 1e3, (e - t0) / 1e3, (e - s) / 1e3, name.split("(")[0][:60]))


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) == 3 and sys.argv[1] == "report":
        report(sys.argv[2])
    else:
        sys.exit(__doc__)
