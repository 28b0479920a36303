#!/usr/bin/env python3
"""Per-launch times of one pass of msm377_ed_batch_mul_var_device, from rocprofv3 --kernel-trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/trace_ed_batch_mul_var.py run
    python tools/trace_ed_batch_mul_var.py summarise DIR > profiles/ed_batch_mul_var/kernel_trace.txt

run: six calls at n = 2^17 (ONE pass, full-width scalars) after two warm-up calls, alternating with
ed_check_points_device(CHECK_SUBGROUP) on the same points.  summarise: median microseconds per launch of the last six
passes, the walk's, the table's and the two normalisations' share of a pass, and the share of the single-lane k_edbm_across.
"""
import csv
import glob
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1 << 17
CALLS = 6


def run():
    sys.path.insert(0, ROOT)
    import torch

    import webgpu_msm_bls12_377_amd as msm

    eng = msm.MsmEngine(N, device=0)
    d_pts = torch.empty(64 * N, dtype=torch.uint8, device="cuda")
    d_out = torch.empty(64 * N, dtype=torch.uint8, device="cuda")
    eng.ed_generate_bases_device(0x377ED, N, d_pts.data_ptr())
    d_s = torch.randint(0, 256, (N, 32), dtype=torch.uint8, generator=torch.Generator().manual_seed(0xBA7C5)).cuda()
    for _ in range(2 + CALLS):
        eng.ed_check_points_device(d_pts.data_ptr(), N, msm.CHECK_SUBGROUP)
        eng.ed_batch_mul_var_device(d_pts.data_ptr(), d_s.data_ptr(), N, d_out.data_ptr())
    eng.close()


def summarise(directory):
    path = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))[0]
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    short = lambda r: r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("msm377::", "").replace("void ", "").split("(")[0]  # noqa: E731
    walks = [i for i, r in enumerate(rows) if "k_edbmv_accumulate" in r["Kernel_Name"]][-CALLS:]
    # a pass: k_edbmv_table, up / across / down (table), k_edbmv_accumulate, up / across / down (outputs)
    names = ["k_edbmv_table", "k_edbm_up (table)", "k_edbm_across (table)", "k_edbm_down<table>", "k_edbmv_accumulate", "k_edbm_up (outputs)", "k_edbm_across (outputs)", "k_edbm_down<wire>"]
    per = [[] for _ in names]
    for w in walks:
        for j, i in enumerate(range(w - 4, w + 4)):
            r = rows[i]
            assert names[j].split(" ")[0].split("<")[0] in short(r), (names[j], short(r))
            per[j].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    med = [statistics.median(p) for p in per]
    total = sum(med)
    print("# rocprofv3 --kernel-trace of %d msm377_ed_batch_mul_var_device calls at n = 2^17 (ONE pass, full-width scalars)" % CALLS)
    print("# alternating with ed_check_points_device(CHECK_SUBGROUP) on the same points, one MI355X; median microseconds per launch")
    for nm, m in zip(names, med):
        print("%-28s %9.1f" % (nm, m))
    print("# sum %.0f us per pass; the walk is %.1f %% of it, the table kernel %.1f %%, the table's normalisation %.1f %%, the outputs' %.1f %%;"
          % (total, 100 * med[4] / total, 100 * med[0] / total, 100 * sum(med[1:4]) / total, 100 * sum(med[5:8]) / total))
    print("# the two single-lane k_edbm_across launches %.1f %% (the number a projective per-point table would be judged against: the table's three launches, %.1f us)"
          % (100 * (med[2] + med[6]) / total, sum(med[1:4])))
    for key in ("k_check_curve", "k_check_subgroup"):
        d = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in rows if key in r["Kernel_Name"]]
        print("%-28s %9.1f   (%d launches)" % (key, statistics.median(d), len(d)))


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) == 3 and sys.argv[1] == "summarise":
        summarise(sys.argv[2])
    else:
        sys.exit(__doc__)
