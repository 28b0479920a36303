#!/usr/bin/env python3
"""Per-launch times of one pass of msm377_ed_batch_lincomb2_device, from rocprofv3 --kernel-trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/trace_ed_batch_lincomb2.py run
    python tools/trace_ed_batch_lincomb2.py summarise DIR > profiles/ed_batch_lincomb2/kernel_trace.txt

run: six calls at n = 2^16 (ONE pass, full-width scalars) after two warm-up calls, alternating with the two
ed_batch_mul_var_device calls (P, a) and (Q, b) on the same inputs.  summarise: median microseconds per launch of the last
six passes, the walk's, the table kernel's and the two normalisations' share of a pass, and the yardstick's walk beside it.
"""
import csv
import glob
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1 << 16
CALLS = 6


def run():
    sys.path.insert(0, ROOT)
    import torch

    import webgpu_msm_bls12_377_amd as msm

    eng = msm.MsmEngine(N, device=0)
    d_p = torch.empty(64 * N, dtype=torch.uint8, device="cuda")
    d_q = torch.empty(64 * N, dtype=torch.uint8, device="cuda")
    d_out = torch.empty(64 * N, dtype=torch.uint8, device="cuda")
    eng.ed_generate_bases_device(0x377ED, N, d_p.data_ptr())
    eng.ed_generate_bases_device(0x377EE, N, d_q.data_ptr())
    gen = torch.Generator().manual_seed(0xBA7C5)
    d_a = torch.randint(0, 256, (N, 32), dtype=torch.uint8, generator=gen).cuda()
    d_b = torch.randint(0, 256, (N, 32), dtype=torch.uint8, generator=gen).cuda()
    for _ in range(2 + CALLS):
        eng.ed_batch_mul_var_device(d_p.data_ptr(), d_a.data_ptr(), N, d_out.data_ptr())
        eng.ed_batch_mul_var_device(d_q.data_ptr(), d_b.data_ptr(), N, d_out.data_ptr())
        eng.ed_batch_lincomb2_device(d_p.data_ptr(), d_q.data_ptr(), d_a.data_ptr(), d_b.data_ptr(), N, d_out.data_ptr())
    eng.close()


def summarise(directory):
    path = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))[0]
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    short = lambda r: r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("msm377::", "").replace("void ", "").split("(")[0]  # noqa: E731
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3  # noqa: E731
    walks = [i for i, r in enumerate(rows) if "k_edbl2_accumulate" in r["Kernel_Name"]][-CALLS:]
    # a pass: k_edbl2_table, up / across / down (16 m table entries), k_edbl2_accumulate, up / across / down (m outputs)
    names = ["k_edbl2_table", "k_edbm_up (tables)", "k_edbm_across (tables)", "k_edbm_down<table>", "k_edbl2_accumulate", "k_edbm_up (outputs)", "k_edbm_across (outputs)", "k_edbm_down<wire>"]
    per = [[] for _ in names]
    for w in walks:
        for j, i in enumerate(range(w - 4, w + 4)):
            r = rows[i]
            assert names[j].split(" ")[0].split("<")[0] in short(r), (names[j], short(r))
            per[j].append(us(r))
    med = [statistics.median(p) for p in per]
    total = sum(med)
    print("# rocprofv3 --kernel-trace of %d msm377_ed_batch_lincomb2_device calls at n = 2^16 (ONE pass, full-width scalars)" % CALLS)
    print("# alternating with the two ed_batch_mul_var_device calls on the same inputs, one MI355X; median microseconds per launch")
    for nm, m in zip(names, med):
        print("%-28s %9.1f" % (nm, m))
    print("# sum %.0f us per pass; the walk is %.1f %% of it, the table kernel %.1f %%, the tables' normalisation %.1f %%, the outputs' %.1f %%"
          % (total, 100 * med[4] / total, 100 * med[0] / total, 100 * sum(med[1:4]) / total, 100 * sum(med[5:8]) / total))
    for key in ("k_edbmv_accumulate", "k_edbmv_table", "k_check_curve"):
        d = [us(r) for r in rows if key in r["Kernel_Name"]]
        print("%-28s %9.1f   (%d launches)" % (key, statistics.median(d), len(d)))
    var = statistics.median([us(r) for r in rows if "k_edbmv_accumulate" in r["Kernel_Name"]])
    print("# joint walk / two variable-base walks at 2^16 outputs each: %.3f (products: %.3f)" % (med[4] / (2 * var), 2752 / 4608))


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) == 3 and sys.argv[1] == "summarise":
        summarise(sys.argv[2])
    else:
        sys.exit(__doc__)
