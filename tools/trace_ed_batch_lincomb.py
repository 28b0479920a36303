#!/usr/bin/env python3
"""Per-launch times of the passes of one warm msm377_ed_batch_lincomb_device call, from rocprofv3 --kernel-trace.

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/trace_ed_batch_lincomb.py run K
    python tools/trace_ed_batch_lincomb.py summarise DIR K > profiles/ed_batch_lincomb/kernel_trace.txt

run: one call at n = 2^20 (16 passes, full-width scalars, K terms) after one warm-up call of the same shape; nothing else
runs.  summarise: median microseconds per launch over the 16 passes of the LAST call -- the table kernel of each round, each
table normalisation with its single-lane k_edbm_across, the walk, and the outputs' normalisation -- and each one's share
of a pass: the numbers a later change to the table rounds is judged against.
"""
import csv
import glob
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 1 << 20
PASS = 1 << 16


def run(k):
    sys.path.insert(0, ROOT)
    import torch

    import webgpu_msm_bls12_377_amd as msm

    eng = msm.MsmEngine(1 << 10, device=0)
    gen = torch.Generator().manual_seed(0xBA7C6)
    terms, keep = [], []
    for t in range(k):
        d_x = torch.empty(64 * N, dtype=torch.uint8, device="cuda")
        eng.ed_generate_bases_device(0x377E0 + t, N, d_x.data_ptr())
        d_s = torch.randint(0, 256, (N, 32), dtype=torch.uint8, generator=gen).cuda()
        keep += [d_x, d_s]
        terms.append((d_x.data_ptr(), d_s.data_ptr(), 64, 32))
    d_out = torch.empty(64 * N, dtype=torch.uint8, device="cuda")
    for _ in range(2):
        eng.ed_batch_lincomb_device(terms, N, d_out.data_ptr())
    eng.close()


def summarise(directory, k):
    path = sorted(glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True))[0]
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    short = lambda r: r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("msm377::", "").replace("void ", "").split("(")[0]  # noqa: E731
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3  # noqa: E731
    passes = N // PASS
    rounds = (k + 1) // 2
    walks = [i for i, r in enumerate(rows) if "k_edbl_accumulate" in r["Kernel_Name"]][-passes:]
    assert len(walks) == passes
    names = []
    for r in range(rounds):
        terms = "terms %d, %d" % (2 * r, 2 * r + 1) if 2 * r + 1 < k else "term %d" % (2 * r)
        names += ["k_edbl_table (round %d: %s)" % (r, terms), "k_edbm_up (round %d)" % r, "k_edbm_across (round %d)" % r, "k_edbm_down<table> (round %d)" % r]
    names += ["k_edbl_accumulate", "k_edbm_up (outputs)", "k_edbm_across (outputs)", "k_edbm_down<wire>"]
    per = [[] for _ in names]
    for w in walks:
        for j, i in enumerate(range(w - 4 * rounds, w + 4)):
            r = rows[i]
            assert names[j].split(" ")[0].split("<")[0] in short(r), (names[j], short(r))
            per[j].append(us(r))
    med = [statistics.median(p) for p in per]
    total = sum(med)
    span = (int(rows[walks[-1] + 3]["End_Timestamp"]) - int(rows[walks[0] - 4 * rounds]["Start_Timestamp"])) / 1e3
    print("# rocprofv3 --kernel-trace of one warm msm377_ed_batch_lincomb_device call, k = %d, n = 2^20 (16 passes of 2^16 outputs, full-width scalars)" % k)
    print("# median us per launch over the 16 passes [min..max], share of a pass")
    for name, m, p in zip(names, med, per):
        print("%-44s %9.1f [%8.1f..%8.1f] %5.1f %%" % (name, m, min(p), max(p), 100 * m / total))
    across = sum(m for n, m in zip(names, med) if "across" in n)
    tables = sum(med[: 4 * rounds])
    print("a pass, sum of the medians                   %9.1f us; first launch to last end of the call %.1f us (%.1f per pass)" % (total, span, span / passes))
    print("the tables of a pass (%d rounds)              %9.1f us, %.1f %%; the %d single-lane k_edbm_across launches %.1f us, %.1f %%; the walk %.1f %%" % (
        rounds, tables, 100 * tables / total, rounds + 1, across, 100 * across / total, 100 * med[4 * rounds] / total))


if __name__ == "__main__":
    if sys.argv[1] == "run":
        run(int(sys.argv[2]))
    else:
        summarise(sys.argv[2], int(sys.argv[3]))
