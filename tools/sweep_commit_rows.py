#!/usr/bin/env python3
"""Row commitments (msm377_g1_commit_rows_device) over a resident generator set, inputs and outputs resident.

Every comparison alternates the new call with a yardstick, call by call in one process after a warm-up of both, and
prints medians with quartiles.  The scalars are one row-major matrix (row i: the k scalars of output i, below 2^252 so
that the MSM pipeline accepts them), so that way A can read a row in place as the scalars of one MSM.

A. One MSM pipeline pass per row: msm377_g1_set_bases_device once (outside the timed region), then
   msm377_g1_msm_fixed_base_batch_device with n = k and batch = rows.  A call costs rows x 0.2 ms or more, so for more
   than A_ROWS rows only the first A_ROWS rows are run and the time is scaled by rows / A_ROWS -- the line says so
   ("A scaled from R rows").  Every row is one whole pipeline pass, so the scaling flatters neither side.
B. ceil(k / 16) msm377_g1_batch_mul_multi_device calls on 16 generators each, joined by msm377_g1_batch_lincomb2_device
   with a = b = 1 (stride 0).  The 16 table slots are keyed by base bytes, so every call on the next 16 generators
   rebuilds them: the rebuilds recur on every call and stay inside the timed region.  Run for k <= 256 only: at k = 1 024
   and 4 096 way B is 64 and 256 rebuilds of 7 ms or more per call, and way A is the better yardstick by far.
The set of the new call and the bases of way A are built outside the timed region; a cold msm377_g1_set_generators is
timed on its own per (k, width).  floor = rows x k x (W + 1) mixed additions of 10 field products at the bucket
accumulation's 71.4 G products/s (for 64-bit scalars the windows that hold a digit: ceil(64 / c) + 1).
Last: k = 4 096 at 1 .. 256 rows against way A in full, the search for the crossover.

    python tools/sweep_commit_rows.py [--repeats 30] [--warmup 5] > profiles/commit_rows/sweep.txt
    python tools/sweep_commit_rows.py --trace-case    # six warm calls, 2^10 rows x 1 024 generators, c = 8: the program of a kernel trace
    python tools/sweep_commit_rows.py report-trace DIR > profiles/commit_rows/kernel_trace.txt
"""
import argparse
import csv
import glob
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PRODUCT_RATE = 10.2e9 * 7  # field products per second of k_accumulate
MADD_PRODUCTS = 10         # XYZZ mixed addition: 8M + 2S
SHAPES = ((16, 32), (14, 64), (12, 256), (10, 1024), (8, 4096))  # (log2 rows, k)
A_ROWS = 1024              # way A runs at most this many rows per call; more are scaled
B_MAX_K = 256
KMAX = 4096


def quartiles(ts):
    q = statistics.quantiles(ts, n=4)
    return statistics.median(ts), q[0], q[2]


def fmt(ts, scale=1.0):
    m, q1, q3 = quartiles(ts)
    return "%.3f [%.3f..%.3f]" % (m * scale, q1 * scale, q3 * scale)


def alternate(calls, repeats, warmup):
    """Each of ``calls`` in turn, ``repeats`` times round after ``warmup`` rounds: one list of ms per call."""
    for _ in range(warmup):
        for call in calls:
            call()
    out = [[] for _ in calls]
    for _ in range(repeats):
        for ts, call in zip(out, calls):
            t0 = time.perf_counter()
            call()
            ts.append((time.perf_counter() - t0) * 1e3)
    return out


def faster(new, old, scale_old=1.0):
    """The medians differ by more than the quartile spread of the two series."""
    mn, n1, n3 = quartiles(new)
    mo, o1, o3 = quartiles(old)
    spread = max(n3 - n1, (o3 - o1) * scale_old)
    if mo * scale_old - mn > spread:
        return "faster"
    return "MISS" if mn - mo * scale_old > spread else "within the spread"


class Bench:
    def __init__(self):
        import torch

        import webgpu_msm_bls12_377_amd as msm

        self.torch, self.msm = torch, msm
        self.eng = msm.MsmEngine(1 << 16, device=0)
        self.d_gens = torch.empty(96 * KMAX, dtype=torch.uint8, device="cuda")
        self.eng.generate_bases_device(0xC0331, KMAX, self.d_gens.data_ptr())
        self.gens = bytes(self.d_gens.cpu().numpy().tobytes())  # 4 096 distinct subgroup points
        gen = torch.Generator().manual_seed(0xC0332)
        self.cells = 1 << 21
        s = torch.randint(0, 256, (self.cells, 32), dtype=torch.uint8, generator=gen)
        s[:, 31] &= 0x0F  # below 2^252 < r: legal for the MSM pipeline of way A
        self.d_s = s.cuda()
        self.d_s64 = self.d_s.clone()
        self.d_s64[:, 8:] = 0
        rows = 1 << 16
        self.d_out = torch.empty(96 * rows, dtype=torch.uint8, device="cuda")
        self.d_tmp = torch.empty(96 * rows, dtype=torch.uint8, device="cuda")
        self.d_inf = torch.empty(rows, dtype=torch.uint8, device="cuda")
        self.d_one = torch.zeros(32, dtype=torch.uint8, device="cuda")
        self.d_one[0] = 1

    def commit(self, s, rows, k):
        self.eng.commit_rows_device(s.data_ptr(), rows, k, self.d_out.data_ptr(), self.d_inf.data_ptr())

    def way_a(self, s, rows, k):
        return self.eng.msm_fixed_base_batch_device(s.data_ptr(), k, rows)

    def way_b(self, s, rows, k):
        one = self.d_one.data_ptr()
        for g in range(0, k, 16):
            out = self.d_out if g == 0 else self.d_tmp
            self.eng.batch_mul_multi_device(self.gens[96 * g : 96 * min(k, g + 16)], s.data_ptr() + 32 * g, rows, out.data_ptr(), self.d_inf.data_ptr(), "wire", 32 * k, 32)
            if g:
                self.eng.batch_lincomb2_device(self.d_out.data_ptr(), self.d_tmp.data_ptr(), one, one, rows, self.d_out.data_ptr(), self.d_inf.data_ptr(), "wire", 0, 0)

    def cold_set(self, k, c, times=3):
        ts = []
        for _ in range(times):
            self.eng.set_generators(None)
            t0 = time.perf_counter()
            self.eng.set_generators(self.gens[: 96 * k], c)
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)


def line(b, name, s, logn, k, c, digits_bits, args, with_b):
    rows = 1 << logn
    eng = b.eng
    cold = b.cold_set(k, c)
    eng.set_bases_device(b.d_gens.data_ptr(), k)  # way A's bases: outside the timed region
    a_rows = min(rows, A_ROWS)
    calls = [lambda: b.commit(s, rows, k), lambda: b.way_a(s, a_rows, k)]
    if with_b:
        eng.set_mul_window(8)
        calls.append(lambda: b.way_b(s, rows, k))
    series = alternate(calls, args.repeats, args.warmup)
    eng.set_mul_window(0)
    scale = rows / a_rows
    windows = -(-digits_bits // c) + 1
    floor = rows * k * windows * MADD_PRODUCTS / PRODUCT_RATE * 1e3
    new, a = series[0], series[1]
    best, verdict = statistics.median(a) * scale, faster(new, a, scale)
    text = "%-10s 2^%-2d x %-4d c = %-2d | call %s | A %s%s" % (name, logn, k, c, fmt(new), fmt(a, scale), " (scaled from %d rows)" % a_rows if scale != 1 else "")
    if with_b:
        text += " | B %s" % fmt(series[2])
        if statistics.median(series[2]) < best:
            best, verdict = statistics.median(series[2]), faster(new, series[2])
    else:
        text += " | B not run (k > %d)" % B_MAX_K
    m = statistics.median(new)
    text += " | call / best = %.3f: %s | floor %.3f, call / floor = %.2f | cold set_generators %.1f ms" % (m / best, verdict, floor, m / floor, cold)
    print(text, flush=True)


def sweep(args):
    b = Bench()
    print("# %s; ms per call, median [q1..q3] of %d calls after %d warm-up calls, the ways alternating call by call; inputs and outputs resident" % (
        b.msm.load_library().msm377_version().decode(), args.repeats, args.warmup))
    print("# call: commit_rows_device on a resident set; A: set_bases once + msm_fixed_base_batch_device(n = k, batch = rows); B: ceil(k / 16) batch_mul_multi_device (c = 8, slots rebuilt) + batch_lincomb2_device(a = b = 1)")
    print("# floor = rows x k x (W + 1) mixed additions of %d field products at %.1f G products/s; verdicts compare medians against the quartile spread of the two series" % (MADD_PRODUCTS, PRODUCT_RATE / 1e9))
    for logn, k in SHAPES:
        line(b, "full-width", b.d_s, logn, k, 8, 256, args, k <= B_MAX_K)
    for logn, k in ((16, 32), (14, 64)):
        line(b, "full-width", b.d_s, logn, k, 16, 256, args, True)
    line(b, "64-bit", b.d_s64, 10, 1024, 8, 64, args, False)
    print("# the crossover: k = 4 096, c = 8, full-width, few rows; A in full")
    b.eng.set_generators(b.gens, 8)
    b.eng.set_bases_device(b.d_gens.data_ptr(), KMAX)
    for rows in (1, 2, 4, 8, 16, 64, 256):
        new, a = alternate([lambda: b.commit(b.d_s, rows, KMAX), lambda: b.way_a(b.d_s, rows, KMAX)], args.repeats, args.warmup)
        print("rows = %-3d k = 4096 | call %s | A %s | call / A = %.3f: %s" % (rows, fmt(new), fmt(a), statistics.median(new) / statistics.median(a), faster(new, a)), flush=True)
    b.eng.set_generators(None)
    b.eng.close()


def trace_case():
    b = Bench()
    b.eng.set_generators(b.gens[: 96 * 1024], 8)
    for _ in range(6):
        b.commit(b.d_s, 1 << 10, 1024)
    b.eng.set_generators(None)
    b.eng.close()


def report_trace(folder):
    files = glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True)
    rows = [r for f in files for r in csv.DictReader(open(f)) if "k_bm" in r["Kernel_Name"] or "k_cr" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        r["name"] = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").replace("msm377::", "").split("(")[0][:60]
    starts = [i for i, r in enumerate(rows) if r["name"].startswith("k_cr_accumulate")]
    print("# warm calls, 2^10 rows x 1 024 generators, c = 8, full-width scalars: the launches of one call, medians over the last %d calls; us under rocprofv3 --kernel-trace" % (len(starts) - 1))
    per = {}
    for a, z in zip(starts[1:], starts[2:] + [len(rows)]):
        for pos, r in enumerate(rows[a:z]):
            per.setdefault((pos, r["name"]), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    total = 0.0
    for (pos, name), ds in sorted(per.items()):
        total += statistics.median(ds)
        print("  %2d  %-24s %9.1f" % (pos, name, statistics.median(ds)))
    print("  sum of the medians %9.1f" % total)


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "report-trace":
        report_trace(sys.argv[2])
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace-case", action="store_true")
    args = ap.parse_args()
    if args.trace_case:
        trace_case()
    else:
        sweep(args)


if __name__ == "__main__":
    main()
