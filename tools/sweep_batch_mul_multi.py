#!/usr/bin/env python3
"""Multi-base batch multiplication (msm377_g1_batch_mul_multi_device), inputs and outputs resident.

Every comparison alternates the new call with its yardstick, call by call in one process after a warm-up of both, and
prints medians.  The scalars are one column-major matrix (column j: the n scalars of base j), so that a single-base call
can read a column in place.

A. The parent's way to out[i] = sum_j [s_ij]B_j: k msm377_g1_batch_mul_device calls (rule width) and k - 1
   msm377_g1_batch_lincomb2_device calls with a = b = 1 (stride 0) on their outputs.  The k single-base calls all run
   on ONE base, which flatters A: with k different bases the context's single table would be rebuilt (7 to 9 ms) before
   every one of them.  n = 2^20, 2^16, 2^12, k = 2 and 4, full-width and 64-bit scalars.  The headline is B / A.
B. k single-base calls on the same columns forced to the same width (again one base: the time does not depend on it).
   Target: at k = 2, n = 2^20, c = 16 the new call takes at most k x the single-base median of the same session -- it
   runs the same k walks and ONE normalisation where k calls run k.  k = 4, 8, 16 are reported without a target.
C. Warm calls at both widths by (n, k) and the cost of a build: a cold call (n = 1 on k bases no slot has seen) minus a
   warm n = 1 call, k = 1, 2, 4, 8, both widths -- the numbers behind batch_mul_multi_rule (csrc/batch_mul_recode.hpp).

    python tools/sweep_batch_mul_multi.py [--repeats 30] [--warmup 5] > profiles/batch_mul_multi/sweep.txt
    python tools/sweep_batch_mul_multi.py --trace-case    # six warm calls, k = 2, n = 2^20, c = 16: the program of a kernel trace
    python tools/sweep_batch_mul_multi.py --build-case    # one cold n = 1 call per (width, k): the program of a build trace
    python tools/sweep_batch_mul_multi.py report-trace DIR > profiles/batch_mul_multi/kernel_trace.txt
    python tools/sweep_batch_mul_multi.py report-build DIR > profiles/batch_mul_multi/build_trace.txt
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

WIDTHS = (8, 16)
PRODUCT_RATE = 10.2e9 * 7  # field products per second of k_accumulate
MADD_PRODUCTS = 10         # XYZZ mixed addition: 8M + 2S
BUILD_KS = (1, 2, 4, 8)


def fmt(ts):
    q = statistics.quantiles(ts, n=4)
    return "%.3f [%.3f..%.3f] (%.3f..%.3f)" % (statistics.median(ts), q[0], q[2], min(ts), max(ts))


def alternate(call_a, call_b, repeats, warmup):
    for _ in range(warmup):
        call_a()
        call_b()
    ta, tb = [], []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call_a()
        t1 = time.perf_counter()
        call_b()
        t2 = time.perf_counter()
        ta.append((t1 - t0) * 1e3)
        tb.append((t2 - t1) * 1e3)
    return ta, tb


class Bench:
    def __init__(self, kmax, cap):
        import torch

        import webgpu_msm_bls12_377_amd as msm

        self.torch, self.msm, self.cap, self.kmax = torch, msm, cap, kmax
        self.eng = msm.MsmEngine(1 << 16, device=0)
        d_pts = torch.empty(96 * 512, dtype=torch.uint8, device="cuda")
        self.eng.generate_bases_device(0xB45E5, 512, d_pts.data_ptr())
        self.points = bytes(d_pts.cpu().numpy().tobytes())  # 512 distinct subgroup points: bases, and fresh ones for cold calls
        self.fresh = kmax  # the next point no slot has seen
        gen = torch.Generator().manual_seed(0xBA7C7)
        self.d_s = torch.randint(0, 256, (kmax, cap, 32), dtype=torch.uint8, generator=gen).cuda()  # column-major
        self.d_s64 = self.d_s.clone()
        self.d_s64[:, :, 8:] = 0
        self.d_out = torch.empty(96 * cap, dtype=torch.uint8, device="cuda")
        self.d_tmp = [torch.empty(96 * cap, dtype=torch.uint8, device="cuda") for _ in range(2)]
        self.d_inf = torch.empty(cap, dtype=torch.uint8, device="cuda")
        self.d_one = torch.zeros(32, dtype=torch.uint8, device="cuda")
        self.d_one[0] = 1

    def bases(self, k):
        return self.points[: 96 * k]

    def take_fresh(self, k):
        out = self.points[96 * self.fresh : 96 * (self.fresh + k)]
        self.fresh += k
        assert self.fresh <= 512
        return out

    def multi(self, s, n, k, bases=None):
        self.eng.batch_mul_multi_device(bases or self.bases(k), s.data_ptr(), n, self.d_out.data_ptr(), self.d_inf.data_ptr(), "wire", 32, 32 * self.cap)

    def single(self, s, n, j, out):
        self.eng.batch_mul_device(self.points[:96], s.data_ptr() + 32 * self.cap * j, n, out.data_ptr(), self.d_inf.data_ptr())

    def parents_way(self, s, n, k):
        """k single-base calls, k - 1 additions through lincomb2 with a = b = 1."""
        one = self.d_one.data_ptr()
        self.single(s, n, 0, self.d_out)
        for j in range(1, k):
            self.single(s, n, j, self.d_tmp[0])
            self.eng.batch_lincomb2_device(self.d_out.data_ptr(), self.d_tmp[0].data_ptr(), one, one, n, self.d_out.data_ptr(), self.d_inf.data_ptr(), "wire", 0, 0)

    def singles(self, s, n, k):
        for j in range(k):
            self.single(s, n, j, self.d_tmp[j & 1])


def sweep(args):
    big = 1 << 20
    b = Bench(16, big)
    eng = b.eng
    print("# %s; ms per call, median [q1..q3] (min..max) of %d calls after %d warm-up calls; inputs and outputs resident" % (b.msm.load_library().msm377_version().decode(), args.repeats, args.warmup))
    print("# floor = k (W + 1) n mixed additions of %d field products at %.1f G products/s" % (MADD_PRODUCTS, PRODUCT_RATE / 1e9))
    print("# A: k batch_mul_device (one base, rule width) + (k - 1) batch_lincomb2_device(a = b = 1), B: batch_mul_multi_device (rule width), alternating, same scalars")
    for name, s in (("full-width", b.d_s), ("64-bit", b.d_s64)):
        for logn in (20, 16, 12):
            for k in (2, 4):
                n = 1 << logn
                ta, tb = alternate(lambda: b.parents_way(s, n, k), lambda: b.multi(s, n, k), args.repeats, args.warmup)
                ma, mb = statistics.median(ta), statistics.median(tb)
                print("A  %-10s n = 2^%-2d k = %-2d c = %-2d | A %s | B %s | B / A = %.3f | %.2f M outputs/s" % (name, logn, k, eng.last_mul_window(), fmt(ta), fmt(tb), mb / ma, n / mb / 1e3), flush=True)
    print("# B: k batch_mul_device calls on the columns (one base), forced to the width, against batch_mul_multi_device at that width; n = 2^20 full-width")
    for c in WIDTHS:
        eng.set_mul_window(c)
        for k in (2, 4, 8, 16):
            ta, tb = alternate(lambda: b.singles(b.d_s, big, k), lambda: b.multi(b.d_s, big, k), args.repeats, args.warmup)
            ma, mb = statistics.median(ta), statistics.median(tb)
            floor = k * (256 // c + 1) * big * MADD_PRODUCTS / PRODUCT_RATE * 1e3
            line = "B  c = %-2d k = %-2d tables %6.1f MB | k singles %s | multi %s | multi / singles = %.3f | multi / floor = %.2f" % (
                c, k, k * ((256 // c) * (1 << (c - 1)) + 1) * 128 / 1e6, fmt(ta), fmt(tb), mb / ma, mb / floor)
            if c == 16 and k == 2:
                line += " | target multi <= k x single = %.3f ms: %s" % (ma, "met" if mb <= ma else "MISSED")
            print(line, flush=True)
    print("# C: warm calls at both widths, full-width scalars; then builds: a cold n = 1 call on k unseen bases minus a warm n = 1 call")
    reps = max(5, args.repeats // 2)
    for k in (2, 4, 8):
        for logn in (12, 14, 16, 17, 18, 19, 20):
            n = 1 << logn
            med = {}
            for c in WIDTHS:
                eng.set_mul_window(c)
                for _ in range(2):
                    b.multi(b.d_s, n, k)
                ts = []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    b.multi(b.d_s, n, k)
                    ts.append((time.perf_counter() - t0) * 1e3)
                med[c] = statistics.median(ts)
            print("C  warm k = %-2d n = 2^%-2d | c = 8: %.3f | c = 16: %.3f | saved by the wide tables: %.3f ms" % (k, logn, med[8], med[16], med[8] - med[16]), flush=True)
    for c in WIDTHS:
        eng.set_mul_window(c)
        for k in BUILD_KS:
            cold, warm = [], []
            for _ in range(3):
                bases = b.take_fresh(k)
                t0 = time.perf_counter()
                b.multi(b.d_s, 1, k, bases)
                t1 = time.perf_counter()
                b.multi(b.d_s, 1, k, bases)
                t2 = time.perf_counter()
                cold.append((t1 - t0) * 1e3)
                warm.append((t2 - t1) * 1e3)
            mc, mw = statistics.median(cold), statistics.median(warm)
            print("C  build c = %-2d k = %-2d | cold %.3f | warm %.3f | build %.3f ms (%.3f per table)" % (c, k, mc, mw, mc - mw, (mc - mw) / k), flush=True)
    eng.set_mul_window(0)
    eng.close()


def trace_case():
    b = Bench(2, 1 << 20)
    b.eng.set_mul_window(16)
    for _ in range(6):
        b.multi(b.d_s, 1 << 20, 2)
    b.eng.close()


def build_case():
    b = Bench(8, 1 << 10)
    b.eng.set_mul_window(8)
    b.multi(b.d_s, 1, 1, b.take_fresh(1))  # warm-up: the scratch is allocated here
    for c in WIDTHS:
        b.eng.set_mul_window(c)
        for k in BUILD_KS:
            b.multi(b.d_s, 1, k, b.take_fresh(k))
    b.eng.close()


def trace_rows(folder):
    files = glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True)
    rows = [r for f in files for r in csv.DictReader(open(f)) if "k_bm" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        r["name"] = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").replace("msm377::", "").split("(")[0][:60]
    return rows


def report_trace(folder):
    rows = trace_rows(folder)
    starts = [i for i, r in enumerate(rows) if r["name"].startswith("k_bmm_accumulate")]
    print("# warm calls, k = 2, n = 2^20, c = 16, full-width scalars: the launches of one call, medians over the last %d calls; us under rocprofv3 --kernel-trace" % (len(starts) - 1))
    per = {}
    for a, z in zip(starts[1:], starts[2:] + [len(rows)]):
        for pos, r in enumerate(rows[a:z]):
            per.setdefault((pos, r["name"]), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    total = 0.0
    for (pos, name), ds in sorted(per.items()):
        total += statistics.median(ds)
        print("  %2d  %-24s %9.1f" % (pos, name, statistics.median(ds)))
    print("  sum of the medians %9.1f" % total)


def report_build(folder):
    rows = trace_rows(folder)
    starts = [i for i, r in enumerate(rows) if r["name"].startswith("k_bmm_row_bases")]
    print("# one cold n = 1 call per (width, k) on k unseen bases: the build's launches, then the call's own four; us under rocprofv3 --kernel-trace")
    cases = [(c, k) for c in WIDTHS for k in BUILD_KS]
    for (c, k), i, j in zip(cases, starts[1:], starts[2:] + [len(rows)]):
        t0 = int(rows[i]["Start_Timestamp"])
        print("width %d, k = %d: %d row-base launch(es)" % (c, k, sum(1 for r in rows[i:j] if r["name"].startswith("k_bmm_row_bases"))))
        for r in rows[i:j]:
            s, e = int(r["Start_Timestamp"]), int(r["End_Timestamp"])
            print("  %9.1f .. %9.1f  dur %8.1f  %s" % ((s - t0) / 1e3, (e - t0) / 1e3, (e - s) / 1e3, r["name"]))


def main():
    if len(sys.argv) == 3 and sys.argv[1] in ("report-trace", "report-build"):
        (report_trace if sys.argv[1] == "report-trace" else report_build)(sys.argv[2])
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace-case", action="store_true")
    ap.add_argument("--build-case", action="store_true")
    args = ap.parse_args()
    if args.trace_case:
        trace_case()
    elif args.build_case:
        build_case()
    else:
        sweep(args)


if __name__ == "__main__":
    main()
