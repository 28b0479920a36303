#!/usr/bin/env python3
"""Edwards-BLS12 batch multiplication (msm377_ed_batch_mul_multi_device), inputs and outputs resident.

Every comparison alternates the new call with its yardstick, call by call in one process after a warm-up of both, and
prints medians.  The scalars are one column-major matrix (column j: the n scalars of base j).

1. Against the parent's only many-point call on this curve: 2^20 64-bit scalars (the SplitMix64 stream, zero-extended) on
   ED_G against msm377_ed_generate_bases_device, bytes compared.  The new call must be faster; the ratio is reported.
2. Against msm377_g1_batch_mul_multi_device at the same (n, k, width): full-width scalars, n = 2^12, 2^16, 2^20,
   k = 1, 2, 4, 16, both widths.  The limb-mad model says 0.34 (7 x 81 against 10 x 169); the condition is a ratio
   below 1 at every shape.
3. Floor: n k (W + 1) additions of 7 products at the product rate k_accumulate<EdDev> reaches in an ed_msm_device of 2^20
   points in the same session (windows x n bucket additions over the accumulation kernel's time).  call / floor beside
   the n = 2^20 lines of 2.
4. Width rule: both widths by (n, k) (the lines of 2), and the build cost, a cold n = 1 call on k unseen bases minus a warm
   one, k = 1, 2, 4, 8.  The call runs batch_mul_multi_rule, measured for G1.

    python tools/sweep_ed_batch_mul.py [--repeats 30] [--warmup 5] > profiles/ed_batch_mul/sweep.txt
    python tools/sweep_ed_batch_mul.py --inverse-case    # warm calls of 1 and 2^12 outputs: what the pass's ONE inversion costs
    python tools/sweep_ed_batch_mul.py --trace-case      # six warm calls, k = 2, n = 2^20, c = 16: the program of a kernel trace
    python tools/sweep_ed_batch_mul.py report-trace DIR > profiles/ed_batch_mul/kernel_trace.txt
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
MADD_PRODUCTS = 7  # mixed addition on affine records
BUILD_KS = (1, 2, 4, 8)
ED_G = (
    1540945439182663264862696551825005342995406165131907382295858612069623286213,
    8003546896475222703853313610036801932325312921786952001586936882361378122196,
)
MASK64 = (1 << 64) - 1


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


def splitmix64(seed, n):
    out, x = [], seed & MASK64
    for _ in range(n):
        x = (x + 0x9E3779B97F4A7C15) & MASK64
        z = x
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
        out.append(z ^ (z >> 31))
    return out


class Bench:
    def __init__(self, kmax, cap):
        import torch

        import webgpu_msm_bls12_377_amd as msm

        self.torch, self.msm, self.cap, self.kmax = torch, msm, cap, kmax
        self.eng = msm.MsmEngine(1 << 20, device=0)
        d_ed = torch.empty(64 * 512, dtype=torch.uint8, device="cuda")
        self.eng.ed_generate_bases_device(0xEDB45E5, 512, d_ed.data_ptr())
        self.ed_points = bytes(d_ed.cpu().numpy().tobytes())  # 512 distinct subgroup points: bases, and fresh ones for cold calls
        d_g1 = torch.empty(96 * 16, dtype=torch.uint8, device="cuda")
        self.eng.generate_bases_device(0xB45E5, 16, d_g1.data_ptr())
        self.g1_points = bytes(d_g1.cpu().numpy().tobytes())
        self.fresh = kmax
        gen = torch.Generator().manual_seed(0xEDBA7C7)
        self.d_s = torch.randint(0, 256, (kmax, cap, 32), dtype=torch.uint8, generator=gen).cuda()  # column-major
        self.d_out = torch.empty(96 * cap, dtype=torch.uint8, device="cuda")
        self.d_inf = torch.empty(cap, dtype=torch.uint8, device="cuda")

    def take_fresh(self, k):
        out = self.ed_points[64 * self.fresh : 64 * (self.fresh + k)]
        self.fresh += k
        assert self.fresh <= 512
        return out

    def ed(self, s, n, k, bases=None):
        self.eng.ed_batch_mul_multi_device(bases or self.ed_points[: 64 * k], s.data_ptr(), n, self.d_out.data_ptr(), 32, 32 * self.cap)

    def g1(self, s, n, k):
        self.eng.batch_mul_multi_device(self.g1_points[: 96 * k], s.data_ptr(), n, self.d_out.data_ptr(), self.d_inf.data_ptr(), "wire", 32, 32 * self.cap)


def product_rate(b):
    """Field products per second of k_accumulate<EdDev> in an Edwards MSM of 2^20 points: windows x n bucket additions."""
    torch, eng, n = b.torch, b.eng, 1 << 20
    d_p = torch.empty(64 * n, dtype=torch.uint8, device="cuda")
    eng.ed_generate_bases_device(0xF100, n, d_p.data_ptr())
    d_k = b.d_s[0, :n].clone()
    d_k[:, 31] &= 0x03  # below 2^250: inside the subgroup order
    eng.set_timing(2)
    ts = []
    for _ in range(8):
        eng.ed_msm_device(d_p.data_ptr(), d_k.data_ptr(), n)
        ts.append(eng.stage_ms()["accumulate_kernel"])
    eng.set_timing(False)
    windows, _ = eng.last_geometry()
    ms = statistics.median(ts[2:])
    return windows * n * eng.accumulate_products() / (ms * 1e-3), ms, windows


def sweep(args):
    big = 1 << 20
    b = Bench(16, big)
    eng, torch = b.eng, b.torch
    print("# %s; ms per call, median [q1..q3] (min..max) of %d calls after %d warm-up calls; inputs and outputs resident" % (b.msm.load_library().msm377_version().decode(), args.repeats, args.warmup))
    # 1
    seed = 0xED5EED
    d_s64 = torch.zeros((big, 32), dtype=torch.uint8)
    import numpy as np

    vals = np.array([v or 1 for v in splitmix64(seed, big)], dtype=np.uint64)
    d_s64[:, :8] = torch.from_numpy(vals.view(np.uint8).reshape(big, 8))
    d_s64 = d_s64.cuda()
    d_ref = torch.empty(64 * big, dtype=torch.uint8, device="cuda")
    gx = ED_G[0].to_bytes(32, "little") + ED_G[1].to_bytes(32, "little")
    for c in (0,) + WIDTHS:
        eng.set_mul_window(c)
        ta, tb = alternate(lambda: eng.ed_generate_bases_device(seed, big, d_ref.data_ptr()),
                           lambda: eng.ed_batch_mul_multi_device(gx, d_s64.data_ptr(), big, b.d_out.data_ptr()), args.repeats, args.warmup)
        same = bool(torch.equal(d_ref, b.d_out[: 64 * big]))
        ma, mb = statistics.median(ta), statistics.median(tb)
        print("1  n = 2^20 64-bit scalars on ED_G, c = %-2d | ed_generate_bases_device %s | ed_batch_mul_multi_device %s | new / parent = %.3f (%s) | bytes equal: %s" % (
            eng.last_mul_window(), fmt(ta), fmt(tb), mb / ma, "faster" if mb < ma else "NOT FASTER", same), flush=True)
    # 3 (the rate first: the floor goes beside the lines of 2)
    rate, acc_ms, windows = product_rate(b)
    print("# 3: k_accumulate<EdDev> in ed_msm_device at 2^20 points: %.3f ms for %d windows x 2^20 additions of %d products = %.2f G products/s; floor = n k (W + 1) x %d products at that rate" % (
        acc_ms, windows, MADD_PRODUCTS, rate / 1e9, MADD_PRODUCTS))
    # 2
    print("# 2: msm377_g1_batch_mul_multi_device (G1) against msm377_ed_batch_mul_multi_device (Ed), same n, k, width, full-width scalars, alternating")
    worst = 0.0
    for c in WIDTHS:
        eng.set_mul_window(c)
        for k in (1, 2, 4, 16):
            for logn in (12, 16, 20):
                n = 1 << logn
                reps = args.repeats if k < 16 or logn < 20 else max(10, args.repeats // 3)
                ta, tb = alternate(lambda: b.g1(b.d_s, n, k), lambda: b.ed(b.d_s, n, k), reps, args.warmup)
                ma, mb = statistics.median(ta), statistics.median(tb)
                worst = max(worst, mb / ma)
                floor = n * k * (256 // c + 1) * MADD_PRODUCTS / rate * 1e3
                print("2  c = %-2d k = %-2d n = 2^%-2d | G1 %s | Ed %s | Ed / G1 = %.3f | Ed / floor = %.2f | %.2f M outputs/s" % (c, k, logn, fmt(ta), fmt(tb), mb / ma, mb / floor, n / mb / 1e3), flush=True)
    print("# 2: largest Ed / G1 = %.3f: the condition (below 1 at every shape) is %s" % (worst, "met" if worst < 1 else "MISSED"))
    # 4
    print("# 4: builds: a cold n = 1 call on k unseen bases minus a warm n = 1 call")
    for c in WIDTHS:
        eng.set_mul_window(c)
        for k in BUILD_KS:
            cold, warm = [], []
            for _ in range(3):
                bases = b.take_fresh(k)
                t0 = time.perf_counter()
                b.ed(b.d_s, 1, k, bases)
                t1 = time.perf_counter()
                b.ed(b.d_s, 1, k, bases)
                t2 = time.perf_counter()
                cold.append((t1 - t0) * 1e3)
                warm.append((t2 - t1) * 1e3)
            mc, mw = statistics.median(cold), statistics.median(warm)
            print("4  build c = %-2d k = %-2d | cold %.3f | warm %.3f | build %.3f ms (%.3f per table)" % (c, k, mc, mw, mc - mw, (mc - mw) / k), flush=True)
    eng.set_mul_window(0)
    eng.close()


def inverse_case(args):
    b = Bench(1, 1 << 12)
    b.eng.set_mul_window(8)
    print("# %s (%s)" % (b.msm.load_library().msm377_version().decode(), os.environ.get("MSM377_LIB", "the tree's library")))
    for n in (1, 1 << 12):
        for _ in range(args.warmup):
            b.ed(b.d_s, n, 1)
        ts = []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            b.ed(b.d_s, n, 1)
            ts.append((time.perf_counter() - t0) * 1e3)
        print("warm call k = 1 c = 8 n = %-5d | %s" % (n, fmt(ts)), flush=True)
    b.eng.close()


def trace_case():
    b = Bench(2, 1 << 20)
    b.eng.set_mul_window(16)
    for _ in range(6):
        b.ed(b.d_s, 1 << 20, 2)
    b.eng.set_mul_window(8)
    for _ in range(6):
        b.ed(b.d_s, 1 << 12, 2)
    b.eng.close()


def report_trace(folder):
    files = glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True)
    rows = [r for f in files for r in csv.DictReader(open(f)) if "k_edbm" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        r["name"] = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").replace("msm377::", "").split("(")[0][:60]
    starts = [i for i, r in enumerate(rows) if r["name"].startswith("k_edbm_accumulate")]
    big, small = starts[:6], starts[6:]
    for label, group in (("k = 2, n = 2^20, c = 16", big), ("k = 2, n = 2^12, c = 8", small)):
        print("# warm calls, %s, full-width scalars: the launches of one call, medians over the last %d calls; us under rocprofv3 --kernel-trace" % (label, len(group) - 1))
        per = {}
        ends = group[2:] + [group[-1] + 4]
        for a, z in zip(group[1:], ends):
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
    ap.add_argument("--inverse-case", action="store_true")
    args = ap.parse_args()
    if args.trace_case:
        trace_case()
    elif args.inverse_case:
        inverse_case(args)
    else:
        sweep(args)


if __name__ == "__main__":
    main()
