#!/usr/bin/env python3
"""Edwards-BLS12 row commitments (msm377_ed_commit_rows_device) over a resident generator set, one GPU, inputs and outputs
resident.

Every comparison alternates the new call with a yardstick, call by call in one process after a warm-up of both, and
prints medians of --repeats calls with quartiles.  The scalars are one row-major matrix (row i: the k scalars of output i,
below 2^250 so that the MSM pipeline of way A accepts them without a rerun).

(1) The parent's ways, each compared byte for byte with the call's records:
    A. one msm377_ed_msm_device per row over the first k generators.  A call costs rows x a whole pipeline pass, so at
       most A_ROWS rows are run and the time is scaled by rows / A_ROWS -- the line says so ("A scaled from R rows").
    B. ceil(k / 16) msm377_ed_batch_mul_multi_device calls on 16 generators each, joined by
       msm377_ed_batch_lincomb2_device with a = b = 1 (stride 0).  The 16 table slots are keyed by base bytes, so every
       call on the next 16 generators rebuilds them: the rebuilds recur on every call and stay inside the timed region.
       Run for k <= 256.
(2) msm377_g1_commit_rows_device at the same rows x k x width over 4 096 G1 generators: the ratio per shape.
(3) floor = rows x k x (W + 1) additions of 7 field products at the product rate k_accumulate<EdDev> reaches in an
    ed_msm_device of 2^20 points in the same session (for 64-bit scalars the windows that hold a digit: ceil(64 / c) + 1).
Then a cold msm377_ed_set_generators per (k, width), and k = 4 096 at 1 .. 256 rows against way A in full: the crossover.

Every step -- the product rate, each shape, the cold sets, the crossover -- is a child process of its own under its own
time limit; the first one that fails or runs out of time ends the sweep.

    python tools/sweep_ed_commit_rows.py [--repeats 30] [--warmup 5] > profiles/ed_commit_rows/sweep.txt
    python tools/sweep_ed_commit_rows.py --trace-case    # six warm calls each of 2^10 x 1 024 and 2^8 x 4 096, c = 8: the program of a kernel trace
    python tools/sweep_ed_commit_rows.py report-trace DIR > profiles/ed_commit_rows/kernel_trace.txt
"""
import argparse
import csv
import glob
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MADD_PRODUCTS = 7  # mixed addition on affine records
# (name, log2 rows, k, width, scalar bits)
LINES = [("full-width", 16, 32, 8, 256), ("full-width", 14, 64, 8, 256), ("full-width", 12, 256, 8, 256), ("full-width", 10, 1024, 8, 256), ("full-width", 8, 4096, 8, 256),
         ("full-width", 16, 32, 16, 256), ("full-width", 14, 64, 16, 256), ("64-bit", 10, 1024, 8, 64)]
COLD = ((32, 8), (64, 8), (256, 8), (1024, 8), (4096, 8), (32, 16), (64, 16))
A_ROWS = 256   # way A runs at most this many rows per call; more are scaled
B_MAX_K = 256
KMAX = 4096
STEP_SECONDS = 240


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
    def __init__(self, g1=False):
        import torch

        import webgpu_msm_bls12_377_amd as msm

        self.torch, self.msm = torch, msm
        self.eng = msm.MsmEngine(1 << 20, device=0)
        self.d_gens = torch.empty(64 * KMAX, dtype=torch.uint8, device="cuda")
        self.eng.ed_generate_bases_device(0xEDC0331, KMAX, self.d_gens.data_ptr())
        self.gens = bytes(self.d_gens.cpu().numpy().tobytes())  # 4 096 distinct subgroup points
        self.g1_gens = None
        if g1:
            d_g1 = torch.empty(96 * KMAX, dtype=torch.uint8, device="cuda")
            self.eng.generate_bases_device(0xC0331, KMAX, d_g1.data_ptr())
            self.g1_gens = bytes(d_g1.cpu().numpy().tobytes())
        gen = torch.Generator().manual_seed(0xEDC0332)
        self.cells = 1 << 21
        s = torch.randint(0, 256, (self.cells, 32), dtype=torch.uint8, generator=gen)
        s[:, 31] &= 0x03  # below 2^250: inside the subgroup order, legal for way A's pipeline without a rerun
        self.d_s = s.cuda()
        self.d_s64 = self.d_s.clone()
        self.d_s64[:, 8:] = 0
        rows = 1 << 16
        self.d_out = torch.empty(96 * rows, dtype=torch.uint8, device="cuda")
        self.d_b = torch.empty(64 * rows, dtype=torch.uint8, device="cuda")
        self.d_tmp = torch.empty(64 * rows, dtype=torch.uint8, device="cuda")
        self.d_inf = torch.empty(rows, dtype=torch.uint8, device="cuda")
        self.d_one = torch.zeros(32, dtype=torch.uint8, device="cuda")
        self.d_one[0] = 1

    def commit(self, s, rows, k):
        self.eng.ed_commit_rows_device(s.data_ptr(), rows, k, self.d_out.data_ptr())

    def g1_commit(self, s, rows, k):
        self.eng.commit_rows_device(s.data_ptr(), rows, k, self.d_out.data_ptr(), self.d_inf.data_ptr())

    def way_a(self, s, rows, k):
        return b"".join(self.eng.ed_msm_device(self.d_gens.data_ptr(), s.data_ptr() + 32 * k * i, k) for i in range(rows))

    def way_b(self, s, rows, k):
        one = self.d_one.data_ptr()
        for g in range(0, k, 16):
            out = self.d_b if g == 0 else self.d_tmp
            self.eng.ed_batch_mul_multi_device(self.gens[64 * g : 64 * min(k, g + 16)], s.data_ptr() + 32 * g, rows, out.data_ptr(), 32 * k, 32)
            if g:
                self.eng.ed_batch_lincomb2_device(self.d_b.data_ptr(), self.d_tmp.data_ptr(), one, one, rows, self.d_b.data_ptr(), 64, 64, 0, 0)

    def records(self, rows):
        return bytes(self.d_out[: 64 * rows].cpu().numpy().tobytes())

    def cold_set(self, k, c, times=3):
        ts = []
        for _ in range(times):
            self.eng.ed_set_generators(None)
            t0 = time.perf_counter()
            self.eng.ed_set_generators(self.gens[: 64 * k], c)
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts)


def product_rate():
    """Field products per second of k_accumulate<EdDev> in an Edwards MSM of 2^20 points: windows x n bucket additions."""
    b = Bench()
    torch, eng, n = b.torch, b.eng, 1 << 20
    d_p = torch.empty(64 * n, dtype=torch.uint8, device="cuda")
    eng.ed_generate_bases_device(0xF100, n, d_p.data_ptr())
    d_k = b.d_s[:n].clone()
    eng.set_timing(2)
    ts = []
    for _ in range(8):
        eng.ed_msm_device(d_p.data_ptr(), d_k.data_ptr(), n)
        ts.append(eng.stage_ms()["accumulate_kernel"])
    eng.set_timing(False)
    windows, _ = eng.last_geometry()
    ms = statistics.median(ts[2:])
    rate = windows * n * eng.accumulate_products() / (ms * 1e-3)
    print("# product rate: ed_msm_device of 2^20 points, %d windows, %d products per addition, accumulation kernel %.3f ms: %.1f G products/s" % (windows, eng.accumulate_products(), ms, rate / 1e9), flush=True)
    print("RATE %r" % rate, flush=True)
    eng.close()


def line(index, rate, args):
    name, logn, k, c, bits = LINES[index]
    b = Bench(g1=True)
    eng, rows = b.eng, 1 << logn
    s = b.d_s if bits == 256 else b.d_s64
    eng.ed_set_generators(b.gens[: 64 * k], c)
    eng.set_generators(b.g1_gens[: 96 * k], c)
    with_b = k <= B_MAX_K
    a_rows = min(rows, A_ROWS)
    # bytes first: each way's records against the call's
    b.commit(s, rows, k)
    mine = b.records(rows)
    same_a = b.way_a(s, a_rows, k) == mine[: 64 * a_rows]
    same_b = None
    if with_b:
        eng.set_mul_window(8)
        b.way_b(s, rows, k)
        same_b = bytes(b.d_b[: 64 * rows].cpu().numpy().tobytes()) == mine
    calls = [lambda: b.commit(s, rows, k), lambda: b.way_a(s, a_rows, k), lambda: b.g1_commit(s, rows, k)]
    if with_b:
        calls.append(lambda: b.way_b(s, rows, k))
    series = alternate(calls, args.repeats, args.warmup)
    eng.set_mul_window(0)
    scale = rows / a_rows
    windows = -(-bits // c) + 1
    floor = rows * k * windows * MADD_PRODUCTS / rate * 1e3
    new, a, g1 = series[0], series[1], series[2]
    m = statistics.median(new)
    best, verdict, which = statistics.median(a) * scale, faster(new, a, scale), "A"
    text = "%-10s 2^%-2d x %-4d c = %-2d | call %s | A %s%s, bytes equal: %s" % (name, logn, k, c, fmt(new), fmt(a, scale), " (scaled from %d rows)" % a_rows if scale != 1 else "", same_a)
    if with_b:
        text += " | B %s, bytes equal: %s" % (fmt(series[3]), same_b)
        if statistics.median(series[3]) < best:
            best, verdict, which = statistics.median(series[3]), faster(new, series[3]), "B"
    else:
        text += " | B not run (k > %d)" % B_MAX_K
    text += " | call / best (%s) = %.3f: %s | G1 commit_rows %s, ed / G1 = %.3f | floor %.3f, call / floor = %.2f" % (which, m / best, verdict, fmt(g1), m / statistics.median(g1), floor, m / floor)
    print(text, flush=True)
    eng.ed_set_generators(None)
    eng.set_generators(None)
    eng.close()


def cold(args):
    b = Bench()
    for k, c in COLD:
        print("cold ed_set_generators k = %-4d c = %-2d: %.1f ms (median of 3)" % (k, c, b.cold_set(k, c)), flush=True)
    b.eng.ed_set_generators(None)
    b.eng.close()


def crossover(args):
    b = Bench()
    print("# the crossover: k = 4 096, c = 8, full-width, few rows; A in full", flush=True)
    b.eng.ed_set_generators(b.gens, 8)
    for rows in (1, 4, 16, 64, 256):
        new, a = alternate([lambda: b.commit(b.d_s, rows, KMAX), lambda: b.way_a(b.d_s, rows, KMAX)], args.repeats, args.warmup)
        print("rows = %-3d k = 4096 | call %s | A %s | call / A = %.3f: %s" % (rows, fmt(new), fmt(a), statistics.median(new) / statistics.median(a), faster(new, a)), flush=True)
    b.eng.ed_set_generators(None)
    b.eng.close()


def sweep(args):
    import webgpu_msm_bls12_377_amd as msm

    print("# %s; ms per call, median [q1..q3] of %d calls after %d warm-up calls, the ways alternating call by call; inputs and outputs resident" % (
        msm.load_library().msm377_version().decode(), args.repeats, args.warmup))
    print("# call: ed_commit_rows_device on a resident set; A: one ed_msm_device per row; B: ceil(k / 16) ed_batch_mul_multi_device (c = 8, slots rebuilt) + ed_batch_lincomb2_device(a = b = 1)")
    print("# floor = rows x k x (W + 1) additions of %d field products at the session's product rate; verdicts compare medians against the quartile spread of the two series" % MADD_PRODUCTS, flush=True)
    common = [sys.executable, os.path.abspath(__file__), "--repeats", str(args.repeats), "--warmup", str(args.warmup)]

    def step(*extra):
        res = subprocess.run(common + list(extra), timeout=STEP_SECONDS, capture_output=True, text=True)
        lines = res.stdout.splitlines()
        for text in lines:
            if not text.startswith("RATE "):
                print(text, flush=True)
        if res.returncode:
            sys.stderr.write(res.stderr[-2000:])
            raise SystemExit("step %s ended with %d: the sweep stops here" % (extra, res.returncode))
        return lines

    rate = float([t for t in step("--step", "rate") if t.startswith("RATE ")][0].split()[1])
    for i in range(len(LINES)):
        step("--step", "line", "--index", str(i), "--rate", repr(rate))
    step("--step", "cold")
    step("--step", "crossover")


def trace_case():
    b = Bench()
    for logn, k in ((10, 1024), (8, 4096)):
        b.eng.ed_set_generators(b.gens[: 64 * k], 8)
        for _ in range(6):
            b.commit(b.d_s, 1 << logn, k)
    b.eng.ed_set_generators(None)
    b.eng.close()


def report_trace(folder):
    files = glob.glob(os.path.join(folder, "**", "*kernel_trace.csv"), recursive=True)
    rows = [r for f in files for r in csv.DictReader(open(f)) if "k_edbm" in r["Kernel_Name"] or "k_edcr" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    for r in rows:
        r["name"] = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").replace("msm377::", "").split("(")[0][:60]
        r["grid"] = "%s x %s" % (r.get("Grid_Size_X", r.get("Grid_Size", "?")), r.get("Grid_Size_Y", "1"))
    starts = [i for i, r in enumerate(rows) if r["name"].startswith("k_edcr_accumulate")]
    calls = [rows[a:z] for a, z in zip(starts, starts[1:] + [len(rows)])]
    assert len(calls) == 12, "the trace case makes six calls of each of two shapes, found %d" % len(calls)
    for shape, group in (("2^10 rows x 1 024 generators", calls[:6]), ("2^8 rows x 4 096 generators", calls[6:])):
        mine = group[1:]  # the first call of a shape is its warm-up
        print("# warm ed_commit_rows_device calls, %s, c = 8, full-width scalars: the launches of one call, medians over %d calls; us under rocprofv3 --kernel-trace" % (shape, len(mine)))
        per = {}
        for c in mine:
            for pos, r in enumerate(c):
                if r["name"].startswith(("k_edbm_row", "k_edbm_entries")):
                    break  # the next set's build
                per.setdefault((pos, r["name"], r["grid"]), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
        total = 0.0
        for (pos, name, grid), ds in sorted(per.items()):
            if len(ds) < len(mine):
                continue
            total += statistics.median(ds)
            print("  %2d  %-24s grid %-16s %9.1f" % (pos, name, grid, statistics.median(ds)))
        print("  sum of the medians %9.1f" % total)


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "report-trace":
        report_trace(sys.argv[2])
        return
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--trace-case", action="store_true")
    ap.add_argument("--step", choices=["rate", "line", "cold", "crossover"])
    ap.add_argument("--index", type=int, default=0)
    ap.add_argument("--rate", type=float, default=0.0)
    args = ap.parse_args()
    if args.trace_case:
        trace_case()
    elif args.step == "rate":
        product_rate()
    elif args.step == "line":
        line(args.index, args.rate, args)
    elif args.step == "cold":
        cold(args)
    elif args.step == "crossover":
        crossover(args)
    else:
        sweep(args)


if __name__ == "__main__":
    main()
