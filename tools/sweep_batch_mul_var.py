#!/usr/bin/env python3
"""Variable-base batch multiplication (msm377_g1_batch_mul_var_device), inputs and outputs resident.

Every size alternates, call by call in one process after a warm-up of both,
       A = msm377_g1_check_points_device(points, n, CHECK_SUBGROUP)   the parent's only per-point chain of this length
       B = msm377_g1_batch_mul_var_device(points, scalars, n)
on the same points ([a_i]G of generate_bases_device).  Full-width uniform scalars at 2^12, 2^16, 2^17, 2^20; 64-bit
scalars and one scalar for all points (stride 0) at 2^20.

Floor model, products counted from the code:
       check chain   252 doublings x 9 + 68 additions x 10                        = 2 948 field products per point
       walk          64 windows x (4 doublings x 9 + 1 addition x 10)             = 2 944 per output (k_bmv_accumulate)
       all of B      the walk + the table (1 doubling of 8, 6 additions of 10, 4 conversions) + the normalisation of the
                     8 table entries and the output (8 products each)              ~ 3 090 per output
at the product rate the bucket accumulation reaches, 10.2 G seven-product additions per second, and
beside it the rate the fixed-base call (k_bm_accumulate, width 16, warm table, 2^20 full-width scalars) reaches in this
very session.  Target of the feature: B <= A x (2 944 / 2 948) x 1.25 at 2^20 full-width.

    python tools/sweep_batch_mul_var.py [--repeats 30] [--warmup 5] > profiles/batch_mul_var/sweep.txt
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import webgpu_msm_bls12_377_amd as msm  # noqa: E402

GX = 81937999373150964239938255573465948239988671502647976594219695644855304257327692006745978603320413799295628339695
GY = 241266749859715473739788878240585681733927191168601896383759122102112907357779751001206799952863815012735208165030
PRODUCT_RATE = 10.2e9 * 7  # field products per second of k_accumulate
CHECK_PRODUCTS = 252 * 9 + 68 * 10
WALK_PRODUCTS = 64 * (4 * 9 + 10)
CALL_PRODUCTS = WALK_PRODUCTS + (8 + 6 * 10 + 4) + 9 * 8
TARGET_SLACK = 1.25


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="12,16,17,20")
    args = ap.parse_args()
    sizes = [1 << int(s) for s in args.sizes.split(",")]
    cap = max(sizes + [1 << 20])
    eng = msm.MsmEngine(cap, device=0)
    d_pts = torch.empty(96 * cap, dtype=torch.uint8, device="cuda")
    d_out = torch.empty(96 * cap, dtype=torch.uint8, device="cuda")
    d_inf = torch.empty(cap, dtype=torch.uint8, device="cuda")
    eng.generate_bases_device(0x377, cap, d_pts.data_ptr())
    gen = torch.Generator().manual_seed(0xBA7C5)
    d_full = torch.randint(0, 256, (cap, 32), dtype=torch.uint8, generator=gen).cuda()
    d_short = d_full.clone()
    d_short[:, 8:] = 0
    print("# %s; ms per call, median [q1..q3] (min..max) of %d calls after %d warm-up calls; inputs and outputs resident" % (msm.load_library().msm377_version().decode(), args.repeats, args.warmup))
    print("# products per point: check chain %d, walk %d, whole var call ~%d; floor = products x n at %.1f G products/s" % (CHECK_PRODUCTS, WALK_PRODUCTS, CALL_PRODUCTS, PRODUCT_RATE / 1e9))

    # the fixed-base call's rate in this session
    n = 1 << 20
    g_bytes = GX.to_bytes(48, "little") + GY.to_bytes(48, "little")
    eng.set_mul_window(16)
    fixed = lambda: eng.batch_mul_device(g_bytes, d_full.data_ptr(), n, d_out.data_ptr(), d_inf.data_ptr())  # noqa: E731
    for _ in range(args.warmup):
        fixed()
    ts = []
    for _ in range(args.repeats):
        t0 = time.perf_counter()
        fixed()
        ts.append((time.perf_counter() - t0) * 1e3)
    eng.set_mul_window(0)
    m = statistics.median(ts)
    print("fixed-base batch_mul, width 16, n = 2^20 | %s | 17 additions x 10 products: %.1f G products/s over the whole call" % (fmt(ts), 170 * n / m / 1e6), flush=True)

    print("# A = check_points_device(CHECK_SUBGROUP), B = batch_mul_var_device, alternating, same points")
    cases = [("full-width", d_full, 32, s) for s in sizes] + [("64-bit", d_short, 32, 1 << 20), ("stride 0, full-width", d_full, 0, 1 << 20)]
    for name, d_s, stride, n in cases:
        call_a = lambda: eng.check_points_device(d_pts.data_ptr(), n, msm.CHECK_SUBGROUP)  # noqa: E731
        call_b = lambda: eng.batch_mul_var_device(d_pts.data_ptr(), d_s.data_ptr(), n, d_out.data_ptr(), d_inf.data_ptr(), "wire", stride)  # noqa: E731
        ta, tb = alternate(call_a, call_b, args.repeats, args.warmup)
        ma, mb = statistics.median(ta), statistics.median(tb)
        floor_walk, floor_call = WALK_PRODUCTS * n / PRODUCT_RATE * 1e3, CALL_PRODUCTS * n / PRODUCT_RATE * 1e3
        line = "%-20s n = 2^%-2d | A %s | B %s | B / A = %.3f | %.2f M outputs/s | B / floor: walk %.2f, whole call %.2f" % (
            name, n.bit_length() - 1, fmt(ta), fmt(tb), mb / ma, n / mb / 1e3, mb / floor_walk, mb / floor_call)
        if name == "full-width" and n == 1 << 20:
            target = ma * WALK_PRODUCTS / CHECK_PRODUCTS * TARGET_SLACK
            line += " | target A x %d / %d x %.2f = %.3f ms: %s" % (WALK_PRODUCTS, CHECK_PRODUCTS, TARGET_SLACK, target, "met" if mb <= target else "MISSED")
        print(line, flush=True)
    eng.close()


if __name__ == "__main__":
    main()
