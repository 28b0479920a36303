#!/usr/bin/env python3
"""Edwards-BLS12 variable-base batch multiplication (msm377_ed_batch_mul_var_device), inputs and outputs resident.

Every shape alternates, call by call in one process after a warm-up of both,
       A = a yardstick on the same n
       B = msm377_ed_batch_mul_var_device(points, scalars, n)
on the points of ed_generate_bases_device.  Full-width uniform scalars at 2^12, 2^16, 2^17, 2^20; 64-bit scalars and one
scalar for all points (stride 0) at 2^20.  Yardsticks:
  (1) msm377_ed_check_points_device(CHECK_SUBGROUP): the only other per-point chain of this length on this curve, the NAF
      of the subgroup order on the canonical Ed:: formulas -- (len - 1) doublings of 8 products and one 7-product addition
      per non-zero digit, counted here from the order itself.  Target: B <= A x (walk products / chain products) x 1.25 at
      2^20 full-width.
  (2) msm377_g1_batch_mul_var_device at the same n: the ratio beside the limb-mad model's 0.34 (81 x 2 304 limb products
      against 169 x 2 944) and the 0.39 - 0.42 the fixed-base call found.
  (3) the floor: 2 304 products per output at the product rate k_accumulate<EdDev> reaches in an msm377_ed_msm_device of
      2^20 points in this session (its accumulation kernel under msm377_ctx_set_timing(2); 16 windows x n additions of
      msm377_ctx_get_products_per_addition products).
--walk-only prints B alone at 2^17 and 2^20: one side of a build-time A/B (MSM377_LIB selects the build).

    python tools/sweep_ed_batch_mul_var.py [--repeats 30] [--warmup 5] > profiles/ed_batch_mul_var/sweep.txt
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

ED_SUBGROUP = 2111115437357092606062206234695386632838870926408408195193685246394721360383
WALK_PRODUCTS = 64 * (3 * 7 + 8 + 7)
CALL_PRODUCTS = WALK_PRODUCTS + 60 + 70  # the table (3 conversions, 1 doubling of 8, 6 additions of 7, make_base) and two normalisations
G1_WALK_PRODUCTS = 64 * (4 * 9 + 10)
TARGET_SLACK = 1.25


def naf(v):
    digits = []
    while v:
        d = (2 - v % 4) if v & 1 else 0
        digits.append(d)
        v = (v - d) // 2
    return digits


CHAIN = naf(ED_SUBGROUP)
CHECK_PRODUCTS = 8 * (len(CHAIN) - 1) + 7 * sum(1 for d in CHAIN if d)


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
    ap.add_argument("--walk-only", action="store_true")
    args = ap.parse_args()
    sizes = [1 << int(s) for s in args.sizes.split(",")]
    cap = 1 << 20
    eng = msm.MsmEngine(cap, device=0)
    d_pts = torch.empty(64 * cap, dtype=torch.uint8, device="cuda")
    d_out = torch.empty(64 * cap, dtype=torch.uint8, device="cuda")
    eng.ed_generate_bases_device(0x377ED, cap, d_pts.data_ptr())
    gen = torch.Generator().manual_seed(0xBA7C5)
    d_full = torch.randint(0, 256, (cap, 32), dtype=torch.uint8, generator=gen).cuda()
    d_short = d_full.clone()
    d_short[:, 8:] = 0
    var = lambda d_s, n, stride=32: eng.ed_batch_mul_var_device(d_pts.data_ptr(), d_s.data_ptr(), n, d_out.data_ptr(), stride)  # noqa: E731
    version = msm.load_library().msm377_version().decode()
    if args.walk_only:
        for n in (1 << 17, 1 << 20):
            for _ in range(args.warmup):
                var(d_full, n)
            ts = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                var(d_full, n)
                ts.append((time.perf_counter() - t0) * 1e3)
            print("%s | ed_batch_mul_var_device full-width n = 2^%d | %s" % (os.environ.get("MSM377_LIB", "csrc/libmsm377.so"), n.bit_length() - 1, fmt(ts)), flush=True)
        eng.close()
        return
    print("# %s; ms per call, median [q1..q3] (min..max) of %d calls after %d warm-up calls; inputs and outputs resident" % (version, args.repeats, args.warmup))
    print("# products per point: check chain %d (%d doublings x 8, %d additions x 7), walk %d, whole call ~%d" % (
        CHECK_PRODUCTS, len(CHAIN) - 1, sum(1 for d in CHAIN if d), WALK_PRODUCTS, CALL_PRODUCTS))

    # (3) the product rate of the Edwards-BLS12 bucket accumulation in this session
    n = 1 << 20
    d_msm = d_full.clone()
    d_msm[:, 31] &= 0x0F  # below 2^252: no rerun
    eng.set_timing(2)
    acc = []
    for i in range(args.warmup + args.repeats):
        eng.ed_msm_device(d_pts.data_ptr(), d_msm.data_ptr(), n)
        if i >= args.warmup:
            acc.append(eng.stage_ms()["accumulate_kernel"])
    eng.set_timing(0)
    per_add = eng.accumulate_products()
    rate = 16 * n * per_add / statistics.median(acc) * 1e3
    print("ed_msm_device n = 2^20, accumulation kernel | %s | 16 x n additions x %d products: %.1f G products/s" % (fmt(acc), per_add, rate / 1e9), flush=True)

    d_g1 = torch.empty(96 * cap, dtype=torch.uint8, device="cuda")
    d_g1_out = torch.empty(96 * cap, dtype=torch.uint8, device="cuda")
    d_inf = torch.empty(cap, dtype=torch.uint8, device="cuda")
    eng.generate_bases_device(0x377, cap, d_g1.data_ptr())
    cases = [("full-width", d_full, 32, s) for s in sizes] + [("64-bit", d_short, 32, 1 << 20), ("stride 0, full-width", d_full, 0, 1 << 20)]
    print("# (1) A = ed_check_points_device(CHECK_SUBGROUP), B = ed_batch_mul_var_device, alternating, same points; (3) floor at the rate above")
    for name, d_s, stride, n in cases:
        call_a = lambda: eng.ed_check_points_device(d_pts.data_ptr(), n, msm.CHECK_SUBGROUP)  # noqa: E731
        ta, tb = alternate(call_a, lambda: var(d_s, n, stride), args.repeats, args.warmup)
        ma, mb = statistics.median(ta), statistics.median(tb)
        floor_walk, floor_call = WALK_PRODUCTS * n / rate * 1e3, CALL_PRODUCTS * n / rate * 1e3
        line = "%-20s n = 2^%-2d | A %s | B %s | B / A = %.3f | %.2f M outputs/s | B / floor: walk %.2f, whole call %.2f" % (
            name, n.bit_length() - 1, fmt(ta), fmt(tb), mb / ma, n / mb / 1e3, mb / floor_walk, mb / floor_call)
        if name == "full-width" and n == 1 << 20:
            target = ma * WALK_PRODUCTS / CHECK_PRODUCTS * TARGET_SLACK
            line += " | target A x %d / %d x %.2f = %.3f ms: %s" % (WALK_PRODUCTS, CHECK_PRODUCTS, TARGET_SLACK, target, "met" if mb <= target else "MISSED")
        print(line, flush=True)
    print("# (2) A = g1 batch_mul_var_device, B = ed_batch_mul_var_device, alternating, same n and scalars; limb-mad model %.2f" % (81 * WALK_PRODUCTS / (169 * G1_WALK_PRODUCTS)))
    for name, d_s, stride, n in cases:
        call_a = lambda: eng.batch_mul_var_device(d_g1.data_ptr(), d_s.data_ptr(), n, d_g1_out.data_ptr(), d_inf.data_ptr(), "wire", stride)  # noqa: E731
        ta, tb = alternate(call_a, lambda: var(d_s, n, stride), args.repeats, args.warmup)
        print("%-20s n = 2^%-2d | A %s | B %s | B / A = %.3f" % (name, n.bit_length() - 1, fmt(ta), fmt(tb), statistics.median(tb) / statistics.median(ta)), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
