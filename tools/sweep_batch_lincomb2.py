#!/usr/bin/env python3
"""Pairwise linear combination (msm377_g1_batch_lincomb2_device), inputs and outputs resident.

Every case alternates, call by call in one process after a warm-up of both,
       A = msm377_g1_batch_mul_var_device(P, a, n) then msm377_g1_batch_mul_var_device(Q, b, n)   the two halves, the only
           way to them without this call (and the sum of the two is still missing)
       B = msm377_g1_batch_lincomb2_device(P, Q, a, b, n)
on the same points ([k_i]G of generate_bases_device; Q is P moved by 977 records).  Full-width uniform scalars at 2^12,
2^16, 2^17, 2^20; at 2^20 also 128-bit scalars, one scalar each for all pairs (strides 0, 0: the fold) and a = b = 1 (the
addition).

Floor model, products counted from the code:
       two walks     2 x 64 windows x (4 doublings x 9 + 1 addition x 10)          = 5 888 field products per output
       joint walk    64 windows x (4 doublings x 9 + 2 additions x 10)             = 3 584 per output (k_bl2_accumulate)
       all of B      the joint walk + two tables (1 doubling of 8, 6 additions of 10, 4 conversions each) + the
                     normalisation of the 16 table entries and the output (8 products each)   ~ 3 864 per output
at the product rate the bucket accumulation reaches, 10.2 G seven-product additions per second.
Target of the feature: B <= 0.75 x A at 2^20 full-width, A measured in the same run.

    python tools/sweep_batch_lincomb2.py [--repeats 30] [--warmup 5] > profiles/batch_lincomb2/sweep.txt
    python tools/sweep_batch_lincomb2.py --trace-case   # six calls of B at 2^20 full-width alone: the program of a kernel trace
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

PRODUCT_RATE = 10.2e9 * 7  # field products per second of k_accumulate
TWO_WALKS = 2 * 64 * (4 * 9 + 10)
JOINT_WALK = 64 * (4 * 9 + 2 * 10)
CALL_PRODUCTS = JOINT_WALK + 2 * (8 + 6 * 10 + 4) + 17 * 8
TARGET = 0.75
SHIFT = 977  # Q_i = P_(i + SHIFT)


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
    ap.add_argument("--trace-case", action="store_true")
    args = ap.parse_args()
    sizes = [1 << int(s) for s in args.sizes.split(",")]
    cap = max(sizes + [1 << 20])
    eng = msm.MsmEngine(cap, device=0)
    d_pts = torch.empty(96 * (cap + SHIFT), dtype=torch.uint8, device="cuda")
    d_out = torch.empty(96 * cap, dtype=torch.uint8, device="cuda")
    d_out2 = torch.empty(96 * cap, dtype=torch.uint8, device="cuda")
    d_inf = torch.empty(cap, dtype=torch.uint8, device="cuda")
    eng.generate_bases_device(0x377, cap + SHIFT, d_pts.data_ptr())
    p, q = d_pts.data_ptr(), d_pts.data_ptr() + 96 * SHIFT
    gen = torch.Generator().manual_seed(0xBA7C6)
    d_a = torch.randint(0, 256, (cap, 32), dtype=torch.uint8, generator=gen).cuda()
    d_b = torch.randint(0, 256, (cap, 32), dtype=torch.uint8, generator=gen).cuda()
    d_a128, d_b128 = d_a.clone(), d_b.clone()
    d_a128[:, 16:] = 0
    d_b128[:, 16:] = 0
    d_one = torch.zeros(32, dtype=torch.uint8, device="cuda")
    d_one[0] = 1
    if args.trace_case:
        n = 1 << 20
        for _ in range(6):
            eng.batch_lincomb2_device(p, q, d_a.data_ptr(), d_b.data_ptr(), n, d_out.data_ptr(), d_inf.data_ptr())
        eng.close()
        return
    print("# %s; ms per call, median [q1..q3] (min..max) of %d calls after %d warm-up calls; inputs and outputs resident" % (msm.load_library().msm377_version().decode(), args.repeats, args.warmup))
    print("# products per output: two walks %d, joint walk %d, whole lincomb2 call ~%d; floor = products x n at %.1f G products/s" % (TWO_WALKS, JOINT_WALK, CALL_PRODUCTS, PRODUCT_RATE / 1e9))
    print("# A = batch_mul_var_device(P, a) + batch_mul_var_device(Q, b), B = batch_lincomb2_device(P, Q, a, b), alternating, same inputs")
    big = 1 << 20
    cases = [("full-width", d_a, d_b, 32, s) for s in sizes]
    cases += [("128-bit", d_a128, d_b128, 32, big), ("strides 0, 0 (fold)", d_a, d_b, 0, big), ("a = b = 1 (addition)", d_one, d_one, 0, big)]
    for name, sa, sb, stride, n in cases:
        def call_a():
            eng.batch_mul_var_device(p, sa.data_ptr(), n, d_out.data_ptr(), d_inf.data_ptr(), "wire", stride)
            eng.batch_mul_var_device(q, sb.data_ptr(), n, d_out2.data_ptr(), d_inf.data_ptr(), "wire", stride)

        def call_b():
            eng.batch_lincomb2_device(p, q, sa.data_ptr(), sb.data_ptr(), n, d_out.data_ptr(), d_inf.data_ptr(), "wire", stride, stride)

        ta, tb = alternate(call_a, call_b, args.repeats, args.warmup)
        ma, mb = statistics.median(ta), statistics.median(tb)
        floor_walk, floor_call = JOINT_WALK * n / PRODUCT_RATE * 1e3, CALL_PRODUCTS * n / PRODUCT_RATE * 1e3
        line = "%-20s n = 2^%-2d | A %s | B %s | B / A = %.3f | %.2f M outputs/s | B / floor: walk %.2f, whole call %.2f" % (
            name, n.bit_length() - 1, fmt(ta), fmt(tb), mb / ma, n / mb / 1e3, mb / floor_walk, mb / floor_call)
        if name == "full-width" and n == big:
            line += " | target B <= %.2f x A = %.3f ms: %s" % (TARGET, TARGET * ma, "met" if mb <= TARGET * ma else "MISSED")
        print(line, flush=True)
    eng.close()


if __name__ == "__main__":
    main()
