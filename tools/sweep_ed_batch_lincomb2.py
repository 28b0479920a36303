#!/usr/bin/env python3
"""Edwards-BLS12 pairwise linear combination (msm377_ed_batch_lincomb2_device), inputs and outputs resident.

Every shape alternates, call by call in one process after a warm-up of both,
       A = a yardstick on the same n
       B = msm377_ed_batch_lincomb2_device(p, q, a, b, n)
on the points of ed_generate_bases_device.  Full-width uniform scalars at 2^12, 2^16, 2^17, 2^20; at 2^20 also 64-bit and
128-bit scalars, one scalar each for all pairs (strides 0), a = b = 1 (the addition alone) and the Schnorr shape (p_stride 0).
Yardsticks:
  (1) the two msm377_ed_batch_mul_var_device calls (P, a) and (Q, b) on the same inputs: the most the library offered before
      this call, and it still lacks the addition.  Target: B / A <= 0.75 at 2^20 full-width (product counts: 2 752 / 4 608 =
      0.597).
  (2) msm377_g1_batch_lincomb2_device at the same n: the ratio beside the limb-mad model's 0.34 (81 x 2 752 limb products
      against 169 x 3 584).
  (3) the floor: 2 752 products per output at the product rate k_accumulate<EdDev> reaches in an msm377_ed_msm_device of
      2^20 points in this session (its accumulation kernel under msm377_ctx_set_timing(2); 16 windows x n additions of
      msm377_ctx_get_products_per_addition products).

    python tools/sweep_ed_batch_lincomb2.py [--repeats 30] [--warmup 5] > profiles/ed_batch_lincomb2/sweep.txt
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

WALK_PRODUCTS = 64 * (3 * 7 + 8 + 2 * 7)
VAR_WALK_PRODUCTS = 64 * (3 * 7 + 8 + 7)
G1_WALK_PRODUCTS = 64 * (4 * 9 + 2 * 10)
TARGET = 0.75


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
    ap.add_argument("--skip-g1", action="store_true")
    args = ap.parse_args()
    sizes = [1 << int(s) for s in args.sizes.split(",")]
    cap = 1 << 20
    eng = msm.MsmEngine(cap, device=0)
    d_p = torch.empty(64 * cap, dtype=torch.uint8, device="cuda")
    d_q = torch.empty(64 * cap, dtype=torch.uint8, device="cuda")
    d_out = torch.empty(64 * cap, dtype=torch.uint8, device="cuda")
    eng.ed_generate_bases_device(0x377ED, cap, d_p.data_ptr())
    eng.ed_generate_bases_device(0x377EE, cap, d_q.data_ptr())
    gen = torch.Generator().manual_seed(0xBA7C5)
    d_a = torch.randint(0, 256, (cap, 32), dtype=torch.uint8, generator=gen).cuda()
    d_b = torch.randint(0, 256, (cap, 32), dtype=torch.uint8, generator=gen).cuda()

    def cut(d_s, nbytes):
        out = d_s.clone()
        out[:, nbytes:] = 0
        return out

    d_one = torch.zeros(32, dtype=torch.uint8, device="cuda")
    d_one[0] = 1
    ptr = lambda t: t.data_ptr()  # noqa: E731

    def l2(n, a, b, strides=(64, 64, 32, 32)):
        eng.ed_batch_lincomb2_device(ptr(d_p), ptr(d_q), ptr(a), ptr(b), n, ptr(d_out), *strides)

    def two_var(n, a, b, strides=(64, 64, 32, 32)):  # p_stride 0 has no counterpart: the yardstick multiplies n copies' worth
        eng.ed_batch_mul_var_device(ptr(d_p), ptr(a), n, ptr(d_out), strides[2])
        eng.ed_batch_mul_var_device(ptr(d_q), ptr(b), n, ptr(d_out), strides[3])

    version = msm.load_library().msm377_version().decode()
    print("# %s; ms per call, median [q1..q3] (min..max) of %d calls after %d warm-up calls; inputs and outputs resident" % (version, args.repeats, args.warmup))
    print("# products per output: joint walk %d, two variable-base walks %d (ratio %.3f)" % (WALK_PRODUCTS, 2 * VAR_WALK_PRODUCTS, WALK_PRODUCTS / (2 * VAR_WALK_PRODUCTS)))

    # (3) the product rate of the Edwards-BLS12 bucket accumulation in this session
    n = 1 << 20
    d_msm = d_a.clone()
    d_msm[:, 31] &= 0x0F  # below 2^252: no rerun
    eng.set_timing(2)
    acc = []
    for i in range(args.warmup + args.repeats):
        eng.ed_msm_device(ptr(d_p), ptr(d_msm), n)
        if i >= args.warmup:
            acc.append(eng.stage_ms()["accumulate_kernel"])
    eng.set_timing(0)
    per_add = eng.accumulate_products()
    rate = 16 * n * per_add / statistics.median(acc) * 1e3
    print("ed_msm_device n = 2^20, accumulation kernel | %s | 16 x n additions x %d products: %.1f G products/s" % (fmt(acc), per_add, rate / 1e9), flush=True)

    big = 1 << 20
    cases = [("full-width", d_a, d_b, (64, 64, 32, 32), s) for s in sizes] + [
        ("64-bit", cut(d_a, 8), cut(d_b, 8), (64, 64, 32, 32), big),
        ("128-bit", cut(d_a, 16), cut(d_b, 16), (64, 64, 32, 32), big),
        ("one scalar each", d_a, d_b, (64, 64, 0, 0), big),
        ("a = b = 1", d_one, d_one, (64, 64, 0, 0), big),
        ("Schnorr (p_stride 0)", d_a, d_b, (0, 64, 32, 32), big),
    ]
    print("# (1) A = ed_batch_mul_var_device(P, a) + ed_batch_mul_var_device(Q, b), B = ed_batch_lincomb2_device, alternating, same inputs; (3) floor at the rate above")
    for name, a, b, strides, n in cases:
        ta, tb = alternate(lambda: two_var(n, a, b, strides), lambda: l2(n, a, b, strides), args.repeats, args.warmup)
        ma, mb = statistics.median(ta), statistics.median(tb)
        line = "%-20s n = 2^%-2d | A %s | B %s | B / A = %.3f | %.2f M outputs/s | B / floor %.2f" % (
            name, n.bit_length() - 1, fmt(ta), fmt(tb), mb / ma, n / mb / 1e3, mb / (WALK_PRODUCTS * n / rate * 1e3))
        if name == "full-width" and n == big:
            line += " | target B / A <= %.2f: %s" % (TARGET, "met" if mb / ma <= TARGET else "MISSED by %.3f" % (mb / ma - TARGET))
        print(line, flush=True)
    if not args.skip_g1:
        d_g1p = torch.empty(96 * cap, dtype=torch.uint8, device="cuda")
        d_g1q = torch.empty(96 * cap, dtype=torch.uint8, device="cuda")
        d_g1_out = torch.empty(96 * cap, dtype=torch.uint8, device="cuda")
        d_inf = torch.empty(cap, dtype=torch.uint8, device="cuda")
        eng.generate_bases_device(0x377, cap, ptr(d_g1p))
        eng.generate_bases_device(0x378, cap, ptr(d_g1q))
        print("# (2) A = g1 batch_lincomb2_device, B = ed_batch_lincomb2_device, alternating, same n and scalars; limb-mad model %.2f" % (81 * WALK_PRODUCTS / (169 * G1_WALK_PRODUCTS)))
        for name, a, b, strides, n in cases:
            if strides[0] == 0:
                continue  # the G1 call has no point strides
            call_a = lambda: eng.batch_lincomb2_device(ptr(d_g1p), ptr(d_g1q), ptr(a), ptr(b), n, ptr(d_g1_out), ptr(d_inf), "wire", strides[2], strides[3])  # noqa: E731
            ta, tb = alternate(call_a, lambda: l2(n, a, b, strides), args.repeats, args.warmup)
            print("%-20s n = 2^%-2d | A %s | B %s | B / A = %.3f" % (name, n.bit_length() - 1, fmt(ta), fmt(tb), statistics.median(tb) / statistics.median(ta)), flush=True)
    eng.close()


if __name__ == "__main__":
    main()
