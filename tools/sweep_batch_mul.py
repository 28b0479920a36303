#!/usr/bin/env python3
"""Fixed-base batch multiplication (msm377_g1_batch_mul_device), inputs and outputs resident.

1. Against the only other route to many points: [a_i]G for the 64-bit SplitMix scalars of a seed, n = 2^20.
       A = msm377_g1_generate_bases_device(seed, n)
       B = msm377_g1_batch_mul_device(G, a, n) with a warm table, a_i zero-extended to 32 bytes
   alternating call by call in one process after a warm-up of both; the bytes are compared once (they must be identical).
2. Full-width uniform scalars, n = 2^12, 2^16, 2^20, each supported width: the warm call (median of REPEATS) and the
   table build = a cold call (n = 1 on a base the context has not seen: the build plus a one-output call) minus the warm
   n = 1 call, both printed.
   Beside the 2^20 line the derived floor: (W + 1) n mixed additions of 10 field products at the product rate the bucket
   accumulation reaches, 10.2 G seven-product additions per second.

    python tools/sweep_batch_mul.py [--repeats 30] [--warmup 5] > profiles/batch_mul/sweep.txt
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import webgpu_msm_bls12_377_amd as msm  # noqa: E402

WIDTHS = (8, 16)
# the generator of BLS12-377 G1 (the base generate_bases_device multiplies)
GX = 81937999373150964239938255573465948239988671502647976594219695644855304257327692006745978603320413799295628339695
GY = 241266749859715473739788878240585681733927191168601896383759122102112907357779751001206799952863815012735208165030
PRODUCT_RATE = 10.2e9 * 7  # field products per second of k_accumulate
MADD_PRODUCTS = 10         # XYZZ mixed addition: 8M + 2S


def quartiles(xs):
    q = statistics.quantiles(xs, n=4)
    return q[0], q[2]


def fmt(ts):
    q1, q3 = quartiles(ts)
    return "%.3f [%.3f..%.3f] (%.3f..%.3f)" % (statistics.median(ts), q1, q3, min(ts), max(ts))


def splitmix_scalars(seed, n):
    """a_i = the (i + 1)-th SplitMix64(seed) output, 0 mapped to 1, as n x 32 little-endian bytes."""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (np.arange(1, n + 1, dtype=np.uint64)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
    z[z == 0] = 1
    out = np.zeros((n, 4), dtype="<u8")
    out[:, 0] = z
    return out.tobytes()


def timed(call, repeats, warmup):
    for _ in range(warmup):
        call()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        call()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--sizes", default="12,16,20")
    ap.add_argument("--cold", type=int, default=7, help="cold calls (fresh bases) per width")
    args = ap.parse_args()
    sizes = [1 << int(s) for s in args.sizes.split(",")]
    cap = max(sizes + [1 << 20])
    eng = msm.MsmEngine(cap, device=0)
    d_pts = torch.empty(96 * cap, dtype=torch.uint8, device="cuda")
    d_out = torch.empty(96 * cap, dtype=torch.uint8, device="cuda")
    d_inf = torch.empty(cap, dtype=torch.uint8, device="cuda")
    g_bytes = GX.to_bytes(48, "little") + GY.to_bytes(48, "little")
    print("# %s; ms per call, median [q1..q3] (min..max) of %d calls after %d warm-up calls; inputs and outputs resident" % (msm.load_library().msm377_version().decode(), args.repeats, args.warmup))

    # ---- 1. against generate_bases_device ----
    n, seed = 1 << 20, 0x377
    d_a = torch.frombuffer(bytearray(splitmix_scalars(seed, n)), dtype=torch.uint8).cuda()
    print("# 1. [a_i]G, 64-bit SplitMix a_i, n = 2^20: A = generate_bases_device, B = batch_mul_device (warm table), alternating")
    for c in WIDTHS + (0,):
        eng.set_mul_window(c)
        call_a = lambda: eng.generate_bases_device(seed, n, d_pts.data_ptr())  # noqa: E731
        call_b = lambda: eng.batch_mul_device(g_bytes, d_a.data_ptr(), n, d_out.data_ptr(), d_inf.data_ptr())  # noqa: E731
        for _ in range(args.warmup):
            call_a()
            call_b()
        assert torch.equal(d_pts[: 96 * n], d_out[: 96 * n]), "the two routes disagree"
        ta, tb = [], []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            call_a()
            t1 = time.perf_counter()
            call_b()
            t2 = time.perf_counter()
            ta.append((t1 - t0) * 1e3)
            tb.append((t2 - t1) * 1e3)
        ma, mb = statistics.median(ta), statistics.median(tb)
        print("width %-2s (ran %2d) | A %s | B %s | A / B = %.2f  (%.1f M outputs/s)" % (c or "by n", eng.last_mul_window(), fmt(ta), fmt(tb), ma / mb, n / mb / 1e3), flush=True)

    # ---- 2. full-width uniform scalars ----
    gen = torch.Generator().manual_seed(0xBA7C4)
    d_s = torch.randint(0, 256, (cap, 32), dtype=torch.uint8, generator=gen).cuda()
    eng.generate_bases_device(0xC01D, 64, d_pts.data_ptr())
    fresh = bytes(d_pts[: 96 * 64].cpu().numpy().tobytes())
    print("# 2. full-width uniform scalars (all 256 bits random), base G; cold = n = 1 on a base the context has not seen")
    used = 0
    for c in WIDTHS:
        eng.set_mul_window(c)
        cold = []
        for _ in range(args.cold):
            base = fresh[96 * used : 96 * used + 96]
            used += 1
            t0 = time.perf_counter()
            eng.batch_mul_device(base, d_s.data_ptr(), 1, d_out.data_ptr(), d_inf.data_ptr())
            cold.append((time.perf_counter() - t0) * 1e3)
        warm1 = timed(lambda: eng.batch_mul_device(base, d_s.data_ptr(), 1, d_out.data_ptr(), d_inf.data_ptr()), args.repeats, 2)
        print("width %-2d | cold n = 1 %s | warm n = 1 %s | table build = cold - warm (medians) %.3f"
              % (c, fmt(cold), fmt(warm1), statistics.median(cold) - statistics.median(warm1)), flush=True)
        W = (256 + c - 1) // c
        for n in sizes:
            eng.batch_mul_device(g_bytes, d_s.data_ptr(), n, d_out.data_ptr(), d_inf.data_ptr())  # the table of G
            ts = timed(lambda: eng.batch_mul_device(g_bytes, d_s.data_ptr(), n, d_out.data_ptr(), d_inf.data_ptr()), args.repeats, args.warmup)
            m = statistics.median(ts)
            line = "width %-2d n = 2^%-2d | warm %s | %.2f M outputs/s" % (c, n.bit_length() - 1, fmt(ts), n / m / 1e3)
            if n == 1 << 20:
                floor = (W + 1) * n * MADD_PRODUCTS / PRODUCT_RATE * 1e3
                line += " | floor (%d additions x %d products at 71.4 G products/s) %.3f ms, measured / floor = %.2f" % (W + 1, MADD_PRODUCTS, floor, m / floor)
            print(line, flush=True)
    eng.set_mul_window(0)
    eng.close()


if __name__ == "__main__":
    main()
